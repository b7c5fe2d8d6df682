"""Device time of the guide pass and of the a-trous filter (Renderer.renderGuides / Denoise, kernel_denoise.hip).  One JSON line
per scene x size:
  guide_ms       device events around one frame-1 guide pass (renderGuides, as_torch) on the current torch stream
  denoise_ms[K]  Renderer.Denoise's own device time (guide pass + K filter passes), K = 0, 1, 5
  pass_ms        (denoise_ms[5] - denoise_ms[0]) / 5: one filter pass
  pass_ms_first  denoise_ms[1] - denoise_ms[0]: the step-1 pass alone
Medians of --reps after --warmup.  The framebuffer is one rendered frame of the scene (the filter's cost does not depend on it).

  python tools/denoise_bench.py [--scenes a,b] [--sizes 1920x1080,3840x2160] [--reps 20] [--warmup 3] [--out file.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import dustraytracer_amd as drt  # noqa: E402
from tests.scenes import SCENES, scene_path  # noqa: E402


def median_ms(fn, reps, warmup):
    out = []
    for i in range(warmup + reps):
        v = fn()
        if i >= warmup:
            out.append(v)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell_box,suzanne_plane,dense_monkey,cs16_dust,room")
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = open(args.out, "w") if args.out else None
    for name in args.scenes.split(","):
        _, pos, fwd, depth = SCENES[name]
        sc = drt.Scene()
        sc.loadGLTFmodel(scene_path(name))
        b = drt.BVHBuilder()
        b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
        b.buildIterative(sc)
        cam = drt.Camera(pos)
        cam.m_Forward_dir = np.array(fwd, np.float32)
        for size in args.sizes.split(","):
            W, H = (int(v) for v in size.split("x"))
            r = drt.Renderer(0)
            r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=depth)
            r.ResizeBuffer(W, H)
            r.Render(cam, sc)

            def guides():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r.renderGuides(cam, sc, 1, as_torch=True)
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1)

            def denoise(k):
                def run():
                    r.Denoise(cam, sc, k)
                    return r.m_LastDenoiseMs
                return run

            rec = dict(scene=name, width=W, height=H, device=torch.cuda.get_device_name(dev))
            rec["guide_ms"] = median_ms(guides, args.reps, args.warmup)
            rec["guide_mrays_per_s"] = W * H / rec["guide_ms"] / 1e3
            rec["denoise_ms"] = {k: median_ms(denoise(k), args.reps, args.warmup) for k in (0, 1, 5)}
            rec["pass_ms"] = (rec["denoise_ms"][5] - rec["denoise_ms"][0]) / 5
            rec["pass_ms_first"] = rec["denoise_ms"][1] - rec["denoise_ms"][0]
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del r
    if out:
        out.close()


if __name__ == "__main__":
    main()
