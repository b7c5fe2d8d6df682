"""Device time of the temporal filter's stages (Renderer.TemporalDenoise, kernel_temporal.hip) next to the single-frame filter's
(Renderer.Denoise, kernel_denoise.hip), in one process.  One JSON line per scene x size:
  temporal_ms[K]   TemporalDenoise's own device time (guide pass + reprojection + variance + K passes), K = 0, 1, 5, with a
                   history in place (a still camera after two calls: every hit pixel reprojects, N < 4 only at first)
  first_call_ms    the same with K = 0 right after a reset: no reprojection taps, the 7x7 spatial variance on every pixel
  denoise_ms[K]    Denoise's device time (guide pass + K passes), K = 0, 1, 5
  guide_ms         device events around one guide pass
  var_pass_ms      (temporal_ms[5] - temporal_ms[0]) / 5, pass_ms = the same of Denoise, pass_ratio = their quotient
  reproject_ms     temporal_ms[0] - guide_ms - copy_ms, copy_ms = denoise_ms[0] - guide_ms (both copy 16 B per pixel each way);
                   reproject_gbps = 150 B per pixel (framebuffer 16, guide 32, previous key + colour + moments ~54, stores 48) over it
Medians of --reps after --warmup, the two filters' runs alternating.

  python tools/temporal_bench.py [--scenes a,b] [--sizes 1920x1080,3840x2160] [--reps 10] [--warmup 3] [--out file.jsonl]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell_box,suzanne_plane,dense_monkey,cs16_dust,room")
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--reps", type=int, default=10)
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

            def temporal(k):
                r.TemporalDenoise(cam, sc, iterations=k)
                return r.m_LastTemporalMs

            def first_call():
                r.resetTemporalHistory()
                r.TemporalDenoise(cam, sc, iterations=0)
                return r.m_LastTemporalMs

            def denoise(k):
                r.Denoise(cam, sc, k)
                return r.m_LastDenoiseMs

            runs = [("guide", guides), ("first", first_call)] + [(("t", k), lambda k=k: temporal(k)) for k in (0, 1, 5)] + \
                   [(("d", k), lambda k=k: denoise(k)) for k in (0, 1, 5)]
            samples = {key: [] for key, _ in runs}
            for _ in range(4):                   # (a history longer than 3 before anything is timed)
                temporal(0)
            for i in range(args.warmup + args.reps):
                for key, fn in runs:
                    if key == ("t", 0):          # ("first" has just reset the history)
                        for _ in range(4):
                            temporal(0)
                    v = fn()
                    if i >= args.warmup:
                        samples[key].append(v)
            med = {key: float(np.median(v)) for key, v in samples.items()}
            rec = dict(scene=name, width=W, height=H, device=torch.cuda.get_device_name(dev), reps=args.reps)
            rec["guide_ms"] = med["guide"]
            rec["first_call_ms"] = med["first"]
            rec["temporal_ms"] = {k: med[("t", k)] for k in (0, 1, 5)}
            rec["denoise_ms"] = {k: med[("d", k)] for k in (0, 1, 5)}
            rec["var_pass_ms"] = (med[("t", 5)] - med[("t", 0)]) / 5
            rec["pass_ms"] = (med[("d", 5)] - med[("d", 0)]) / 5
            rec["pass_ratio"] = rec["var_pass_ms"] / rec["pass_ms"]
            rec["copy_ms"] = med[("d", 0)] - med["guide"]
            rec["reproject_ms"] = med[("t", 0)] - med["guide"] - rec["copy_ms"]
            rec["reproject_gbps"] = 150.0 * W * H / (rec["reproject_ms"] * 1e-3) / 1e9 if rec["reproject_ms"] > 0 else None
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
