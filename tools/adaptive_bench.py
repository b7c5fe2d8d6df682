"""Cost of adaptive sampling against the frame loop (GPU): m_LastAdaptiveMs of RenderAdaptive(spp) against RenderBatch(spp frames) on
the same scene, size and depth, alternating in one process; one JSON line.  The adaptive call is timed twice per round: the first
call after a reset (uniform counts) and the second (ragged counts).  Per-kernel times: run it under a kernel trace.

    python tools/adaptive_bench.py [--scene cornell_box] [--size 1920 1080] [--spp 8] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dustraytracer_amd as drt  # noqa: E402
from tests.scenes import SCENES, scene_path  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cornell_box")
    ap.add_argument("--size", type=int, nargs=2, default=[1920, 1080])
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    _, pos, fwd, depth = SCENES[a.scene]
    sc = drt.Scene()
    sc.loadGLTFmodel(scene_path(a.scene))
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
    b.buildIterative(sc)
    cam = drt.Camera(pos)
    cam.m_Forward_dir = np.array(fwd, np.float32)
    r = drt.Renderer(0)
    r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=depth, max_samples=1 << 30)
    r.ResizeBuffer(*a.size)
    batch, first, second, infos = [], [], [], []
    for i in range(a.rounds + 1):                    # round 0 warms up
        r.resetAccumulationBuffer()
        t = r.RenderBatch(cam, sc, a.spp)
        r.resetAdaptive()
        i1 = r.RenderAdaptive(cam, sc, spp=a.spp)
        i2 = r.RenderAdaptive(cam, sc, spp=a.spp)
        if i:
            batch.append(t); first.append(i1.ms); second.append(i2.ms)
            infos = [i1, i2]
    med = statistics.median
    print(json.dumps(dict(scene=a.scene, width=a.size[0], height=a.size[1], depth=depth, spp=a.spp, rounds=a.rounds, kernel=r.kernelInfo(),
                          render_batch_ms=med(batch), render_batch_ms_all=batch, adaptive_first_ms=med(first), adaptive_first_ms_all=first,
                          adaptive_second_ms=med(second), adaptive_second_ms_all=second,
                          second_call=dict(samples=infos[1].samples, active_pixels=infos[1].active_pixels, max_count=infos[1].max_count))))


if __name__ == "__main__":
    main()
