"""Throughput of the nearest-surface query (Renderer.nearest, kernel_nearest.hip).  One JSON line per scene x point set:
  near     points within 1 % of the scene's extent of a surface (random points on random triangles, offset in a random direction)
  in_box   uniform in the scene's box
  far      uniform in a box ten times larger about the same centre
and, for scale, one line with traceRays on the same scene's 1920x1080 frame-1 camera rays.
ms = device events around --calls back-to-back queries, median of --reps after --warmup, per query; Mqueries/s = points / ms / 1000.
`visits` = mean nodes visited per point, counted by the float32 restatement (tests/nearest_ref.py) on the first --count points.

  python tools/nearest_bench.py [--scenes a,b] [--points N] [--reps 15] [--warmup 3] [--calls 16] [--count 2000] [--out file.jsonl]
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
from tests import nearest_ref as nr  # noqa: E402
from tests.scenes import SCENES, scene_path  # noqa: E402
from tools.ray_query_bench import camera_rays  # noqa: E402


def timed(fn, reps, warmup, calls):
    """Median ms of one call: device events around `calls` calls in a row (a single query of 10^6 points is a fraction of a ms)."""
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / calls)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="dense_monkey,cs16_dust")
    ap.add_argument("--points", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--count", type=int, default=2000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = open(args.out, "a") if args.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for name in args.scenes.split(","):
        _, pos, fwd, _ = SCENES[name]
        sc = drt.Scene()
        sc.loadGLTFmodel(scene_path(name))
        b = drt.BVHBuilder()
        b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
        b.buildIterative(sc)
        g = nr.from_product(sc)
        rng = np.random.default_rng(1234)
        n = args.points
        lo, hi = nr.bounds(g)
        d = rng.normal(size=(n, 3))
        d *= rng.uniform(0, 0.01 * float((hi - lo).max()), (n, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
        sets = {"near": (nr.surface_points(g, n, rng, offset=0.0) + d).astype(np.float32), "in_box": nr.box_points(g, n, rng),
                "far": nr.box_points(g, n, rng, 10.0)}
        r = drt.Renderer(0)
        for set_name, pts in sets.items():
            p = torch.cat([torch.from_numpy(pts), torch.full((n, 1), float("inf"))], dim=1).to(dev)      # packed: nothing but the query is timed
            ms, t_lo, t_hi = timed(lambda: r.nearest(sc, p), args.reps, args.warmup, args.calls)
            visits = np.zeros(min(args.count, n), np.int64)
            ref = nr.nearest(g, pts[:len(visits)], visits=visits)
            got = r.nearest(sc, pts[:len(visits)])
            same = all(np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)) for a, b in zip(got, ref))
            emit({"scene": name, "triangles": len(g.v0), "bvh_depth": sc.bvh_depth, "points_set": set_name, "points": n, "ms": round(ms, 4),
                  "ms_min": round(t_lo, 4), "ms_max": round(t_hi, 4), "mqueries_per_s": round(n / ms / 1000.0, 1),
                  "visits_per_point": round(float(visits.mean()), 1), "visits_max": int(visits.max()), "bit_equal_to_restatement": bool(same)})
        cam = drt.Camera(pos)
        cam.m_Forward_dir = np.array(fwd, np.float32)
        org, dirs = camera_rays(cam, dev)
        rays = torch.empty((len(org), 8), dtype=torch.float32, device=dev)
        rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = org, 0.0, dirs, drt.FLT_MAX
        ms, t_lo, t_hi = timed(lambda: r.traceRays(sc, rays), args.reps, args.warmup, args.calls)
        emit({"scene": name, "points_set": "traceRays, 1920x1080 camera rays", "points": len(org), "ms": round(ms, 4), "ms_min": round(t_lo, 4),
              "ms_max": round(t_hi, 4), "mqueries_per_s": round(len(org) / ms / 1000.0, 1)})


if __name__ == "__main__":
    main()
