"""Throughput of the sphere cast (Renderer.sphereCast, kernel_sphere_cast.hip).  One JSON line per scene x radius: 2^20 casts of the
four kinds of tests/sweep_ref.cast_sets (aimed at surfaces, starting near surfaces, parallel to faces, from far outside; tmin 0 or
positive, tmax infinite or finite) with one radius for all -- 0, 1 % and 10 % of the scene's extent -- and, next to each figure,
traceRays on the same packed rays as the yardstick.
ms = device events around --calls back-to-back queries, median of --reps after --warmup, per query; Mqueries/s = casts / ms / 1000.
`visits` = mean nodes visited per cast, counted by the float32 restatement (tests/sweep_ref.py) on the first --count casts, which
are also compared with the device's records bit for bit.

  python tools/sphere_cast_bench.py [--scenes a,b] [--casts N] [--reps 15] [--warmup 3] [--calls 8] [--count 1000] [--out file.jsonl]
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
from tests import sweep_ref as sw  # noqa: E402
from tests.scenes import scene_path  # noqa: E402
from tools.nearest_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell_box,suzanne_plane,dense_monkey")
    ap.add_argument("--casts", type=int, default=1 << 20)
    ap.add_argument("--radii", default="0,0.01,0.1")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--count", type=int, default=1000)
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
        sc = drt.Scene()
        sc.loadGLTFmodel(scene_path(name))
        b = drt.BVHBuilder()
        b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
        b.buildIterative(sc)
        g = nr.from_product(sc)
        lo, hi = nr.bounds(g)
        ext = float((hi - lo).max())
        n = args.casts
        org, dirs, _, tmin, tmax = sw.cast_sets(g, n, np.random.default_rng(1234))
        perm = np.random.default_rng(1).permutation(n)                          # the four kinds mixed within every wave
        org, dirs, tmin, tmax = org[perm], dirs[perm], tmin[perm], tmax[perm]
        rays = torch.from_numpy(np.ascontiguousarray(np.concatenate([org, tmin[:, None], dirs, tmax[:, None]], axis=1))).to(dev)
        r = drt.Renderer(0)
        ray_ms, _, _ = timed(lambda: r.traceRays(sc, rays), args.reps, args.warmup, args.calls)
        for frac in (float(x) for x in args.radii.split(",")):
            radius = np.float32(frac * ext)
            radii = torch.full((n,), float(radius), dtype=torch.float32, device=dev)
            ms, t_lo, t_hi = timed(lambda: r.sphereCast(sc, rays, radius=radii), args.reps, args.warmup, args.calls)
            k = min(args.count, n)
            visits = np.zeros(k, np.int64)
            ref = sw.sphere_cast(g, org[:k], dirs[:k], radius, tmin[:k], tmax[:k], visits=visits)
            got = r.sphereCast(sc, org[:k], dirs[:k], float(radius), tmin[:k], tmax[:k])
            same = all(np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)) for a, b in zip(got, ref))
            emit({"scene": name, "triangles": len(g.v0), "bvh_depth": sc.bvh_depth, "casts": n, "radius_of_extent": frac, "ms": round(ms, 4),
                  "ms_min": round(t_lo, 4), "ms_max": round(t_hi, 4), "mqueries_per_s": round(n / ms / 1000.0, 1),
                  "trace_rays_ms": round(ray_ms, 4), "trace_rays_mqueries_per_s": round(n / ray_ms / 1000.0, 1), "ratio_to_trace_rays": round(ray_ms / ms, 3),
                  "hit_fraction": round(float((ref.prim >= 0).mean()), 3), "visits_per_cast": round(float(visits.mean()), 1), "visits_max": int(visits.max()),
                  "bit_equal_to_restatement": bool(same)})


if __name__ == "__main__":
    main()
