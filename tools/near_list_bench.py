"""Throughput of the nearest-triangle lists (Renderer.kNearest / withinRadius, kernel_near_list.hip) next to Renderer.nearest on the same
points from the same process: nearest is the same traversal with one record in registers, hence the yardstick.  One JSON line per
scene x point set (tools/nearest_bench.py's sets: near, in_box, far):
  nearest            Renderer.nearest
  k_nearest_k1/4/8   Renderer.kNearest (the offsets, the [N, k] tables and the counts are allocated inside the call)
  raw_k1/4/8         drt_renderer_nearest_list in mode K alone on buffers made beforehand, offsets = k * arange(N + 1), surf given
  within_1/10        Renderer.withinRadius (count pass, scan, the read-back of the total, fill) at the radius whose mean count over the
                     first --probe points is nearest 1 / 10 (bisection with the count pass); `radius` and `mean_count` say what it found
  count_1/10         the count pass alone at those radii: mode GATHER with capacity 0
The far set has no within_* figures: a mean count of 1 or 10 there is a few points inside the mesh's box with lists of thousands and
the rest with none, which measures the one-record-per-step insert at a length it is not meant for.
ms = device events around --calls back-to-back queries, median of --reps after --warmup, per query; Mpoints/s = points / ms / 1000;
ratio = nearest's ms / the query's ms.  The first --count points at k = 4 are compared with the restatement (tests/near_list_ref.py).

  python tools/near_list_bench.py [--scenes a,b] [--sets near,in_box,far] [--points N] [--reps 9] [--warmup 2] [--calls 4] [--count 500] [--out file.jsonl]
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
from tests import near_list_ref as nl  # noqa: E402
from tests import nearest_ref as nr  # noqa: E402
from tests.scenes import scene_path  # noqa: E402
from tools.nearest_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="dense_monkey,cs16_dust")
    ap.add_argument("--sets", default="near,in_box,far")
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--count", type=int, default=500)
    ap.add_argument("--probe", type=int, default=1 << 16)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = open(args.out, "a") if args.out else None
    n = args.points
    for name in args.scenes.split(","):
        sc = drt.Scene()
        sc.loadGLTFmodel(scene_path(name))
        b = drt.BVHBuilder()
        b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
        b.buildIterative(sc)
        g = nr.from_product(sc)
        rng = np.random.default_rng(1234)
        lo, hi = nr.bounds(g)
        extent = float((hi - lo).max())
        d = rng.normal(size=(n, 3))
        d *= rng.uniform(0, 0.01 * extent, (n, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
        sets = {"near": (nr.surface_points(g, n, rng, offset=0.0) + d).astype(np.float32), "in_box": nr.box_points(g, n, rng),
                "far": nr.box_points(g, n, rng, 10.0)}
        r = drt.Renderer(0)
        stream = torch.cuda.current_stream(dev).cuda_stream
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        no_room = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        bufs = {k: ((torch.arange(n + 1, dtype=torch.int64, device=dev) * k).to(torch.int32), torch.empty((n * k, 4), dtype=torch.float32, device=dev),
                    torch.empty((n * k, 4), dtype=torch.float32, device=dev)) for k in (1, 4, 8)}
        for set_name in args.sets.split(","):
            pts = sets[set_name]
            xyz = torch.from_numpy(pts).to(dev)
            p = torch.cat([xyz, torch.full((n, 1), float("inf"), device=dev)], dim=1).contiguous()   # packed: nothing but the query is timed

            def raw(points, m, offsets, near, surf, capacity, cnt, mode):
                ptr = lambda x: None if x is None else x.data_ptr()
                rc = drt._lib.drt_renderer_nearest_list(r._h, sc._h, points.data_ptr(), offsets.data_ptr(), ptr(near), ptr(surf), capacity, ptr(cnt), m,
                                                        mode, stream)
                assert rc == drt.OK, drt._lib.drt_last_error()

            def mean_count(radius, q):
                raw(q, len(q), no_room, None, None, 0, counts, drt.NEAR_GATHER)
                return float(counts[:len(q)].float().mean().item())

            def radius_for(target):
                """The radius whose mean count over the probe points is nearest `target`: bisection in log space."""
                q = p[:min(args.probe, n)].clone()
                a, c = 1e-5 * extent, 20.0 * extent
                for _ in range(24):
                    mid = float(np.sqrt(a * c))
                    q[:, 3] = mid
                    if mean_count(mid, q) < target:
                        a = mid
                    else:
                        c = mid
                q[:, 3] = c
                return c, mean_count(c, q)

            row = {"scene": name, "triangles": len(g.v0), "bvh_depth": sc.bvh_depth, "points_set": set_name, "points": n}
            jobs = [("nearest", lambda: r.nearest(sc, p))]
            for k in (1, 4, 8):
                jobs.append(("k_nearest_k%d" % k, lambda k=k: r.kNearest(sc, p, k=k)))
                jobs.append(("raw_k%d" % k, lambda k=k: raw(p, n, bufs[k][0], bufs[k][1], bufs[k][2], n * k, counts, drt.NEAR_K)))
            for target in (1, 10) if set_name != "far" else ():
                radius, found = radius_for(target)
                pr = p.clone()
                pr[:, 3] = radius
                rad = pr[:, 3].contiguous()
                row["within_%d_radius" % target] = {"radius": round(radius, 6), "radius_over_extent": round(radius / extent, 6), "mean_count": round(found, 3)}
                jobs.append(("within_%d" % target, lambda rad=rad: r.withinRadius(sc, xyz, rad)))
                jobs.append(("count_%d" % target, lambda pr=pr: raw(pr, n, no_room, None, None, 0, counts, drt.NEAR_GATHER)))
            for key, fn in jobs:
                ms, t_lo, t_hi = timed(fn, args.reps, args.warmup, args.calls)
                row[key] = {"ms": round(ms, 4), "ms_min": round(t_lo, 4), "ms_max": round(t_hi, 4), "mpoints_per_s": round(n / ms / 1000.0, 1)}
            for key, _ in jobs[1:]:
                row[key]["ratio_to_nearest"] = round(row["nearest"]["ms"] / row[key]["ms"], 3)
            m = min(args.count, n)
            ref, ref_counts = nl.near_list(g, pts[:m], np.inf, 4, nl.K)
            got = r.kNearest(sc, pts[:m], k=4)
            same = all(np.array_equal(np.ascontiguousarray(getattr(got, f)).reshape(np.shape(getattr(ref, f))).view(np.uint32),
                                      np.ascontiguousarray(getattr(ref, f)).view(np.uint32)) for f in ref._fields)
            row["bit_equal_to_restatement"] = bool(same and np.array_equal(got.count.view(np.uint32), ref_counts))
            line = json.dumps(row)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
