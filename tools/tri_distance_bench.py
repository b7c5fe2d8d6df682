"""Throughput of the triangle distance queries (Renderer.triangleDistance / withinDistance, kernel_tri_distance.hip) next to two
yardsticks from the same process at the same commit: Renderer.nearest on each query's centroid -- the same bound-shrinking search with
a point-triangle test at the leaves, at 8 waves per SIMD -- and drt_renderer_overlap_triangles in count mode on the same queries --
the seventeen-axis predicate alone, at 5 waves per SIMD, over the nodes the queries' bounds touch.  One JSON line per scene x query
size (vertices = a centre + uniform offsets in +-size x the scene's extent; the centres are half near surfaces, half in the scene's box):
  nearest_mode       drt_renderer_triangle_distance in mode NEAREST with max_dist NULL on buffers made beforehand
  within             the same in mode ANY with max_dist = --within x the scene's extent for every query
  point_nearest      drt_renderer_nearest on the centroids, max_dist infinite
  overlap_count      drt_renderer_overlap_triangles in mode LIST with capacity 0
ms = device events around --calls back-to-back queries, median of --reps after --warmup, per query; Mqueries/s = queries / ms / 1000;
ratio_to_point_nearest and ratio_to_overlap_count = the yardstick's ms / the distance query's ms (below 1: the distance query is
slower).  `touching` is the share of queries with d2 = 0, `found_within` the share the ANY mode finds.  The first --count records of each
timed set are compared with the restatement (tests/tri_distance_ref.py), bit for bit.  Measurements, not pass marks.

  python tools/tri_distance_bench.py [--scenes a,b] [--sizes 0.005,0.02,0.05] [--queries N] [--within 0.01] [--reps 9] [--warmup 2] [--calls 4] [--count 300] [--out file.jsonl]
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
from tests import tri_distance_ref as td  # noqa: E402
from tests import tri_overlap_ref as tv  # noqa: E402
from tools.nearest_bench import timed  # noqa: E402
from tools.overlap_bench import load  # noqa: E402


def same(got, want):
    eq = got.view(np.uint32) == want.view(np.uint32)
    eq[:, 3] |= np.isnan(got[:, 3]) & np.isnan(want[:, 3])
    return bool(eq.all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell_box,soup")
    ap.add_argument("--sizes", default="0.005,0.02,0.05")
    ap.add_argument("--queries", type=int, default=1 << 18)
    ap.add_argument("--within", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--count", type=int, default=300)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = open(args.out, "a") if args.out else None
    n = args.queries
    for name in args.scenes.split(","):
        sc = load(name)
        g = nr.from_product(sc)
        rng = np.random.default_rng(1234)
        lo, hi = nr.bounds(g)
        extent = float((hi - lo).max())
        centers = np.concatenate([nr.surface_points(g, n // 2, rng), nr.box_points(g, n - n // 2, rng)]).astype(np.float32)
        unit = rng.uniform(-1, 1, (n, 3, 3)).astype(np.float32)
        r = drt.Renderer(0)
        stream = torch.cuda.current_stream(dev).cuda_stream
        records = torch.empty((n, 12), dtype=torch.float32, device=dev)
        point_out = torch.empty((n, 8), dtype=torch.float32, device=dev)
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        no_room = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        within = np.float32(args.within * extent)
        md = torch.full((n,), float(within), dtype=torch.float32, device=dev)
        for size in (float(s) for s in args.sizes.split(",")):
            host_q = (centers[:, None, :] + unit * np.float32(size * extent)).astype(np.float32)
            tris = torch.from_numpy(tv.pack(host_q)).to(dev)
            points = torch.empty((n, 4), dtype=torch.float32, device=dev)
            points[:, 0:3] = torch.from_numpy(host_q.mean(axis=1).astype(np.float32)).to(dev)
            points[:, 3] = float("inf")

            def distance(mode):
                rc = drt._lib.drt_renderer_triangle_distance(r._h, sc._h, tris.data_ptr(), md.data_ptr() if mode == drt.TRIDIST_ANY else None,
                                                             records.data_ptr(), n, mode, stream)
                assert rc == drt.OK, drt._lib.drt_last_error()

            def point_nearest():
                rc = drt._lib.drt_renderer_nearest(r._h, sc._h, points.data_ptr(), point_out.data_ptr(), n, stream)
                assert rc == drt.OK, drt._lib.drt_last_error()

            def overlap_count():
                rc = drt._lib.drt_renderer_overlap_triangles(r._h, sc._h, tris.data_ptr(), no_room.data_ptr(), None, 0, counts.data_ptr(), n,
                                                             drt.OVERLAP_LIST, stream)
                assert rc == drt.OK, drt._lib.drt_last_error()

            row = {"scene": name, "triangles": len(g.v0), "bvh_depth": sc.bvh_depth, "queries": n, "size_over_extent": size,
                   "within_over_extent": args.within}
            m = min(args.count, n)
            checks = {}
            for key, mode, fn in (("nearest_mode", drt.TRIDIST_NEAREST, lambda: distance(drt.TRIDIST_NEAREST)),
                                  ("within", drt.TRIDIST_ANY, lambda: distance(drt.TRIDIST_ANY)), ("point_nearest", None, point_nearest),
                                  ("overlap_count", None, overlap_count)):
                ms, t_lo, t_hi = timed(fn, args.reps, args.warmup, args.calls)
                row[key] = {"ms": round(ms, 4), "ms_min": round(t_lo, 4), "ms_max": round(t_hi, 4), "mqueries_per_s": round(n / ms / 1000.0, 1)}
                if mode is not None:
                    torch.cuda.synchronize()
                    got = records[:m].cpu().numpy()
                    prim = records.view(torch.int32)[:, 7]
                    if mode == drt.TRIDIST_NEAREST:
                        row["touching"] = round(float(((prim >= 0) & (records[:, 3] == 0)).double().mean().item()), 4)
                    else:
                        row["found_within"] = round(float((prim >= 0).double().mean().item()), 4)
                    ref = td.distance(g, host_q[:m], None if mode == drt.TRIDIST_NEAREST else np.full(m, within, np.float32), mode)
                    checks[key] = same(got, td.records(ref))
            for key in ("nearest_mode", "within"):
                row[key]["ratio_to_point_nearest"] = round(row["point_nearest"]["ms"] / row[key]["ms"], 3)
                row[key]["ratio_to_overlap_count"] = round(row["overlap_count"]["ms"] / row[key]["ms"], 3)
            row["bit_equal_to_restatement"] = checks
            line = json.dumps(row)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
