"""Throughput of the triangle overlap queries (Renderer.overlapTriangles / intersectsAny, kernel_tri_overlap.hip) next to
Renderer.overlapBoxes on each query's axis-aligned bounds (lo = qmin, hi = qmax), from the same process: the box query has the
same cull (up to the rounding of center -+ half) and visits the same nodes and leaf triangles, so the ratio isolates the 17-axis triangle-triangle test (at 5 waves
per SIMD) against the 13-axis box-triangle test (at 8).  One JSON line per scene x query size (vertices = a centre + uniform offsets in
+-size x the scene's extent):
  count              drt_renderer_overlap_triangles in mode LIST with capacity 0 on buffers made beforehand: the count pass alone
  any                the same in mode ANY
  table_k8           Renderer.overlapTriangles(k=8): one pass into [N, 8] tables (the offsets, the table and the counts are allocated inside)
  list               Renderer.overlapTriangles(): the count pass, the scan, the read-back of the total, the fill
  box_count, box_any, box_table_k8, box_list    the same four of the box query on the queries' bounds
ms = device events around --calls back-to-back queries, median of --reps after --warmup, per query; Mqueries/s = queries / ms / 1000;
Mtris/s = triangles listed / ms / 1000; `listed` and `box_listed` are the mean counts per query, whose ratio is the bounds' excess;
ratio_to_box = the box query's ms / the triangle query's ms.  The first --count queries are compared with the restatement
(tests/tri_overlap_ref.py).

  python tools/tri_overlap_bench.py [--scenes a,b] [--sizes 0.005,0.02,0.05] [--queries N] [--reps 9] [--warmup 2] [--calls 4] [--count 300] [--out file.jsonl]
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
from tests import overlap_ref as ov  # noqa: E402
from tests import tri_overlap_ref as tv  # noqa: E402
from tools.nearest_bench import timed  # noqa: E402
from tools.overlap_bench import load  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell_box,soup")
    ap.add_argument("--sizes", default="0.005,0.02,0.05")
    ap.add_argument("--queries", type=int, default=1 << 18)
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
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        no_room = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        for size in (float(s) for s in args.sizes.split(",")):
            host_q = (centers[:, None, :] + unit * np.float32(size * extent)).astype(np.float32)
            tris = torch.from_numpy(tv.pack(host_q)).to(dev)
            qmin, qmax = tv.bounds_of(host_q)
            boxes = torch.from_numpy(ov.from_corners(qmin, qmax)).to(dev)

            def tri_raw(mode):
                rc = drt._lib.drt_renderer_overlap_triangles(r._h, sc._h, tris.data_ptr(), no_room.data_ptr(), None, 0, counts.data_ptr(), n, mode, stream)
                assert rc == drt.OK, drt._lib.drt_last_error()

            def box_raw(mode):
                rc = drt._lib.drt_renderer_overlap_boxes(r._h, sc._h, boxes.data_ptr(), no_room.data_ptr(), None, 0, counts.data_ptr(), n, mode, stream)
                assert rc == drt.OK, drt._lib.drt_last_error()

            tri_raw(drt.OVERLAP_LIST)
            listed = float(counts.double().mean().item())
            longest = int(counts.max().item())
            box_raw(drt.OVERLAP_LIST)
            box_listed = float(counts.double().mean().item())
            row = {"scene": name, "triangles": len(g.v0), "bvh_depth": sc.bvh_depth, "queries": n, "size_over_extent": size,
                   "listed": round(listed, 3), "longest_list": longest, "box_listed": round(box_listed, 3)}
            jobs = [("count", lambda: tri_raw(drt.OVERLAP_LIST), listed), ("any", lambda: tri_raw(drt.OVERLAP_ANY), None),
                    ("table_k8", lambda: r.overlapTriangles(sc, tris, k=8), None), ("list", lambda: r.overlapTriangles(sc, tris), listed),
                    ("box_count", lambda: box_raw(drt.OVERLAP_LIST), box_listed), ("box_any", lambda: box_raw(drt.OVERLAP_ANY), None),
                    ("box_table_k8", lambda: r.overlapBoxes(sc, boxes, k=8), None), ("box_list", lambda: r.overlapBoxes(sc, boxes), box_listed)]
            for key, fn, per_query in jobs:
                ms, t_lo, t_hi = timed(fn, args.reps, args.warmup, args.calls)
                row[key] = {"ms": round(ms, 4), "ms_min": round(t_lo, 4), "ms_max": round(t_hi, 4), "mqueries_per_s": round(n / ms / 1000.0, 1)}
                if per_query is not None:
                    row[key]["mtris_per_s"] = round(n * per_query / ms / 1000.0, 1)
            for key in ("count", "any", "table_k8", "list"):
                row[key]["ratio_to_box"] = round(row["box_" + key]["ms"] / row[key]["ms"], 3)
            m = min(args.count, n)
            ref, ref_counts = tv.overlap(g, host_q[:m], 8)
            got = r.overlapTriangles(sc, host_q[:m], k=8)
            row["bit_equal_to_restatement"] = bool(np.array_equal(got.prim.reshape(-1), ref) and np.array_equal(got.count.view(np.uint32), ref_counts))
            line = json.dumps(row)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
