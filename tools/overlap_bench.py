"""Throughput of the box overlap queries (Renderer.overlapBoxes / overlapsAny, kernel_overlap.hip) next to Renderer.withinRadius on the
same centres with the circumscribed radius, from the same process: withinRadius is the closest existing query -- the same traversal
shape, and a superset of the volume -- hence the yardstick.  One JSON line per scene x box size (half extent = --sizes x the scene's
extent, cubes; every other box turned about a random axis):
  count              drt_renderer_overlap_boxes in mode LIST with capacity 0 on buffers made beforehand: the count pass alone
  any                the same in mode ANY
  table_k8           Renderer.overlapBoxes(k=8): one pass into [N, 8] tables (the offsets, the table and the counts are allocated inside)
  list               Renderer.overlapBoxes(): the count pass, the scan, the read-back of the total, the fill
  sphere_count       drt_renderer_nearest_list in mode GATHER with capacity 0 on the same centres, radius = |half| (the circumscribed sphere)
  sphere_list        Renderer.withinRadius on them
ms = device events around --calls back-to-back queries, median of --reps after --warmup, per query; Mboxes/s = boxes / ms / 1000;
Mtris/s = triangles listed / ms / 1000; `listed` and `sphere_listed` are the mean counts per box, whose ratio is the sphere's excess;
ratio_to_sphere = the sphere query's ms / the box query's ms.  The first --count boxes are compared with the restatement
(tests/overlap_ref.py).

  python tools/overlap_bench.py [--scenes a,b] [--sizes 0.005,0.02,0.05] [--boxes N] [--reps 9] [--warmup 2] [--calls 4] [--count 300] [--out file.jsonl]
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
from tests import ray_query_ref as rq  # noqa: E402
from tests.scenes import scene_path  # noqa: E402
from tools.nearest_bench import timed  # noqa: E402


def load(name):
    if name == "soup":
        sc, _ = rq.programmatic_scene(drt, *rq.soup(3000, 5), 2, 8)
        return sc
    sc = drt.Scene()
    sc.loadGLTFmodel(scene_path(name))
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
    b.buildIterative(sc)
    return sc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell_box,soup")
    ap.add_argument("--sizes", default="0.005,0.02,0.05")
    ap.add_argument("--boxes", type=int, default=1 << 18)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--count", type=int, default=300)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = open(args.out, "a") if args.out else None
    n = args.boxes
    for name in args.scenes.split(","):
        sc = load(name)
        g = nr.from_product(sc)
        rng = np.random.default_rng(1234)
        lo, hi = nr.bounds(g)
        extent = float((hi - lo).max())
        centers = np.concatenate([nr.surface_points(g, n // 2, rng), nr.box_points(g, n - n // 2, rng)]).astype(np.float32)
        rot, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
        axes = rot.astype(np.float32)
        axes[::2] = np.eye(3, dtype=np.float32)
        r = drt.Renderer(0)
        stream = torch.cuda.current_stream(dev).cuda_stream
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        no_room = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        for size in (float(s) for s in args.sizes.split(",")):
            half = np.float32(size * extent)
            host_boxes = ov.pack(centers, half, axes)
            boxes = torch.from_numpy(host_boxes).to(dev)
            radius = np.float32(np.sqrt(3.0)) * half                                # the circumscribed sphere
            xyz = torch.from_numpy(centers).to(dev)
            p = torch.cat([xyz, torch.full((n, 1), float(radius), device=dev)], dim=1).contiguous()
            rad = p[:, 3].contiguous()

            def box_raw(mode):
                rc = drt._lib.drt_renderer_overlap_boxes(r._h, sc._h, boxes.data_ptr(), no_room.data_ptr(), None, 0, counts.data_ptr(), n, mode, stream)
                assert rc == drt.OK, drt._lib.drt_last_error()

            def sphere_raw():
                rc = drt._lib.drt_renderer_nearest_list(r._h, sc._h, p.data_ptr(), no_room.data_ptr(), None, None, 0, counts.data_ptr(), n,
                                                        drt.NEAR_GATHER, stream)
                assert rc == drt.OK, drt._lib.drt_last_error()

            box_raw(drt.OVERLAP_LIST)
            listed = float(counts.double().mean().item())
            sphere_raw()
            sphere_listed = float(counts.double().mean().item())
            row = {"scene": name, "triangles": len(g.v0), "bvh_depth": sc.bvh_depth, "boxes": n, "half_over_extent": size,
                   "listed": round(listed, 3), "sphere_listed": round(sphere_listed, 3)}
            jobs = [("count", lambda: box_raw(drt.OVERLAP_LIST), listed, None), ("any", lambda: box_raw(drt.OVERLAP_ANY), None, None),
                    ("table_k8", lambda: r.overlapBoxes(sc, boxes, k=8), None, None), ("list", lambda: r.overlapBoxes(sc, boxes), listed, None),
                    ("sphere_count", sphere_raw, sphere_listed, None), ("sphere_list", lambda: r.withinRadius(sc, xyz, rad), sphere_listed, None)]
            for key, fn, per_box, _ in jobs:
                ms, t_lo, t_hi = timed(fn, args.reps, args.warmup, args.calls)
                row[key] = {"ms": round(ms, 4), "ms_min": round(t_lo, 4), "ms_max": round(t_hi, 4), "mboxes_per_s": round(n / ms / 1000.0, 1)}
                if per_box is not None:
                    row[key]["mtris_per_s"] = round(n * per_box / ms / 1000.0, 1)
            for key, sphere in (("count", "sphere_count"), ("any", "sphere_count"), ("table_k8", "sphere_list"), ("list", "sphere_list")):
                row[key]["ratio_to_sphere"] = round(row[sphere]["ms"] / row[key]["ms"], 3)
            m = min(args.count, n)
            ref, ref_counts = ov.overlap(g, host_boxes[:m], 8)
            got = r.overlapBoxes(sc, host_boxes[:m], k=8)
            row["bit_equal_to_restatement"] = bool(np.array_equal(got.prim.reshape(-1), ref) and np.array_equal(got.count.view(np.uint32), ref_counts))
            line = json.dumps(row)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
