"""Device time of the hit-list queries (Renderer.firstHits / listHits, kernel_list_hits.hip) next to Renderer.crossings on the same
rays from the same run: crossings is the same traversal without the list, hence the floor.  One JSON line per scene:
  crossings          Renderer.crossings
  first_hits_k4/k8   Renderer.firstHits (the offsets, the [N, k] table and the counts are allocated inside the call)
  raw_k4/k8          drt_renderer_list_hits alone on buffers made beforehand, offsets = k * arange(N + 1)
  fill               listHits' second pass alone: drt_renderer_list_hits on the exclusive scan of crossings' counts, counts = NULL
  count_only         drt_renderer_list_hits with hits = NULL (every capacity 0): the traversal plus one 4-byte store per ray
Rays: tests/ray_query_ref.surface_rays (seeded), tmin = 0, tmax = +inf, packed on the device beforehand.  ms = device events around
--calls back-to-back queries, median of --reps after --warmup, per query; Mrays/s = rays / ms / 1000.  The first --count rays are
compared with the restatement (tests/hits_ref.py).

  python tools/list_hits_bench.py [--scenes cornell_box,torus] [--rays N] [--reps 15] [--warmup 3] [--calls 8] [--count 1000] [--out file.jsonl]
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
from tests import hits_ref as hr  # noqa: E402
from tests import inside_ref as ir  # noqa: E402
from tests import ray_query_ref as rq  # noqa: E402
from tests.scenes import scene_path  # noqa: E402
from tools.nearest_bench import timed  # noqa: E402


def load(name):
    if name == "torus":
        return rq.programmatic_scene(drt, *ir.streams(ir.torus()), 4, 8)[0]
    sc = drt.Scene()
    sc.loadGLTFmodel(scene_path(name))
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
    b.buildIterative(sc)
    return sc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell_box,torus")
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--count", type=int, default=1000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = open(args.out, "a") if args.out else None
    n = args.rays
    for name in args.scenes.split(","):
        sc = load(name)
        osc = ir.product_scene(sc)
        org, dirs = rq.surface_rays(osc, n, np.random.default_rng(1234))
        rays = torch.empty((n, 8), dtype=torch.float32)
        rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = torch.from_numpy(org), 0.0, torch.from_numpy(dirs), float("inf")
        rays = rays.to(dev)                                                       # packed: nothing but the query is timed
        r = drt.Renderer(0)
        stream = torch.cuda.current_stream(dev).cuda_stream
        count = r.crossings(sc, rays).count
        splits = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        splits[1:] = torch.cumsum(count.to(torch.int64), dim=0)
        total = int(splits[-1].item())
        splits = splits.to(torch.int32)
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        bufs = {k: ((torch.arange(n + 1, dtype=torch.int64, device=dev) * k).to(torch.int32), torch.empty((n * k, 4), dtype=torch.float32, device=dev))
                for k in (4, 8)}
        csr = torch.empty((max(total, 1), 4), dtype=torch.float32, device=dev)

        def raw(offsets, hits, capacity, cnt):
            rc = drt._lib.drt_renderer_list_hits(r._h, sc._h, rays.data_ptr(), offsets.data_ptr(), None if hits is None else hits.data_ptr(), capacity,
                                                 None if cnt is None else cnt.data_ptr(), n, stream)
            assert rc == drt.OK, drt._lib.drt_last_error()

        row = {"scene": name, "triangles": len(osc.tris), "bvh_depth": sc.bvh_depth, "rays": n, "hits_per_ray": round(total / n, 3),
               "max_hits": int(count.max().item()), "truncated_at_4": round(float((count > 4).float().mean().item()), 5),
               "truncated_at_8": round(float((count > 8).float().mean().item()), 5)}
        for key, fn in (("crossings", lambda: r.crossings(sc, rays)),
                        ("first_hits_k4", lambda: r.firstHits(sc, rays, k=4)), ("first_hits_k8", lambda: r.firstHits(sc, rays, k=8)),
                        ("raw_k4", lambda: raw(bufs[4][0], bufs[4][1], 4 * n, counts)), ("raw_k8", lambda: raw(bufs[8][0], bufs[8][1], 8 * n, counts)),
                        ("fill", lambda: raw(splits, csr, total, None)), ("count_only", lambda: raw(splits, None, 0, counts))):
            if key == "fill" and total == 0:
                continue
            ms, t_lo, t_hi = timed(fn, args.reps, args.warmup, args.calls)
            row[key] = {"ms": round(ms, 4), "ms_min": round(t_lo, 4), "ms_max": round(t_hi, 4), "mrays_per_s": round(n / ms / 1000.0, 1)}
        m = min(args.count, n)
        ref, ref_totals = hr.list_hits(osc, org[:m], dirs[:m], 0.0, np.inf, 4)
        got = r.firstHits(sc, org[:m], dirs[:m], k=4)
        same = all(np.array_equal(np.ascontiguousarray(getattr(got, f)).reshape(-1).view(np.uint32), np.ascontiguousarray(getattr(ref, f)).view(np.uint32))
                   for f in ref._fields) and np.array_equal(got.count.view(np.uint32), ref_totals)
        whole = r.listHits(sc, org[:m], dirs[:m])
        ref = hr.list_hits(osc, org[:m], dirs[:m], 0.0, np.inf, ref_totals)[0]
        same = same and all(np.array_equal(np.ascontiguousarray(getattr(whole, f)).view(np.uint32), np.ascontiguousarray(getattr(ref, f)).view(np.uint32))
                            for f in ref._fields)
        row["bit_equal_to_restatement"] = bool(same)
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
