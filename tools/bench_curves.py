"""Times of the intersection-curve call (drt_renderer_chain_intersections, kernel_curve.hip and the phases it shares with
kernel_contour.hip) beside the fill of drt_renderer_intersect_triangles that wrote the records it chains, as tools/bench_contours.py
times the section contours beside the section fill.  The scene is a closed UV sphere of radius 1 (--segments round the axis, half as
many from pole to pole; 1 400 gives 2 * 10^6 triangles), built on the GPU with the editor's tree (leaf 20, bins 8); the queries are
--meshes small closed UV spheres (--small segments round the axis, radius --radius) with random rotations, centred at random points
of the large one: every one of them cuts it in a loop.  One JSON line:
  fill     the intersection fill of the queries' records into segments made beforehand
  chain    the chain call on those records, with counts
  table    triEdgeAdjacency of the query meshes on the host, by a host clock (made once per tool, not per frame)
ms = device events around one call, median / min / max of --reps after --warmup; chain_over_fill = chain ms / fill ms; rounds = the
jumping rounds launched, ceil(log2(records)); rounds_busy = those that can still rank a record or move a minimum, 1 +
ceil(log2(longest chain)), from the longest chain found (every later round returns at its first instruction); hw_queues = the
GPU_MAX_HW_QUEUES the process ran under.  The first --check query meshes are compared with the restatement (tests/curve_ref.py): closed
meshes link only among themselves, so their chains stand in front of the list.

  python tools/bench_curves.py [--segments 1400] [--meshes 8192] [--small 8] [--radius 0.05] [--reps 25] [--warmup 3] [--check 16] [--out file.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=1400)
    ap.add_argument("--meshes", type=int, default=8192)
    ap.add_argument("--small", type=int, default=8)
    ap.add_argument("--radius", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", type=int, default=16)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    import dustraytracer_amd as drt
    from tests import curve_ref as cu
    from tests import curve_scenes as cv
    from tools.nearest_bench import timed

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(12)
    pos = cv.placed(*cv.uv_sphere(args.segments, args.segments // 2), cv.rotation(rng))
    n_tris = len(pos)
    sc = drt.Scene()
    sc.addMaterial((0.8, 0.8, 0.8), -1)
    sc.setGeometry(pos, np.tile(np.array([0, 1, 0], np.float32), (n_tris, 3, 1)), np.zeros((n_tris, 3, 2), np.float32), np.zeros(n_tris, np.int32))
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount, b.m_BuildDevice = 20, 8, 0
    b.buildIterative(sc)
    small_v, small_t = cv.uv_sphere(args.small, max(args.small // 2, 2), args.radius)
    centres = rng.normal(size=(args.meshes, 3))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    host_q = np.concatenate([cv.placed(small_v, small_t, cv.rotation(rng), c) for c in centres])
    per_mesh = len(small_t)
    n = len(host_q)
    t0 = time.perf_counter()
    table = drt.triEdgeAdjacency(host_q)
    table_ms = (time.perf_counter() - t0) * 1e3
    assert (table >= 0).all()                                                  # closed query meshes

    r = drt.Renderer(0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    tris = torch.zeros((n, 12), dtype=torch.float32, device=dev)
    tris[:, :9] = torch.from_numpy(host_q).to(dev).reshape(n, 9)
    cuts = r.intersectTriangles(sc, tris)
    total = int(cuts.prim.shape[0])
    assert total > 0
    rec = torch.empty((total, 8), dtype=torch.float32, device=dev)
    slots = torch.empty((total, 4), dtype=torch.int32, device=dev)
    counts = torch.empty(3, dtype=torch.int32, device=dev)
    query_adj = torch.from_numpy(table).to(dev)
    L = drt._lib

    def fill():
        rc = L.drt_renderer_intersect_triangles(r._h, sc._h, tris.data_ptr(), cuts.splits.data_ptr(), rec.data_ptr(), total, None, n, stream)
        assert rc == drt.OK, L.drt_last_error()

    def chain():
        rc = L.drt_renderer_chain_intersections(r._h, sc._h, rec.data_ptr(), cuts.splits.data_ptr(), query_adj.data_ptr(), slots.data_ptr(), counts.data_ptr(),
                                                n, total, stream)
        assert rc == drt.OK, L.drt_last_error()

    row = {"mesh": "uv_sphere", "triangles": n_tris, "bvh_depth": sc.bvh_depth, "query_meshes": args.meshes, "triangles_per_query_mesh": per_mesh,
           "queries": n, "radius": args.radius, "records": total, "reps": args.reps, "warmup": args.warmup,
           "rounds": int(np.ceil(np.log2(max(total, 1)))), "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "default")}
    fill()
    chain()
    times = {"fill": [], "chain": []}
    for rep in range(args.warmup + args.reps):                                 # interleaved; the warm-up is discarded
        for key, fn in (("fill", fill), ("chain", chain)):
            ms, _, _ = timed(fn, 1, 0, 1)
            if rep >= args.warmup:
                times[key].append(ms)
    for key, t in times.items():
        row[key] = {"ms": round(float(np.median(t)), 4), "ms_min": round(float(np.min(t)), 4), "ms_max": round(float(np.max(t)), 4)}
    row["chain_over_fill"] = round(row["chain"]["ms"] / row["fill"]["ms"], 2)
    row["table"] = {"host_ms": round(table_ms, 2)}
    torch.cuda.synchronize()
    starts = slots[:, 1] == torch.arange(total, dtype=torch.int32, device=dev)
    got_counts = counts.cpu().numpy()
    row["chains"], row["closed"], row["not_live"] = (int(x) for x in got_counts)
    row["longest_chain"] = int(slots[:, 2][starts].max().item())
    row["rounds_busy"] = min(row["rounds"], 1 + int(np.ceil(np.log2(max(row["longest_chain"], 1)))))
    row["statuses"] = torch.bincount((slots[:, 3] >> 1).to(torch.int64), minlength=6).cpu().tolist()
    m = min(args.check, args.meshes)
    if m:
        k = m * per_mesh
        splits = cuts.splits[:k + 1].cpu().numpy().astype(np.int64)
        part = int(splits[-1])
        want, want_counts = cu.chain(sc.edgeAdjacency().reshape(-1), table.reshape(-1)[:3 * k], cuts.prim[:part].cpu().numpy(), cuts.code[:part].cpu().numpy(),
                                     splits, n_tris)
        got = slots[:part].cpu().numpy().view(cu.SLOT).reshape(-1)
        row["checked_records"] = part
        row["bit_equal_to_restatement"] = bool(got.tobytes() == want.tobytes())
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if row.get("bit_equal_to_restatement", True) else 1


if __name__ == "__main__":
    sys.exit(main())
