"""What the intersection segments cost next to the pair list a caller has today: count + fill of Renderer.intersectTriangles
(kernel_intersect.hip) against count + fill of Renderer.overlapTriangles (kernel_tri_overlap.hip) on the same queries, from the same
process, the two interleaved rep by rep.  The mesh is the soup of tools/bvh_build_bench.py (n triangles of 0.1 across, centres uniform
in [-10, 10]^3, seed 1; 10^6 by default), built on the GPU with the editor's tree (leaf 20, bins 8), and the queries are that mesh itself
in tree order displaced by --shift of its extent along (1, 1, 1) / sqrt(3): a moved copy of a part against the part.  One JSON line:
  segments / pairs   the whole call: the count pass, the scan, the read-back of the total, the fill -- ms by a host clock around the
                     call and a device synchronise, median of --reps after --warmup, min and max beside it
  *_count, *_fill    the two passes alone on buffers made beforehand, device events around each
  ratio              segments ms / pairs ms, whole calls
  records, listed    what the two return in all; pairs_without_segment, segments_without_pair: the difference of the two sets
The first --check queries are compared with the restatement (tests/intersect_ref.py).

  python tools/intersect_bench.py [--triangles 1000000] [--shift 0.01] [--reps 25] [--warmup 3] [--check 200] [--out file.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import dustraytracer_amd as drt  # noqa: E402
from tests import intersect_ref as ix  # noqa: E402
from tests import nearest_ref as nr  # noqa: E402


def soup(n, seed=1):
    """tools/bvh_build_bench.py's soup, built on the GPU."""
    rng = np.random.default_rng(seed)
    pos = (rng.uniform(-10, 10, (n, 1, 3)) + rng.uniform(-0.05, 0.05, (n, 3, 3))).astype(np.float32)
    sc = drt.Scene()
    sc.addMaterial((0.8, 0.8, 0.8), -1)
    sc.setGeometry(pos, np.tile(np.array([0, 1, 0], np.float32), (n, 3, 1)), np.zeros((n, 3, 2), np.float32), np.zeros(n, np.int32))
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount, b.m_BuildDevice = 20, 8, 0
    b.buildIterative(sc)
    return sc


def stats(times):
    return {"ms": round(float(np.median(times)), 4), "ms_min": round(float(np.min(times)), 4), "ms_max": round(float(np.max(times)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=1000000)
    ap.add_argument("--shift", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", type=int, default=200)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps: the median of at least 20 is what is reported")
    dev = torch.device("cuda", 0)
    sc = soup(args.triangles)
    own = np.ascontiguousarray(sc.m_PrimitivesBuffer["vertex"]["position"], np.float32).reshape(-1, 3, 3)
    extent = float((own.reshape(-1, 3).max(axis=0) - own.reshape(-1, 3).min(axis=0)).max())
    host_q = (own + np.float32(args.shift * extent / np.sqrt(3.0))).astype(np.float32)
    n = len(host_q)
    r = drt.Renderer(0)
    tris = torch.zeros((n, 12), dtype=torch.float32, device=dev)
    tris[:, :9] = torch.from_numpy(host_q).to(dev).reshape(n, 9)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def whole(fn):
        t0 = time.perf_counter()
        res = fn(sc, tris)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, res

    calls = {"segments": r.intersectTriangles, "pairs": r.overlapTriangles}
    times = {k: [] for k in calls}
    first = {}
    for rep in range(args.warmup + args.reps):                                   # interleaved; the warm-up is discarded
        for key, fn in calls.items():
            ms, res = whole(fn)
            if rep >= args.warmup:
                times[key].append(ms)
            first.setdefault(key, res)
    seg, pairs = first["segments"], first["pairs"]

    # the two passes alone, on buffers made beforehand
    no_room = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    rec = torch.empty((max(len(seg.prim), 1), 8), dtype=torch.float32, device=dev)
    prim = torch.empty(max(len(pairs.prim), 1), dtype=torch.int32, device=dev)
    L = drt._lib
    passes = {
        "segments_count": lambda: L.drt_renderer_intersect_triangles(r._h, sc._h, tris.data_ptr(), no_room.data_ptr(), None, 0, counts.data_ptr(), n, stream),
        "pairs_count": lambda: L.drt_renderer_overlap_triangles(r._h, sc._h, tris.data_ptr(), no_room.data_ptr(), None, 0, counts.data_ptr(), n, drt.OVERLAP_LIST, stream),
        "segments_fill": lambda: L.drt_renderer_intersect_triangles(r._h, sc._h, tris.data_ptr(), seg.splits.data_ptr(), rec.data_ptr(), len(rec), None, n, stream),
        "pairs_fill": lambda: L.drt_renderer_overlap_triangles(r._h, sc._h, tris.data_ptr(), pairs.splits.data_ptr(), prim.data_ptr(), len(prim), None, n, drt.OVERLAP_LIST, stream)}
    pass_times = {k: [] for k in passes}
    for rep in range(args.warmup + args.reps):
        for key, fn in passes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            assert fn() == drt.OK, L.drt_last_error()
            b.record()
            b.synchronize()
            if rep >= args.warmup:
                pass_times[key].append(a.elapsed_time(b))

    def keys(res):
        owner = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), (res.splits[1:] - res.splits[:-1]).to(torch.int64))
        return owner * (1 << 32) + res.prim.to(torch.int64)

    ks, kp = keys(seg), keys(pairs)
    row = {"mesh": "soup", "triangles": n, "bvh_depth": sc.bvh_depth, "queries": n, "shift_over_extent": args.shift, "reps": args.reps,
           "warmup": args.warmup, "records": int(len(seg.prim)), "listed": int(len(pairs.prim)),
           "pairs_without_segment": int((~torch.isin(kp, ks)).sum().item()), "segments_without_pair": int((~torch.isin(ks, kp)).sum().item())}
    for key in calls:
        row[key] = stats(times[key])
    for key in passes:
        row[key] = stats(pass_times[key])
    row["ratio"] = round(row["segments"]["ms"] / row["pairs"]["ms"], 3)
    m = min(args.check, n)
    g = nr.from_product(sc)
    splits, ref = ix.whole(g, host_q[:m])
    got = r.intersectTriangles(sc, host_q[:m])
    words = np.zeros((len(got.prim), 8), np.int32)
    words[:, 0:3], words[:, 4:7], words[:, 3], words[:, 7] = got.p.view(np.int32), got.q.view(np.int32), got.prim, got.code
    row["bit_equal_to_restatement"] = bool(np.array_equal(got.splits, splits) and words.tobytes() == ref.tobytes())
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
