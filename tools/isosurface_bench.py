"""Cost of isosurface extraction (Renderer.isosurface, kernel_isosurface.hip) next to its two yardsticks: the count pass reads the field
once, so it is measured against a device-to-device copy of the field's bytes; the fill pass is bound by its 48-byte records, so it is
measured against a device-to-device copy of the output's bytes.  One JSON line per field:
  sphere N     |x| - 0.8 made in torch at N^3 over (-1.03, -1.1, -1.07)..(1.05, 1.02, 1.09), level 0
  winding N    Renderer.windingGrid of a scene at N^3, level 0.5, flip, border 0 (the remesh pipeline's last step)
ms = device events around --calls back-to-back launches, per launch; the copy and the pass alternate in the same process, median of
--reps after --warmup, with the fastest and the slowest.  `call_ms` is the whole Python call -- count, cumulative sum, the read-back of
the total, fill -- by the host clock around a device synchronise.  Also: triangles per second of the two passes together, the share
of rows with a triangle, and whether the first --count records equal the restatement (tests/isosurface_ref.py).

  python tools/isosurface_bench.py [--sizes 128,256,512] [--scene dense_monkey] [--scene-size 128] [--reps 15] [--warmup 3] [--calls 8]
                                   [--count 300] [--out file.jsonl]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import dustraytracer_amd as drt  # noqa: E402
from tests import isosurface_ref as iso  # noqa: E402
from tests.scenes import scene_path  # noqa: E402

NAN = float("nan")


def event_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def alternate(fns, reps, warmup, calls):
    """{name: (median, fastest, slowest) ms} of functions measured in turn, round after round."""
    ms = {k: [] for k in fns}
    for i in range(reps + warmup):
        for k, fn in fns.items():
            t = event_ms(fn, calls)
            if i >= warmup:
                ms[k].append(t)
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ms.items()}


def stat(t, nbytes=None):
    d = {"ms": round(t[0], 4), "ms_min": round(t[1], 4), "ms_max": round(t[2], 4)}
    if nbytes is not None:
        d["gb_per_s"] = round(nbytes / t[0] / 1e6, 1)
    return d


def measure(r, name, field, level, lo, hi, flip, border, args):
    dev = field.device
    res = (field.shape[2], field.shape[1], field.shape[0])
    cell = iso.cell_of(lo, hi, res)
    grid = drt._Grid()
    grid.lo[:], grid.cell[:], grid.dims[:] = [float(v) for v in np.float32(lo)], [float(v) for v in cell], res
    b = NAN if border is None else float(border)
    surf = r.isosurface(field, level, lo, hi, flip=flip, border=border)
    total, rows = int(surf.tris.shape[0]), int(surf.splits.shape[0]) - 1
    counts = torch.empty(rows, dtype=torch.int32, device=dev)
    out = torch.empty((max(total, 1), 12), dtype=torch.float32, device=dev)
    field_copy, out_copy = torch.empty_like(field), torch.empty_like(out)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def count_pass():
        drt._check(drt._lib.drt_renderer_isosurface(r._h, field.data_ptr(), ctypes.byref(grid), level, b, int(flip), None, None, 0, counts.data_ptr(), stream))

    def fill_pass():
        drt._check(drt._lib.drt_renderer_isosurface(r._h, field.data_ptr(), ctypes.byref(grid), level, b, int(flip), surf.splits.data_ptr(),
                                                    out.data_ptr(), total, None, stream))

    fns = {"copy_field": lambda: field_copy.copy_(field), "count": count_pass, "copy_out": lambda: out_copy.copy_(out)}
    if total:
        fns["fill"] = fill_pass
    t = alternate(fns, args.reps, args.warmup, args.calls)
    call = []
    for i in range(args.reps + args.warmup):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.isosurface(field, level, lo, hi, flip=flip, border=border)
        torch.cuda.synchronize()
        if i >= args.warmup:
            call.append((time.perf_counter() - t0) * 1e3)
    row = {"field": name, "samples": list(res), "level": level, "flip": bool(flip), "border": border, "triangles": total, "rows": rows,
           "nonempty_rows": round(float(((surf.splits[1:] - surf.splits[:-1]) > 0).float().mean().item()), 4),
           "field_bytes": field.numel() * 4, "out_bytes": total * 48,
           "count": stat(t["count"], field.numel() * 4), "copy_field": stat(t["copy_field"], 2 * field.numel() * 4),
           "copy_out": stat(t["copy_out"], 2 * max(total, 1) * 48),
           "count_over_copy": round(t["count"][0] / t["copy_field"][0], 3),
           "call_ms": round(float(np.median(call)), 4), "call_ms_min": round(min(call), 4), "call_ms_max": round(max(call), 4)}
    if total:
        row["fill"] = stat(t["fill"], total * 48)
        row["fill_over_copy"] = round(t["fill"][0] / t["copy_out"][0], 3)
        row["mtriangles_per_s"] = round(total / (t["count"][0] + t["fill"][0]) / 1000.0, 1)
        assert torch.equal(out.view(torch.int32), surf.records().view(torch.int32))
    # the first records against the restatement: the leading z slabs of the field hold them
    k = min(args.count, total)
    if k:
        nx, ny = (res[0] + 1, res[1] + 1) if border is not None else (res[0] - 1, res[1] - 1)
        last_cz = int(surf.cube[k - 1].item()) // (nx * ny)
        slabs = min(res[2], last_cz + 2)                       # samples z < slabs decide the cubes up to cz = last_cz
        _, ref = iso.isosurface(field[:slabs].cpu().numpy(), level, lo, cell, flip=flip, border=border)
        row["first_records_equal_restatement"] = bool(len(ref) >= k and surf.records()[:k].cpu().numpy().tobytes() == ref[:k].tobytes())
        row["records_compared"] = k
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256,512")
    ap.add_argument("--scene", default="dense_monkey")
    ap.add_argument("--scene-size", type=int, default=128)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--count", type=int, default=300)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = open(args.out, "a") if args.out else None
    r = drt.Renderer(0)

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    lo, hi = np.float32([-1.03, -1.1, -1.07]), np.float32([1.05, 1.02, 1.09])
    for n in [int(v) for v in args.sizes.split(",") if v]:
        cell = iso.cell_of(lo, hi, (n,) * 3)
        ax = [float(lo[k]) + (torch.arange(n, dtype=torch.float32, device=dev) + 0.5) * float(cell[k]) for k in range(3)]
        z, y, x = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        field = torch.sqrt(x * x + y * y + z * z) - 0.8
        del x, y, z
        emit(measure(r, "sphere %d" % n, field, 0.0, lo, hi, False, None, args))
        del field
    if args.scene:
        sc = drt.Scene()
        sc.loadGLTFmodel(scene_path(args.scene))
        b = drt.BVHBuilder()
        b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
        b.buildIterative(sc)
        root = sc.m_BVHNodes[-1]
        n = args.scene_size
        cell = iso.cell_of(root["bmin"], root["bmax"], (n,) * 3)
        slo, shi = (root["bmin"] - cell).astype(np.float32), (root["bmax"] + cell).astype(np.float32)      # Renderer.remesh's margin of one cell
        field = r.windingGrid(sc, n + 2, slo, shi)
        row = measure(r, "winding %s %d" % (args.scene, n + 2), field, 0.5, slo, shi, True, 0.0, args)
        row["scene_triangles"] = int(len(sc.m_PrimitivesBuffer))
        emit(row)


if __name__ == "__main__":
    main()
