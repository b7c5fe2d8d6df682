"""Cost of mesh simplification (Renderer.simplify, kernel_simplify.hip) next to two yardsticks: a device-to-device copy of the bytes the
call reads and writes, and the host path to the same answer -- the numpy restatement (tests/simplify_ref.py) with its transfers.  The
meshes are tools/weld_bench.py's, welded:
  sphere N     the isosurface of |x| - 0.8 at N^3; the grids are N/2, N/4 and N/8 cells across the field's box
  remesh S N   Renderer.remesh of a scene at N^3; the grids are N/2, N/4 and N/8 cells across the mesh's own box (the default box)
One JSON line per mesh, grid and placement.  ms = device events around --calls back-to-back calls, per call; the copy and the call
alternate in the same process, median of --reps after --warmup, with the fastest and the slowest.  The raw entry point is timed (no
allocation, no read-back); `call_ms` is the whole Python call by the host clock around a device synchronise.  DRT_SIMPLIFY_SUMS=plain
in the environment makes the library add one atomic per term instead of one per run of lanes; `sums` records which form ran.  The 64-bit integer atomic rate of the
chip is not assumed anywhere: `atomics_per_ns` reports what the whole call was seen to do.  The host path runs once per mesh, at the first
divisor and the last placement (--host 0 skips it).

  python tools/simplify_bench.py [--sizes 128,256,512] [--scene dense_monkey] [--scene-size 128] [--divisors 2,4,8] [--reps 15]
                                 [--warmup 3] [--calls 4] [--host 1] [--out file.jsonl]
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
from tests import simplify_ref as sr  # noqa: E402
from tests.scenes import scene_path  # noqa: E402
from tools.isosurface_bench import alternate, stat  # noqa: E402


def measure(r, name, mesh, grid, res, placement, args, host):
    dev = mesh.vertices.device
    nv, nt = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    stream = torch.cuda.current_stream(dev).cuda_stream
    cluster = torch.empty(nv, dtype=torch.int32, device=dev)
    out_v = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    first = torch.empty(nv, dtype=torch.int32, device=dev)
    out_f = torch.empty((nt, 3), dtype=torch.int32, device=dev)
    source = torch.empty(nt, dtype=torch.int32, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    code = drt.SIMPLIFY_PLACEMENTS[placement]

    def call():
        drt._check(drt._lib.drt_renderer_simplify(r._h, mesh.vertices.data_ptr(), nv, mesh.faces.data_ptr(), nt, ctypes.byref(grid), code,
                                                  cluster.data_ptr(), out_v.data_ptr(), first.data_ptr(), nv, out_f.data_ptr(), source.data_ptr(),
                                                  nt, counts.data_ptr(), stream))

    call()
    c, m = (int(x) for x in counts.tolist())
    # the bytes the call reads and writes once: the positions, the faces (quadric: and the positions gathered through them), the ids,
    # the stored clusters and triangles -- as one copy of half that size (a copy reads and writes every byte of its buffer)
    nbytes = nv * 12 + nt * 12 + (nt * 36 if code else 0) + nv * 4 + c * 16 + m * 16
    buf = torch.empty(max(nbytes // 8, 1), dtype=torch.float32, device=dev)
    dst = torch.empty_like(buf)
    t = alternate({"copy": lambda: dst.copy_(buf), "simplify": call}, args.reps, args.warmup, args.calls)
    lo, cell, dims = np.float32(list(grid.lo)), np.float32(list(grid.cell)), [int(d) for d in grid.dims]
    whole = []
    kw = dict(resolution=tuple(dims), lo=lo, hi=(lo.astype(np.float64) + cell.astype(np.float64) * dims).astype(np.float32), placement=placement)
    for i in range(5 + args.warmup):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.simplify(mesh, **kw)
        torch.cuda.synchronize()
        if i >= args.warmup:
            whole.append((time.perf_counter() - t0) * 1e3)
    atomics = nv * 4 + (27 * nt if code else 0)                               # an upper bound: every vertex in the grid, every corner adding
    row = {"mesh": name, "triangles": nt, "vertices": nv, "grid": dims, "divisor": res, "placement": placement,
           "sums": os.environ.get("DRT_SIMPLIFY_SUMS", "runs"), "clusters": c, "triangles_out": m, "bytes": nbytes,
           "simplify": stat(t["simplify"], nbytes), "copy": stat(t["copy"], nbytes), "over_copy": round(t["simplify"][0] / t["copy"][0], 2),
           "atomics_per_ns": round(atomics / t["simplify"][0] / 1e6, 2), "call_ms": round(float(np.median(whole)), 4)}
    if host:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want = sr.simplify(mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy(), lo, cell, dims, code)
        moved = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in want[:5]]
        torch.cuda.synchronize()
        row["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        row["host_equal"] = bool(want.counts == (c, m) and torch.equal(moved[3], cluster) and torch.equal(moved[1], out_f[:m]) and
                                 torch.equal(moved[4], source[:m]) and torch.equal(moved[2], first[:c]) and
                                 torch.equal(moved[0].view(torch.int32), out_v[:c].view(torch.int32)))
    return row


def grid_of(lo, hi, res):
    g = drt._Grid()
    cell = ((np.float32(hi) - np.float32(lo)) / np.float32(res)).astype(np.float32)
    g.lo[:], g.cell[:], g.dims[:] = [float(x) for x in np.float32(lo)], [float(x) for x in cell], [int(res)] * 3
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256,512")
    ap.add_argument("--scene", default="dense_monkey")
    ap.add_argument("--scene-size", type=int, default=128)
    ap.add_argument("--divisors", default="2,4,8")
    ap.add_argument("--placements", default="mean,quadric")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--host", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = open(args.out, "a") if args.out else None
    r = drt.Renderer(0)
    divisors = [int(v) for v in args.divisors.split(",") if v]
    placements = [p for p in args.placements.split(",") if p]

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
        mesh = r.weld(r.isosurface(field, 0.0, lo, hi))
        del field
        for d in divisors:
            for p in placements:
                emit(measure(r, "sphere %d" % n, mesh, grid_of(lo, hi, n // d), d, p, args, args.host and d == divisors[0] and p == placements[-1]))
        del mesh
    if args.scene:
        sc = drt.Scene()
        sc.loadGLTFmodel(scene_path(args.scene))
        b = drt.BVHBuilder()
        b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
        b.buildIterative(sc)
        mesh = r.weld(r.remesh(sc, args.scene_size))
        box = torch.stack([mesh.vertices.amin(dim=0), mesh.vertices.amax(dim=0)]).cpu().numpy()
        for d in divisors:
            for p in placements:
                emit(measure(r, "remesh %s %d" % (args.scene, args.scene_size), mesh,
                             drt.Renderer._simplify_grid(box, args.scene_size // d, None, None, None), d, p, args,
                             args.host and d == divisors[0] and p == placements[-1]))


if __name__ == "__main__":
    main()
