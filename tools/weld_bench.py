"""Cost of welding, vertex normals and one smoothing step (Renderer.weld / vertexNormals / smooth, kernel_weld.hip) next to two
yardsticks each: a device-to-device copy of the bytes the call reads and writes, and the host path to the same answer with its
transfers -- np.unique over the 12-byte positions for the weld, triEdgeAdjacency (the only connectivity the project could recover from
soup before) beside it, and the numpy restatement (tests/weld_ref.py) for the normals and the step.  One JSON line per mesh:
  sphere N     the isosurface of |x| - 0.8 at N^3 (tools/isosurface_bench.py's field)
  remesh S N   Renderer.remesh of a scene at N^3
ms = device events around --calls back-to-back calls, per call; the copy and the call alternate in the same process, median of --reps
after --warmup, with the fastest and the slowest.  The raw entry points are timed (no allocation, no read-back); `call_ms` is the whole
Python weld -- allocation, the launches, the read-back of V -- by the host clock around a device synchronise.  The 64-bit integer
atomic rate of the chip is not assumed anywhere: `atomics_per_ns` reports what the sums were seen to do.  The host paths run --host-reps
times (they take seconds on the large meshes; 0 skips them).

  python tools/weld_bench.py [--sizes 128,256,512] [--scene dense_monkey] [--scene-size 128] [--reps 15] [--warmup 3] [--calls 4]
                             [--host-reps 2] [--out file.jsonl]
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
from tests import weld_ref as wd  # noqa: E402
from tests.scenes import scene_path  # noqa: E402
from tools.isosurface_bench import alternate, stat  # noqa: E402


def host_ms(fn, reps):
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms": round(float(np.median(ms)), 2), "ms_min": round(min(ms), 2), "ms_max": round(max(ms), 2)} if ms else None


def measure(r, name, surf, args):
    dev = surf.tris.device
    rec = surf.records()                                         # the fill's own 48-byte records: the weld reads them in place
    n = int(rec.shape[0])
    mesh = r.weld(surf)
    v = int(mesh.vertices.shape[0])
    stream = torch.cuda.current_stream(dev).cuda_stream
    faces = torch.empty((n, 3), dtype=torch.int32, device=dev)
    first = torch.empty(v, dtype=torch.int32, device=dev)
    vertices = torch.empty((v, 3), dtype=torch.float32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    normals, moved = torch.empty_like(vertices), torch.empty_like(vertices)
    factor = (ctypes.c_float * 1)(0.5)
    L, h = drt._lib, r._h

    def weld():
        drt._check(L.drt_renderer_weld(h, rec.data_ptr(), n, 48, faces.data_ptr(), first.data_ptr(), vertices.data_ptr(), v, count.data_ptr(), stream))

    def normals_of(weight):
        return lambda: drt._check(L.drt_renderer_vertex_normals(h, mesh.vertices.data_ptr(), v, mesh.faces.data_ptr(), n, weight, normals.data_ptr(), stream))

    def step():
        drt._check(L.drt_renderer_smooth_vertices(h, mesh.vertices.data_ptr(), v, mesh.faces.data_ptr(), n, factor, 1, None, moved.data_ptr(), stream))

    # the bytes each call reads and writes once, as one copy of half that size (a copy reads and writes every byte of its buffer)
    weld_bytes = n * 36 + n * 12 + v * 16
    mesh_bytes = n * 12 + n * 36 + v * 12                        # the faces, the positions gathered through them, the result
    buf = {k: torch.empty(max(b // 8, 1), dtype=torch.float32, device=dev) for k, b in (("weld", weld_bytes), ("mesh", mesh_bytes))}
    dst = {k: torch.empty_like(b) for k, b in buf.items()}
    fns = {"copy_weld": lambda: dst["weld"].copy_(buf["weld"]), "weld": weld, "copy_mesh": lambda: dst["mesh"].copy_(buf["mesh"]),
           "normals_angle": normals_of(0), "normals_area": normals_of(1), "smooth_step": step}
    t = alternate(fns, args.reps, args.warmup, args.calls)
    weld()
    torch.cuda.synchronize()
    assert int(count.item()) == v and torch.equal(faces, mesh.faces) and torch.equal(first, mesh.first)
    assert torch.equal(vertices.view(torch.int32), mesh.vertices.view(torch.int32))
    call = []
    for i in range(args.reps + args.warmup):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.weld(surf)
        torch.cuda.synchronize()
        if i >= args.warmup:
            call.append((time.perf_counter() - t0) * 1e3)
    row = {"mesh": name, "triangles": n, "vertices": v, "weld_bytes": weld_bytes, "mesh_bytes": mesh_bytes,
           "weld": stat(t["weld"], weld_bytes), "copy_weld": stat(t["copy_weld"], weld_bytes),
           "weld_over_copy": round(t["weld"][0] / t["copy_weld"][0], 2), "mcorners_per_s": round(3 * n / t["weld"][0] / 1000.0, 1),
           "copy_mesh": stat(t["copy_mesh"], mesh_bytes)}
    for key, atomics in (("normals_angle", 9 * n), ("normals_area", 9 * n), ("smooth_step", 12 * n)):
        row[key] = stat(t[key], mesh_bytes)
        row[key]["over_copy"] = round(t[key][0] / t["copy_mesh"][0], 2)
        row[key]["atomics_per_ns"] = round(atomics / t[key][0] / 1e6, 2)      # an upper bound on the time the atomics took: the whole call
    row.update({"call_ms": round(float(np.median(call)), 4), "call_ms_min": round(min(call), 4), "call_ms_max": round(max(call), 4)})
    if args.host_reps:
        tris = surf.tris

        def host_weld():
            return wd.weld(tris.cpu().numpy())

        hv, hf, hfirst, hn = host_weld()
        row["host_unique"] = host_ms(host_weld, args.host_reps)
        row["host_equal"] = bool(hn == v and hf.tolist() == mesh.faces.cpu().numpy().tolist() and hv.tobytes() == mesh.vertices.cpu().numpy().tobytes())
        row["host_edge_adjacency"] = host_ms(lambda: drt.triEdgeAdjacency(tris), args.host_reps)
        row["host_normals_angle"] = host_ms(lambda: torch.from_numpy(wd.vertex_normals(mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy())).to(dev),
                                            args.host_reps)
        row["host_smooth_step"] = host_ms(lambda: torch.from_numpy(wd.smooth_step(mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy(), 0.5)).to(dev),
                                          args.host_reps)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256,512")
    ap.add_argument("--scene", default="dense_monkey")
    ap.add_argument("--scene-size", type=int, default=128)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--host-reps", type=int, default=2)
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
        surf = r.isosurface(field, 0.0, lo, hi)
        del field
        emit(measure(r, "sphere %d" % n, surf, args))
        del surf
    if args.scene:
        sc = drt.Scene()
        sc.loadGLTFmodel(scene_path(args.scene))
        b = drt.BVHBuilder()
        b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
        b.buildIterative(sc)
        row = measure(r, "remesh %s %d" % (args.scene, args.scene_size), r.remesh(sc, args.scene_size), args)
        row["scene_triangles"] = int(len(sc.m_PrimitivesBuffer))
        emit(row)


if __name__ == "__main__":
    main()
