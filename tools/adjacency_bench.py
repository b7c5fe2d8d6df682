"""Cost of the device edge adjacency (Renderer.edgeAdjacency / boundaryVertices, kernel_adjacency.hip) next to two yardsticks: the
host routine it replaces (triEdgeAdjacency: a sort over 3 N half-edges) on the same arrays, and a device-to-device copy of the bytes the
call reads and writes.  One JSON line per mesh or scene:
  sphere N       the isosurface of |x| - 0.8 at N^3 (tools/weld_bench.py's meshes), by position on the fill's own 48-byte records and by
                 index on the weld's faces, each with and without the edge numbering, and the boundary vertices
  scene S        the first Renderer.shells call after an upload of scene S -- the call that waits for the scene's table -- on a
                 renderer made with DRT_ADJACENCY=host (the parent's route: the host's sort and an upload) and on a default one (the
                 kernel), with the parts of the device route timed on their own; `strip:N` is the strip of tests/topology_scenes.py at
                 N triangles
ms of the mesh rows = device events around --calls back-to-back calls, per call; the copy and the calls alternate in the same process,
median of --reps after --warmup, with the fastest and the slowest.  The raw entry points are timed (no allocation, no read-back).  The
scene rows are host wall clock around the call and a device synchronise, because the host's sort is host time; the scene is uploaded
afresh, without a table, in front of every repeat and outside the timed span.  The host routine runs --host-reps times (it takes a
second on the largest mesh; 0 skips it), and its table is compared with the device's.

  python tools/adjacency_bench.py [--sizes 128,256,512] [--scenes cs16_dust,dense_monkey,strip:1048576] [--reps 15] [--warmup 3]
                                  [--calls 4] [--host-reps 2] [--out file.jsonl]
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
from tests import contour_scenes as cs  # noqa: E402
from tests import isosurface_ref as iso  # noqa: E402
from tests import topology_scenes as ts  # noqa: E402
from tools.isosurface_bench import alternate, stat  # noqa: E402
from tools.overlap_bench import load  # noqa: E402
from tools.weld_bench import host_ms  # noqa: E402


def measure_mesh(r, name, surf, args):
    dev = surf.tris.device
    rec = surf.records()                                         # the fill's own 48-byte records, read in place
    n = int(rec.shape[0])
    mesh = r.weld(surf)
    v = int(mesh.vertices.shape[0])
    stream = torch.cuda.current_stream(dev).cuda_stream
    adj, edge = (torch.empty((n, 3), dtype=torch.int32, device=dev) for _ in range(2))
    half_edge = torch.empty(3 * n, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    flags = torch.empty(v, dtype=torch.uint8, device=dev)
    L, h = drt._lib, r._h

    def tri(edges):
        tail = (edge.data_ptr(), half_edge.data_ptr(), 3 * n, count.data_ptr()) if edges else (None, None, 0, None)
        return lambda: drt._check(L.drt_renderer_tri_adjacency(h, rec.data_ptr(), n, 48, adj.data_ptr(), *tail, stream))

    def face(edges):
        tail = (edge.data_ptr(), half_edge.data_ptr(), 3 * n, count.data_ptr()) if edges else (None, None, 0, None)
        return lambda: drt._check(L.drt_renderer_face_adjacency(h, mesh.faces.data_ptr(), n, adj.data_ptr(), *tail, stream))

    def boundary():
        drt._check(L.drt_renderer_boundary_vertices(h, mesh.faces.data_ptr(), adj.data_ptr(), n, v, 0, flags.data_ptr(), stream))

    # the bytes each call reads and writes once, as one copy of half that size (a copy reads and writes every byte of its buffer)
    tri_bytes, face_bytes = n * 36 + n * 12, n * 12 + n * 12
    buf = {k: torch.empty(max(b // 8, 1), dtype=torch.float32, device=dev) for k, b in (("tri", tri_bytes), ("face", face_bytes))}
    dst = {k: torch.empty_like(b) for k, b in buf.items()}
    fns = {"copy_tri": lambda: dst["tri"].copy_(buf["tri"]), "tri": tri(False), "tri_edges": tri(True),
           "copy_face": lambda: dst["face"].copy_(buf["face"]), "face": face(False), "face_edges": face(True), "boundary": boundary}
    t = alternate(fns, args.reps, args.warmup, args.calls)
    tri(True)()
    torch.cuda.synchronize()
    by_position, e = adj.clone(), int(count.item())
    face(True)()
    torch.cuda.synchronize()
    row = {"mesh": name, "triangles": n, "vertices": v, "edges": e, "euler": v - e + n, "tri_bytes": tri_bytes, "face_bytes": face_bytes,
           "by_index_equal": bool(torch.equal(adj, by_position) and int(count.item()) == e),
           "twins": int((adj >= 0).sum()), "open": int((adj == -1).sum()), "bad": int((adj == -2).sum())}
    for key, nbytes, copy in (("tri", tri_bytes, "copy_tri"), ("tri_edges", tri_bytes, "copy_tri"), ("face", face_bytes, "copy_face"),
                              ("face_edges", face_bytes, "copy_face")):
        row[key] = stat(t[key], nbytes)
        row[key]["over_copy"] = round(t[key][0] / t[copy][0], 2)
        row[key]["mhalf_edges_per_s"] = round(3 * n / t[key][0] / 1000.0, 1)
    row["copy_tri"], row["copy_face"], row["boundary"] = stat(t["copy_tri"], tri_bytes), stat(t["copy_face"], face_bytes), stat(t["boundary"])
    if args.host_reps:
        tris = surf.tris
        table = drt.triEdgeAdjacency(tris)                       # a device tensor in: copied to the host, sorted there, copied back
        row["host_equal"] = bool(torch.equal(table, by_position))
        row["host_edge_adjacency"] = host_ms(lambda: drt.triEdgeAdjacency(tris), args.host_reps)
        row["host_over_tri"] = round(row["host_edge_adjacency"]["ms"] / t["tri"][0], 1)
    return row


def wall(fn, before, reps, warmup):
    """median / fastest / slowest host ms of fn() and a device synchronise; before() runs in front of every repeat, untimed"""
    ms = []
    for k in range(warmup + reps):
        before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def make_scene(name):
    if name.startswith("strip:"):
        pos = ts.strip(int(name[6:]) // 2)
        sc = drt.Scene()
        sc.addMaterial(*cs.ONE_MATERIAL[0])
        sc.setGeometry(pos, np.tile(np.float32([0, 0, 1]), (len(pos), 3, 1)), np.zeros((len(pos), 3, 2), np.float32), np.zeros(len(pos), np.int32))
        b = drt.BVHBuilder()
        b.m_TargetLeafPrimitivesCount, b.m_BinCount = 4, 8
        b.buildIterative(sc)
        return sc
    return ts.scene(drt, name) if name in ts.ALL_NAMES else load(name)


def measure_scene(renderers, name, args):
    dev = torch.device("cuda", 0)
    L = drt._lib
    sc = make_scene(name)
    other = cs.flat_scene(drt, cs.SINGLE)[0]                      # uploading it drops everything a renderer holds of `sc`
    n = int(L.drt_scene_triangle_count(sc._h))
    stream = torch.cuda.current_stream(dev).cuda_stream
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.zeros(3, dtype=torch.int32, device=dev)
    terms = torch.empty((n, 4), dtype=torch.float64, device=dev)
    tables = {}
    row = {"scene": name, "triangles": n}
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = sc.edgeAdjacency()
        walls.append((time.perf_counter() - t0) * 1e3)
    row["adjacency_host"] = {"ms": round(float(np.median(walls)), 3), "ms_min": round(min(walls), 3), "ms_max": round(max(walls), 3)}
    for route, r in renderers.items():
        def forget(r=r):
            """the scene uploaded afresh, with no table: another scene, then a call on `sc` that needs none"""
            drt._check(L.drt_renderer_shell_terms(r._h, other._h, terms.data_ptr(), stream))
            drt._check(L.drt_renderer_shell_terms(r._h, sc._h, terms.data_ptr(), stream))

        def shells(r=r):
            drt._check(L.drt_renderer_shell_labels(r._h, sc._h, labels.data_ptr(), counts.data_ptr(), stream))

        row["shells_first_" + route] = wall(shells, forget, args.reps, args.warmup)
        row["shells_cached_" + route] = wall(shells, lambda: None, args.reps, args.warmup)
        row["route_" + route] = r.adjacencyRoute()
        adj = torch.empty((n, 3), dtype=torch.int32, device=dev)
        drt._check(L.drt_renderer_edge_adjacency(r._h, sc._h, adj.data_ptr(), stream))
        tables[route] = adj.cpu().numpy()
    row["tables_equal"] = bool(all(t.tobytes() == want.tobytes() for t in tables.values()))
    row["host_over_device"] = round(row["shells_first_host"]["ms"] / row["shells_first_device"]["ms"], 2)
    # the device route's parts on their own: the kernel on positions already on the device, and the labelling that both routes share
    tree = torch.from_numpy(ts.tree_positions(sc)).to(dev)
    adj = torch.empty((n, 3), dtype=torch.int32, device=dev)
    r = renderers["device"]
    t = alternate({"kernel": lambda: drt._check(L.drt_renderer_tri_adjacency(r._h, tree.data_ptr(), n, 36, adj.data_ptr(), None, None, 0, None, stream))},
                  args.reps, args.warmup, args.calls)
    row["kernel"] = stat(t["kernel"])
    torch.cuda.synchronize()
    row["kernel_equal"] = bool(adj.cpu().numpy().tobytes() == want.tobytes())
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256,512")
    ap.add_argument("--scenes", default="cs16_dust,dense_monkey,strip:1048576")
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
        emit(measure_mesh(r, "sphere %d" % n, surf, args))
        del surf
    scenes = [s for s in args.scenes.split(",") if s]
    if scenes:
        before = os.environ.get("DRT_ADJACENCY")
        os.environ["DRT_ADJACENCY"] = "host"                      # read when the renderer is created
        try:
            host_route = drt.Renderer(0)
        finally:
            if before is None:
                del os.environ["DRT_ADJACENCY"]
            else:
                os.environ["DRT_ADJACENCY"] = before
        for name in scenes:
            emit(measure_scene({"host": host_route, "device": r}, name, args))


if __name__ == "__main__":
    main()
