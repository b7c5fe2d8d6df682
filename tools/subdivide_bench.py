"""Cost of one level of mesh subdivision (Renderer.subdivide, kernel_subdivide.hip) next to two yardsticks, neither of which is the code
under test: drt_renderer_face_adjacency with the edge numbering alone on the same faces -- the call's own first stage -- and the host
path to the same answer, the numpy restatement (tests/subdivide_ref.py) with its transfers.  What subdivision adds on top of the
adjacency is compared with a device-to-device copy of the bytes it writes, 12 (V + E) + 48 N.  The meshes are tools/weld_bench.py's,
welded:
  sphere N     the isosurface of |x| - 0.8 at N^3 (32, 128, 256: about 2^14, 2^18 and 2^20 triangles)
  remesh S N   Renderer.remesh of a scene at N^3 (tools/simplify_bench.py's mesh)
  fan N        a closed fan of N triangles round one vertex: N atomics on one sum
One JSON line per mesh.  ms = device events around --calls back-to-back calls, per call; the copy, the adjacency and the two schemes
alternate in the same process, median of --reps after --warmup, with the fastest and the slowest.  The raw entry point is timed (no
allocation, no read-back); `call_ms` is the whole Python call of one Loop level by the host clock around a device synchronise.  The
host path runs once per mesh (--host 0 skips it), and its bytes are compared with the device's.

  python tools/subdivide_bench.py [--sizes 32,128,256] [--scene dense_monkey] [--scene-size 128] [--fan 4096] [--reps 15] [--warmup 3]
                                  [--calls 4] [--host 1] [--out file.jsonl]
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
from tests import isosurface_ref as iso  # noqa: E402
from tests import subdivide_ref as sr  # noqa: E402
from tests.scenes import scene_path  # noqa: E402
from tools.isosurface_bench import alternate, stat  # noqa: E402


def measure(r, name, vertices, faces, args):
    dev = vertices.device
    nv, nt = int(vertices.shape[0]), int(faces.shape[0])
    cap = nv + 3 * nt
    stream = torch.cuda.current_stream(dev).cuda_stream
    out_v = torch.empty((cap, 3), dtype=torch.float32, device=dev)
    parents = torch.empty((cap, 2), dtype=torch.int32, device=dev)
    out_f = torch.empty((4 * nt, 3), dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    adj, edge = (torch.empty((nt, 3), dtype=torch.int32, device=dev) for _ in range(2))
    half_edge = torch.empty(3 * nt, dtype=torch.int32, device=dev)
    edges = torch.zeros(1, dtype=torch.int32, device=dev)
    L, h = drt._lib, r._h

    def level(code):
        return lambda: drt._check(L.drt_renderer_subdivide(h, vertices.data_ptr(), nv, faces.data_ptr(), nt, code, out_v.data_ptr(),
                                                           parents.data_ptr(), cap, out_f.data_ptr(), count.data_ptr(), stream))

    def adjacency():
        drt._check(L.drt_renderer_face_adjacency(h, faces.data_ptr(), nt, adj.data_ptr(), edge.data_ptr(), half_edge.data_ptr(), 3 * nt,
                                                 edges.data_ptr(), stream))

    level(1)()
    total = int(count.item())
    ne = total - nv
    # the bytes subdivision writes on top of the adjacency, as one copy of half that size (a copy reads and writes every byte of its buffer)
    nbytes = 12 * (nv + ne) + 48 * nt
    buf = torch.empty(max(nbytes // 8, 1), dtype=torch.float32, device=dev)
    dst = torch.empty_like(buf)
    t = alternate({"copy": lambda: dst.copy_(buf), "adjacency": adjacency, "midpoint": level(0), "loop": level(1)}, args.reps, args.warmup, args.calls)
    whole = []
    for i in range(5 + args.warmup):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.subdivide((vertices, faces))
        torch.cuda.synchronize()
        if i >= args.warmup:
            whole.append((time.perf_counter() - t0) * 1e3)
    row = {"mesh": name, "triangles": nt, "vertices": nv, "edges": ne, "stream_bytes": nbytes, "copy": stat(t["copy"], nbytes),
           "adjacency": stat(t["adjacency"]), "call_ms": round(float(np.median(whole)), 4)}
    for key in ("midpoint", "loop"):
        row[key] = stat(t[key])
        row[key]["over_adjacency"] = round(t[key][0] / t["adjacency"][0], 2)
        row[key]["added_ms"] = round(t[key][0] - t["adjacency"][0], 4)
        row[key]["added_over_copy"] = round((t[key][0] - t["adjacency"][0]) / t["copy"][0], 2)
        row[key]["mtriangles_per_s"] = round(nt / t[key][0] / 1000.0, 1)
    row["loop"]["atomics_per_ns"] = round(8 * ne / max(t["loop"][0] - t["midpoint"][0], 1e-9) / 1e6, 2)      # over what Loop adds to midpoint
    if args.host:
        for key, code in (("midpoint", 0), ("loop", 1)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            want = sr.subdivide(vertices.cpu().numpy(), faces.cpu().numpy(), code)
            moved = [torch.from_numpy(x).to(dev) for x in want]
            torch.cuda.synchronize()
            row[key]["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            row[key]["host_over_device"] = round(row[key]["host_ms"] / t[key][0], 1)
            level(code)()
            torch.cuda.synchronize()
            row[key]["host_equal"] = bool(int(count.item()) == len(want[0]) and torch.equal(moved[1], out_f) and
                                          torch.equal(moved[2], parents[:total]) and
                                          torch.equal(moved[0].view(torch.int32), out_v[:total].view(torch.int32)))
    return row


def fan(n, dev):
    a = 2 * np.pi * np.arange(n) / n
    v = np.concatenate([np.float32([[0.1, -0.2, 0.7]]), np.stack([np.cos(a), np.sin(a), 0.05 * np.cos(7 * a)], axis=1).astype(np.float32)])
    ring = np.arange(n, dtype=np.int32)
    f = np.stack([np.zeros(n, np.int32), 1 + ring, 1 + (ring + 1) % n], axis=1)
    return torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32,128,256")
    ap.add_argument("--scene", default="dense_monkey")
    ap.add_argument("--scene-size", type=int, default=128)
    ap.add_argument("--fan", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--host", type=int, default=1)
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
        mesh = r.weld(r.isosurface(field, 0.0, lo, hi))
        del field
        emit(measure(r, "sphere %d" % n, mesh.vertices, mesh.faces, args))
        del mesh
    if args.scene:
        sc = drt.Scene()
        sc.loadGLTFmodel(scene_path(args.scene))
        b = drt.BVHBuilder()
        b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
        b.buildIterative(sc)
        mesh = r.weld(r.remesh(sc, args.scene_size))
        emit(measure(r, "remesh %s %d" % (args.scene, args.scene_size), mesh.vertices, mesh.faces, args))
    if args.fan:
        emit(measure(r, "fan %d" % args.fan, *fan(args.fan, dev), args))


if __name__ == "__main__":
    main()
