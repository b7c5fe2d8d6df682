"""Times of the plane-section query (drt_renderer_plane_sections, kernel_section.hip: one wave per plane) for axis-2 slices of a scene,
next to what the library offered before it: drt_renderer_overlap_boxes with zero-thickness slabs that cover the scene at the same
heights (one box per lane, the one-record-per-step insert).  The two do not answer the same question -- a slab lists every triangle
that TOUCHES the plane by index, 4 bytes each; a section lists every triangle that is CUT with its segment, 32 bytes each -- so the
mean list lengths are printed beside the times.  One JSON line per (scene, planes):
  count, fill            the section query with capacity 0 on buffers made beforehand, and the fill into segments made beforehand
                         from that count (offsets = the exclusive scan)
  box_count, box_fill    the same two passes of the box query on the slabs
ms = device events around one call, median / min / max of --reps after --warmup; ratio = box ms / section ms.  The first --check
planes are compared with the restatement (tests/section_ref.py).

  python tools/bench_sections.py --scene dense_monkey --planes 1024 [--reps 9] [--warmup 3] [--check 8] [--out file.jsonl]
  python tools/bench_sections.py --all [--limit 300] [--out file.jsonl]

--all runs every (scene, planes) step of the table -- dense_monkey and cs16_dust at 64, 1024 and 16384 planes -- in a fresh process of
its own under `timeout`, one after the other, and stops at the first step that fails: nothing is retried.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = ("dense_monkey", "cs16_dust")
PLANES = (64, 1024, 16384)


def run_all(args):
    for scene in SCENES:
        for planes in PLANES:
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--scene", scene, "--planes", str(planes),
                   "--reps", str(args.reps), "--warmup", str(args.warmup), "--check", str(args.check)]
            if args.out:
                cmd += ["--out", args.out]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                print("bench_sections: %s at %d planes ended with status %d: stopping" % (scene, planes, rc), file=sys.stderr)
                return rc
    return 0


def one(args):
    import torch

    import dustraytracer_amd as drt
    from tests import nearest_ref as nr
    from tests import section_ref as sr
    from tools.nearest_bench import timed
    from tools.overlap_bench import load

    dev = torch.device("cuda", 0)
    sc = load(args.scene)
    n = args.planes
    r = drt.Renderer(0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    nodes = sc.m_BVHNodes
    lo, hi = np.asarray(nodes[-1]["bmin"], np.float32), np.asarray(nodes[-1]["bmax"], np.float32)
    heights = float(lo[2]) + (torch.arange(n, dtype=torch.float32, device=dev) + 0.5) * (float(hi[2] - lo[2]) / n)     # Renderer.slices' own
    planes = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    planes[:, 2], planes[:, 3] = 1.0, heights
    boxes = torch.zeros((n, 16), dtype=torch.float32, device=dev)             # slabs: the scene's extent in x and y, no thickness
    boxes[:, 0], boxes[:, 1], boxes[:, 2] = float(lo[0] + hi[0]) / 2, float(lo[1] + hi[1]) / 2, heights
    boxes[:, 3], boxes[:, 4] = float(hi[0] - lo[0]) / 2, float(hi[1] - lo[1]) / 2
    boxes[:, 6], boxes[:, 10], boxes[:, 14] = 1.0, 1.0, 1.0
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    no_room = torch.zeros(n + 1, dtype=torch.int32, device=dev)

    def section(offsets, out, capacity, cnt):
        rc = drt._lib.drt_renderer_plane_sections(r._h, sc._h, planes.data_ptr(), offsets.data_ptr(), None if out is None else out.data_ptr(), capacity,
                                                  None if cnt is None else cnt.data_ptr(), n, drt.SECTION_LIST, stream)
        assert rc == drt.OK, drt._lib.drt_last_error()

    def box(offsets, out, capacity, cnt):
        rc = drt._lib.drt_renderer_overlap_boxes(r._h, sc._h, boxes.data_ptr(), offsets.data_ptr(), None if out is None else out.data_ptr(), capacity,
                                                 None if cnt is None else cnt.data_ptr(), n, drt.OVERLAP_LIST, stream)
        assert rc == drt.OK, drt._lib.drt_last_error()

    row = {"scene": args.scene, "triangles": int(drt._lib.drt_scene_triangle_count(sc._h)), "bvh_depth": sc.bvh_depth, "planes": n}
    jobs = []
    for key, call, width in (("", section, 8), ("box_", box, 1)):
        call(no_room, None, 0, counts)
        splits = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        splits[1:] = torch.cumsum(counts.to(torch.int64), dim=0)
        total = int(splits[-1].item())
        assert total < 2 ** 31
        row[key + "records"] = total
        row[key + "mean_list"] = round(total / n, 1)
        row[key + "longest_list"] = int(counts.max().item())
        offsets = splits.to(torch.int32)
        out = torch.empty((max(total, 1), width), dtype=torch.int32, device=dev)
        jobs.append((key + "count", lambda call=call: call(no_room, None, 0, counts)))
        if total:
            jobs.append((key + "fill", lambda call=call, offsets=offsets, out=out, total=total: call(offsets, out, total, None)))
    for key, fn in jobs:
        ms, t_lo, t_hi = timed(fn, args.reps, args.warmup, 1)
        row[key] = {"ms": round(ms, 4), "ms_min": round(t_lo, 4), "ms_max": round(t_hi, 4)}
    for key in ("count", "fill"):
        if key in row and "box_" + key in row:
            row[key]["box_over_section"] = round(row["box_" + key]["ms"] / row[key]["ms"], 3)
    m = min(args.check, n)
    if m:
        g = nr.from_product(sc)
        host = planes[:m].cpu().numpy()
        full, totals = sr.whole(g, host)
        got = r.planeSections(sc, host)
        rec = np.zeros(len(got.prim), sr.SECTION)
        rec["p"], rec["q"], rec["prim"], rec["code"] = got.p, got.q, got.prim, got.code
        row["bit_equal_to_restatement"] = bool(rec.tobytes() == full.tobytes() and np.array_equal(np.diff(got.splits), totals.astype(np.int64)))
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--scene", default="dense_monkey")
    ap.add_argument("--planes", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", type=int, default=8)
    ap.add_argument("--limit", type=int, default=300, help="seconds each step of --all may take")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sys.exit(run_all(args) if args.all else one(args))


if __name__ == "__main__":
    main()
