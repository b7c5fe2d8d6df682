"""Times of the section-contour call (drt_renderer_chain_sections, kernel_contour.hip) for axis-2 slices of a scene, beside the
plane-section fill that wrote the records it chains (drt_renderer_plane_sections into segments made beforehand): the library offered no
chaining before, so the fill is the yardstick a user feels.  One JSON line per step:
  fill     the section fill of the planes' records
  chain    the chain call on those records, with the per-plane counts
ms = device events around one call, median / min / max of --reps after --warmup; chain_over_fill = chain ms / fill ms; rounds = the
jumping rounds launched, ceil(log2(records)); longest_chain = the longest chain found.  The first --check planes are compared with the
restatement (tests/contour_ref.py) in the same run.

  python tools/bench_contours.py --scene dense_monkey --planes 1024 [--reps 9] [--warmup 3] [--check 8] [--out file.jsonl]
  python tools/bench_contours.py --scene ring            (the 5 000-record ring of tests/contour_scenes.py alone: one closed chain)
  python tools/bench_contours.py --all [--limit 300] [--out file.jsonl]

--all runs every step of the table -- dense_monkey and cs16_dust at 64, 1024 and 16384 planes, then the ring -- in a fresh process of
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
    steps = [(scene, planes) for scene in SCENES for planes in PLANES] + [("ring", 1)]
    for scene, planes in steps:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--scene", scene, "--planes", str(planes),
               "--reps", str(args.reps), "--warmup", str(args.warmup), "--check", str(args.check)]
        if args.out:
            cmd += ["--out", args.out]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print("bench_contours: %s at %d planes ended with status %d: stopping" % (scene, planes, rc), file=sys.stderr)
            return rc
    return 0


def one(args):
    import torch

    import dustraytracer_amd as drt
    from tests import contour_ref as cr
    from tests import contour_scenes as cs
    from tests import section_ref as sr
    from tools.nearest_bench import timed
    from tools.overlap_bench import load

    dev = torch.device("cuda", 0)
    r = drt.Renderer(0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    if args.scene == "ring":
        sc, _ = cs.scene(drt, "ring")
        planes = torch.tensor([[0.0, 0.0, 1.0, 0.0]], dtype=torch.float32, device=dev)
    else:
        sc = load(args.scene)
        nodes = sc.m_BVHNodes
        lo, hi = np.asarray(nodes[-1]["bmin"], np.float32), np.asarray(nodes[-1]["bmax"], np.float32)
        heights = float(lo[2]) + (torch.arange(args.planes, dtype=torch.float32, device=dev) + 0.5) * (float(hi[2] - lo[2]) / args.planes)
        planes = torch.zeros((args.planes, 4), dtype=torch.float32, device=dev)
        planes[:, 2], planes[:, 3] = 1.0, heights
    n = planes.shape[0]
    sec = r.planeSections(sc, planes)
    total = int(sec.prim.shape[0])
    rec = torch.empty((max(total, 1), 8), dtype=torch.float32, device=dev)
    slots = torch.empty((max(total, 1), 4), dtype=torch.int32, device=dev)
    chains = torch.empty((n, 2), dtype=torch.int32, device=dev)

    def fill():
        rc = drt._lib.drt_renderer_plane_sections(r._h, sc._h, planes.data_ptr(), sec.splits.data_ptr(), rec.data_ptr(), total, None, n, drt.SECTION_LIST, stream)
        assert rc == drt.OK, drt._lib.drt_last_error()

    def chain():
        rc = drt._lib.drt_renderer_chain_sections(r._h, sc._h, rec.data_ptr(), sec.splits.data_ptr(), slots.data_ptr(), chains.data_ptr(), n, total, stream)
        assert rc == drt.OK, drt._lib.drt_last_error()

    row = {"scene": args.scene, "triangles": int(drt._lib.drt_scene_triangle_count(sc._h)), "planes": n, "records": total,
           "rounds": int(np.ceil(np.log2(max(total, 1))))}
    assert total > 0
    fill()
    for key, fn in (("fill", fill), ("chain", chain)):
        ms, t_lo, t_hi = timed(fn, args.reps, args.warmup, 1)
        row[key] = {"ms": round(ms, 4), "ms_min": round(t_lo, 4), "ms_max": round(t_hi, 4)}
    row["chain_over_fill"] = round(row["chain"]["ms"] / row["fill"]["ms"], 2)
    torch.cuda.synchronize()
    starts = slots[:, 1] == torch.arange(total, dtype=torch.int32, device=dev)
    row["chains"], row["closed"] = int(chains[:, 0].sum().item()), int(chains[:, 1].sum().item())
    row["longest_chain"] = int(slots[:, 2][starts].max().item())
    m = min(args.check, n)
    if m:
        adj = cr.adjacency(cs.tree_positions(sc))
        assert np.array_equal(sc.edgeAdjacency().reshape(-1), adj)
        splits = sec.splits.cpu().numpy()[:m + 1]
        host = np.zeros(int(splits[-1]), sr.SECTION)                          # (the link reads prim and code alone)
        host["prim"], host["code"] = sec.prim[:len(host)].cpu().numpy(), sec.code[:len(host)].cpu().numpy()
        want, want_chains = cr.chain(adj, host, splits)
        got = slots[:len(host)].cpu().numpy().view(cr.SLOT).reshape(-1)
        row["bit_equal_to_restatement"] = bool(got.tobytes() == want.tobytes()
                                               and np.array_equal(chains[:m].cpu().numpy().view(np.uint32), want_chains))
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return 0 if row.get("bit_equal_to_restatement", True) else 1


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
