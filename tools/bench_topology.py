"""Times of the mesh-topology calls (drt_renderer_shell_labels, drt_renderer_boundary_loops, drt_renderer_shell_terms,
kernel_topology.hip) on one scene, beside what every user of them pays once per upload anyway: the host's edge_adjacency() build of
the same scene and the upload of that table.  The library offered no labelling before, so those two are the yardsticks.  One JSON line:
  adjacency_host   Scene.edgeAdjacency(), wall clock
  table_upload     the 12-byte-per-triangle table, host to device
  shells_first     the first drt_renderer_shell_labels after an upload whose table is already on the device: the labelling, the counts
                   and the boundary list (the scene is uploaded again in front of every repeat, outside the timed span)
  shells_cached    the same call again: two copies
  loops            drt_renderer_boundary_loops into slots for every record
  terms            drt_renderer_shell_terms
ms = device events around one call, median / min / max of --reps after --warmup; steps = the labelling steps enqueued, those that did
something and those that hooked.  With --check the labels and the slots are compared with tests/topology_ref.py in the same run.

  python tools/bench_topology.py --scene dense_monkey [--reps 9] [--warmup 3] [--check] [--out file.jsonl]
  python tools/bench_topology.py --scene strip:1048576      (the strip of tests/topology_scenes.py at that many triangles)
  python tools/bench_topology.py --all [--limit 600] [--out file.jsonl]

--all runs cs16_dust, dense_monkey, the band (ring) and the strip of tests/topology_scenes.py, each in a fresh process of its own under
`timeout`, one after the other, and stops at the first step that fails: nothing is retried.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = ("cs16_dust", "dense_monkey", "ring", "strip")


def run_all(args):
    for scene in SCENES:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--scene", scene, "--reps", str(args.reps),
               "--warmup", str(args.warmup)] + (["--check"] if args.check else []) + (["--out", args.out] if args.out else [])
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print("bench_topology: %s ended with status %d: stopping" % (scene, rc), file=sys.stderr)
            return rc
    return 0


def one(args):
    import torch

    import dustraytracer_amd as drt
    from tests import contour_scenes as cs
    from tests import topology_ref as tr
    from tests import topology_scenes as ts
    from tools.nearest_bench import timed
    from tools.overlap_bench import load

    dev = torch.device("cuda", 0)
    r = drt.Renderer(0)
    L = drt._lib
    stream = torch.cuda.current_stream(dev).cuda_stream
    if args.scene.startswith("strip:"):                                       # a strip of that many triangles (not part of --all)
        pos = ts.strip(int(args.scene[6:]) // 2)
        sc = drt.Scene()
        sc.addMaterial(*cs.ONE_MATERIAL[0])
        sc.setGeometry(pos, np.tile(np.float32([0, 0, 1]), (len(pos), 3, 1)), np.zeros((len(pos), 3, 2), np.float32), np.zeros(len(pos), np.int32))
        b = drt.BVHBuilder()
        b.m_TargetLeafPrimitivesCount, b.m_BinCount = 4, 8
        b.buildIterative(sc)
    else:
        sc = ts.scene(drt, args.scene) if args.scene in ts.ALL_NAMES else load(args.scene)
    other = cs.flat_scene(drt, cs.SINGLE)[0]                                  # uploading it drops everything the renderer holds of `sc`
    n = int(L.drt_scene_triangle_count(sc._h))
    row = {"scene": args.scene, "triangles": n}

    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        adj = sc.edgeAdjacency()
        walls.append((time.perf_counter() - t0) * 1e3)
    row["adjacency_host"] = {"ms": round(float(np.median(walls)), 3), "ms_min": round(min(walls), 3), "ms_max": round(max(walls), 3)}
    table = torch.from_numpy(adj).pin_memory()
    on_device = torch.empty((n, 3), dtype=torch.int32, device=dev)
    ms, t_lo, t_hi = timed(lambda: on_device.copy_(table, non_blocking=True), args.reps, args.warmup, 1)
    row["table_upload"] = {"ms": round(ms, 4), "ms_min": round(t_lo, 4), "ms_max": round(t_hi, 4)}

    def ok(rc):
        assert rc == drt.OK, L.drt_last_error()

    labels = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.zeros(3, dtype=torch.int32, device=dev)
    loop_counts = torch.zeros(3, dtype=torch.int32, device=dev)
    terms = torch.empty((n, 4), dtype=torch.float64, device=dev)
    miss = torch.zeros((1, 8), dtype=torch.int32, device=dev)
    miss[0, 3] = -1
    one_split = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    one_slot = torch.empty((1, 4), dtype=torch.int32, device=dev)

    def shells():
        ok(L.drt_renderer_shell_labels(r._h, sc._h, labels.data_ptr(), counts.data_ptr(), stream))

    def forget():
        """The scene uploaded afresh with its table on the device and nothing labelled: another scene, then a chain call on one miss
        record (it uploads the scene and the table, and chains nothing)."""
        ok(L.drt_renderer_shell_terms(r._h, other._h, terms.data_ptr(), stream))
        ok(L.drt_renderer_chain_sections(r._h, sc._h, miss.data_ptr(), one_split.data_ptr(), one_slot.data_ptr(), None, 1, 1, stream))
        torch.cuda.synchronize()

    firsts = []
    for k in range(args.warmup + args.reps):
        forget()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        shells()
        b.record()
        b.synchronize()
        if k >= args.warmup:
            firsts.append(a.elapsed_time(b))
    row["shells_first"] = {"ms": round(float(np.median(firsts)), 4), "ms_min": round(min(firsts), 4), "ms_max": round(max(firsts), 4)}
    row["steps"] = dict(zip(("enqueued", "busy", "hooks"), r.topologySteps()))
    row["shells"], row["open"], row["bad"] = (int(v) for v in counts.cpu().numpy().view(np.uint32))
    m = row["open"]
    slots = torch.empty((max(m, 1), 4), dtype=torch.int32, device=dev)

    def loops():
        ok(L.drt_renderer_boundary_loops(r._h, sc._h, slots.data_ptr() if m else None, m, loop_counts.data_ptr(), stream))

    for key, fn in (("shells_cached", shells), ("loops", loops),
                    ("terms", lambda: ok(L.drt_renderer_shell_terms(r._h, sc._h, terms.data_ptr(), stream)))):
        ms, t_lo, t_hi = timed(fn, args.reps, args.warmup, 1)
        row[key] = {"ms": round(ms, 4), "ms_min": round(t_lo, 4), "ms_max": round(t_hi, 4)}
    torch.cuda.synchronize()
    row["records"], row["loops_found"], row["closed"] = (int(v) for v in loop_counts.cpu().numpy().view(np.uint32))
    row["loop_rounds"] = int(np.ceil(np.log2(max(m, 1))))
    row["first_over_adjacency_host"] = round(row["shells_first"]["ms"] / row["adjacency_host"]["ms"], 4)
    if args.check:
        flat = adj.reshape(-1)
        want = tr.labels(flat)
        want_slots, want_counts = tr.loops(flat)
        row["bit_equal_to_restatement"] = bool(labels.cpu().numpy().tobytes() == want.tobytes()
                                               and slots[:m].cpu().numpy().view(tr.SLOT).reshape(-1).tobytes() == want_slots.tobytes()
                                               and np.array_equal(loop_counts.cpu().numpy().view(np.uint32), want_counts))
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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--limit", type=int, default=600, help="seconds each step of --all may take")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sys.exit(run_all(args) if args.all else one(args))


if __name__ == "__main__":
    main()
