"""Throughput of the inside vote and the signed distance (Renderer.inside / signedDistance, kernel_crossings.hip), next to two
baselines from the same run: nearest alone, and three occluded calls on the vote's own rays (what a user had to build a parity
test from -- it stops at the first hit, so it is a lower bound on the traversal work, not an alternative).  One JSON line per scene x
point set, tools/nearest_bench.py's sets:
  near     points within 1 % of the scene's extent of a surface
  in_box   uniform in the scene's box
  far      uniform in a box ten times larger about the same centre
ms = device events around --calls back-to-back queries, median of --reps after --warmup, per query; Mpoints/s = points / ms / 1000.
`crossings_per_point` = mean triangles counted over the three rays, and the share of points inside, from Renderer.crossings /
inside on the whole set; the first --count points are compared with the restatement (tests/inside_ref.py).

  python tools/inside_bench.py [--scenes a,b] [--points N] [--reps 15] [--warmup 3] [--calls 8] [--count 1000] [--out file.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import dustraytracer_amd as drt  # noqa: E402
from tests import inside_ref as ir  # noqa: E402
from tests import nearest_ref as nr  # noqa: E402
from tests.scenes import scene_path  # noqa: E402
from tools.nearest_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="dense_monkey,cs16_dust")
    ap.add_argument("--points", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--count", type=int, default=1000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = open(args.out, "a") if args.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for name in args.scenes.split(","):
        sc = drt.Scene()
        sc.loadGLTFmodel(scene_path(name))
        b = drt.BVHBuilder()
        b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
        b.buildIterative(sc)
        g, osc = nr.from_product(sc), ir.product_scene(sc)
        rng = np.random.default_rng(1234)
        n = args.points
        lo, hi = nr.bounds(g)
        d = rng.normal(size=(n, 3))
        d *= rng.uniform(0, 0.01 * float((hi - lo).max()), (n, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
        sets = {"near": (nr.surface_points(g, n, rng, offset=0.0) + d).astype(np.float32), "in_box": nr.box_points(g, n, rng),
                "far": nr.box_points(g, n, rng, 10.0)}
        r = drt.Renderer(0)
        for set_name, pts in sets.items():
            p = torch.cat([torch.from_numpy(pts), torch.full((n, 1), float("inf"))], dim=1).to(dev)      # packed: nothing but the query is timed
            rays = []
            for k in range(3):
                q = torch.empty((n, 8), dtype=torch.float32, device=dev)
                q[:, 0:3], q[:, 3], q[:, 7] = p[:, 0:3], 0.0, float("inf")
                q[:, 4:7] = torch.from_numpy(ir.DIRS[k]).to(dev)
                rays.append(q)
            row = {"scene": name, "triangles": len(g.v0), "bvh_depth": sc.bvh_depth, "points_set": set_name, "points": n}
            for key, fn in (("inside", lambda: r.inside(sc, p, votes=True)), ("inside_winding", lambda: r.inside(sc, p, rule="winding", votes=True)),
                            ("signed_distance", lambda: r.signedDistance(sc, p)), ("nearest", lambda: r.nearest(sc, p)),
                            ("occluded_x3", lambda: [r.occluded(sc, q) for q in rays]), ("crossings_x3", lambda: [r.crossings(sc, q) for q in rays])):
                ms, t_lo, t_hi = timed(fn, args.reps, args.warmup, args.calls)
                row[key] = {"ms": round(ms, 4), "ms_min": round(t_lo, 4), "ms_max": round(t_hi, 4), "mpoints_per_s": round(n / ms / 1000.0, 1)}
            counts = sum(r.crossings(sc, q).count.sum().item() for q in rays)
            row["crossings_per_point"] = round(counts / n, 2)
            row["inside_share"] = round(float(r.inside(sc, p).float().mean().item()), 4)
            m = min(args.count, n)
            same = np.array_equal(r.inside(sc, pts[:m], votes=True), ir.votes(osc, pts[:m]))
            sd, ref = r.signedDistance(sc, pts[:m]), ir.signed_distance(osc, pts[:m], g=g)
            same = same and all(np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)) for a, b in zip(sd, ref))
            row["bit_equal_to_restatement"] = bool(same)
            emit(row)


if __name__ == "__main__":
    main()
