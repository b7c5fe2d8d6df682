"""Throughput of the generalised winding numbers (Renderer.windingNumbers, kernel_winding.hip) next to the inside vote on the same
points (Renderer.inside, kernel_crossings.hip), the exact sum the hierarchy replaces, and the cost of the moments after a refit next to
the refit itself.  One JSON line per scene x point set, tools/nearest_bench.py's sets:
  near     points within 1 % of the scene's extent of a surface
  in_box   uniform in the scene's box
  far      uniform in a box ten times larger about the same centre
ms = device events around --calls back-to-back queries, median of --reps after --warmup, per query; Mpoints/s = points / ms / 1000.
beta = inf runs on the first --exact-points points, one call per measurement.  `error`: the largest |w(beta) - w(inf)| over those
points and the largest |w(inf) - float64 brute force| over the first --count of them; scenes of at most --restate-triangles triangles
also compare the first --count answers at beta = 2 with the restatement (tests/winding_ref.py).  One more line per scene: ms of
Renderer.refit, of the first winding call on 64 points after it (which makes the moments) and of the same call again.

  python tools/winding_bench.py [--scenes a,b] [--points N] [--reps 15] [--warmup 3] [--calls 8] [--exact-points 262144] [--count 200]
                                [--restate-triangles 20000] [--out file.jsonl]
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
from tests import winding_ref as wr  # noqa: E402
from tests.scenes import scene_path  # noqa: E402
from tools.nearest_bench import timed  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="dense_monkey,cs16_dust")
    ap.add_argument("--points", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--exact-points", type=int, default=1 << 18)
    ap.add_argument("--count", type=int, default=200)
    ap.add_argument("--restate-triangles", type=int, default=20000)
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
        mom = wr.moments(osc) if len(g.v0) <= args.restate_triangles else None
        for set_name, pts in sets.items():
            p = torch.cat([torch.from_numpy(pts), torch.full((n, 1), float("inf"))], dim=1).to(dev)      # packed: nothing but the query is timed
            row = {"scene": name, "triangles": len(g.v0), "bvh_depth": sc.bvh_depth, "points_set": set_name, "points": n}
            for key, fn in (("winding_beta2", lambda: r.windingNumbers(sc, p)), ("winding_beta3", lambda: r.windingNumbers(sc, p, beta=3.0)),
                            ("winding_beta4", lambda: r.windingNumbers(sc, p, beta=4.0)), ("winding_inside", lambda: r.windingInside(sc, p)),
                            ("winding_signed_distance", lambda: r.windingSignedDistance(sc, p)),
                            ("inside", lambda: r.inside(sc, p, votes=True)), ("signed_distance", lambda: r.signedDistance(sc, p))):
                ms, t_lo, t_hi = timed(fn, args.reps, args.warmup, args.calls)
                row[key] = {"ms": round(ms, 4), "ms_min": round(t_lo, 4), "ms_max": round(t_hi, 4), "mpoints_per_s": round(n / ms / 1000.0, 1)}
            row["beta2_over_inside"] = round(row["winding_beta2"]["ms"] / row["inside"]["ms"], 3)
            m = min(args.exact_points, n)
            pe = p[:m].contiguous()
            ms, t_lo, t_hi = timed(lambda: r.windingNumbers(sc, pe, beta=float("inf")), max(3, args.reps // 5), 1, 1)
            row["winding_exact"] = {"points": m, "ms": round(ms, 4), "ms_min": round(t_lo, 4), "ms_max": round(t_hi, 4), "mpoints_per_s": round(m / ms / 1000.0, 4)}
            ms, _, _ = timed(lambda: r.windingNumbers(sc, pe), args.reps, args.warmup, args.calls)
            row["winding_beta2_same_points"] = {"points": m, "ms": round(ms, 4)}
            exact = r.windingNumbers(sc, pe, beta=float("inf"))
            row["error"] = {"beta%d_vs_exact" % beta: round(float((r.windingNumbers(sc, pe, beta=float(beta)) - exact).abs().max().item()), 6) for beta in (2, 3, 4)}
            k = min(args.count, m)
            row["error"]["exact_vs_float64"] = float(np.abs(exact[:k].cpu().numpy().astype(np.float64) - wr.brute_force64(osc.tris["p"], pts[:k])).max())
            row["inside_share"] = {"winding": round(float(r.windingInside(sc, p).float().mean().item()), 4),
                                   "parity": round(float(r.inside(sc, p).float().mean().item()), 4)}
            if mom is not None:
                got, ref = r.windingNumbers(sc, pts[:k]), wr.winding(osc, pts[:k], 2.0, mom)
                row["bit_equal_to_restatement"] = bool(((got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))).all())
            else:
                row["bit_equal_to_restatement"] = None
            emit(row)
        # the moments after a refit next to the refit: the same positions again, so the answers stay
        pos = torch.from_numpy(np.ascontiguousarray(sc.m_PrimitivesBuffer["vertex"]["position"][np.argsort(sc.triangleOrder())], np.float32)).to(dev)
        p64 = torch.cat([torch.from_numpy(sets["in_box"][:64]), torch.full((64, 1), float("inf"))], dim=1).to(dev)
        before = r.windingNumbers(sc, p64).clone()
        refit, first, again = [], [], []
        for _ in range(args.reps + args.warmup):
            refit.append(r.refit(sc, pos))
            first.append(event_ms(lambda: r.windingNumbers(sc, p64)))
            again.append(event_ms(lambda: r.windingNumbers(sc, p64)))
        refit, first, again = [float(np.median(v[args.warmup:])) for v in (refit, first, again)]
        emit({"scene": name, "triangles": len(g.v0), "bvh_depth": sc.bvh_depth, "refit_ms": round(refit, 4),
              "first_winding_call_after_refit_ms": round(first, 4), "same_call_again_ms": round(again, 4), "moments_ms": round(first - again, 4),
              "moments_over_refit": round((first - again) / refit, 3),
              "answers_unchanged": bool(torch.equal(r.windingNumbers(sc, p64).view(torch.int32), before.view(torch.int32)))})


if __name__ == "__main__":
    main()
