"""Throughput of the triangle casts (Renderer.triangleCast / castsAny, kernel_tri_cast.hip) next to two yardsticks from the same process
at the same commit: drt_renderer_triangle_distance on the same triangles -- the same fifteen feature pairs and the same predicate under
a bound-shrinking search, at 4 waves per SIMD -- and drt_renderer_sphere_cast from each triangle's centroid along the same motion with
the circumscribed radius (the largest centroid-vertex distance) -- the same ray-ordered traversal with a seven-shape test at the leaves,
at 8 waves per SIMD.  One JSON line per scene x query size x direction length (vertices = a centre + uniform offsets in +-size x the
scene's extent; the centres are half near surfaces, half in the scene's box; directions are uniform on the sphere, of length
--lengths x the extent, and tmax = 1):
  first              drt_renderer_triangle_cast in mode FIRST on buffers made beforehand
  any                the same in mode ANY
  tri_distance       drt_renderer_triangle_distance in mode NEAREST with max_dist NULL
  sphere_cast        drt_renderer_sphere_cast, tmin 0, tmax 1
ms = device events around --calls back-to-back queries, median of --reps after --warmup, per query; Mcasts/s = casts / ms / 1000;
ratio_to_tri_distance and ratio_to_sphere_cast = the yardstick's ms / the cast's ms (below 1: the cast is slower).  `hit` is the share
of casts with prim >= 0, `start_overlap` the share with t = 0.  The first --count records of each timed set are compared with the
restatement (tests/tri_cast_ref.py), bit for bit.  Measurements, not pass marks.

  python tools/tri_cast_bench.py [--scenes a,b] [--sizes 0.005,0.02,0.05] [--lengths 0.1,1.0] [--queries N] [--reps 9] [--warmup 2] [--calls 4] [--count 300] [--out file.jsonl]
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
from tests import nearest_ref as nr  # noqa: E402
from tests import tri_cast_ref as tc  # noqa: E402
from tests import tri_overlap_ref as tv  # noqa: E402
from tools.nearest_bench import timed  # noqa: E402
from tools.overlap_bench import load  # noqa: E402


def same(got, want):
    eq = got.view(np.uint32) == want.view(np.uint32)
    floats = [0, 1, 2, 3, 4, 5, 6, 8, 9]
    eq[:, floats] |= np.isnan(got[:, floats]) & np.isnan(want[:, floats])
    return bool(eq.all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell_box,soup")
    ap.add_argument("--sizes", default="0.005,0.02,0.05")
    ap.add_argument("--lengths", default="0.1,1.0")
    ap.add_argument("--queries", type=int, default=1 << 18)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--count", type=int, default=300)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = open(args.out, "a") if args.out else None
    n = args.queries
    for name in args.scenes.split(","):
        sc = load(name)
        g = nr.from_product(sc)
        rng = np.random.default_rng(1234)
        lo, hi = nr.bounds(g)
        extent = float((hi - lo).max())
        centers = np.concatenate([nr.surface_points(g, n // 2, rng), nr.box_points(g, n - n // 2, rng)]).astype(np.float32)
        unit = rng.uniform(-1, 1, (n, 3, 3)).astype(np.float32)
        way = rng.normal(size=(n, 3))
        way = (way / np.linalg.norm(way, axis=1, keepdims=True)).astype(np.float32)
        r = drt.Renderer(0)
        stream = torch.cuda.current_stream(dev).cuda_stream
        records = torch.empty((n, 12), dtype=torch.float32, device=dev)
        near_out = torch.empty((n, 12), dtype=torch.float32, device=dev)
        sweep_out = torch.empty((n, 8), dtype=torch.float32, device=dev)
        for size in (float(s) for s in args.sizes.split(",")):
            host_q = (centers[:, None, :] + unit * np.float32(size * extent)).astype(np.float32)
            tris = torch.from_numpy(tv.pack(host_q)).to(dev)
            centroid = host_q.mean(axis=1).astype(np.float32)
            radii = torch.from_numpy(np.linalg.norm(host_q - centroid[:, None, :], axis=2).max(axis=1).astype(np.float32)).to(dev)
            for length in (float(s) for s in args.lengths.split(",")):
                host_d = (way * np.float32(length * extent)).astype(np.float32)
                motions = torch.ones((n, 4), dtype=torch.float32, device=dev)          # tmax = 1
                motions[:, 0:3] = torch.from_numpy(host_d).to(dev)
                rays = torch.zeros((n, 8), dtype=torch.float32, device=dev)            # drt_ray {org, tmin = 0, dir, tmax = 1}
                rays[:, 0:3], rays[:, 4:7], rays[:, 7] = torch.from_numpy(centroid).to(dev), motions[:, 0:3], 1.0

                def cast(mode):
                    rc = drt._lib.drt_renderer_triangle_cast(r._h, sc._h, tris.data_ptr(), motions.data_ptr(), records.data_ptr(), n, mode, stream)
                    assert rc == drt.OK, drt._lib.drt_last_error()

                def tri_distance():
                    rc = drt._lib.drt_renderer_triangle_distance(r._h, sc._h, tris.data_ptr(), None, near_out.data_ptr(), n, drt.TRIDIST_NEAREST, stream)
                    assert rc == drt.OK, drt._lib.drt_last_error()

                def sphere_cast():
                    rc = drt._lib.drt_renderer_sphere_cast(r._h, sc._h, rays.data_ptr(), radii.data_ptr(), sweep_out.data_ptr(), n, stream)
                    assert rc == drt.OK, drt._lib.drt_last_error()

                row = {"scene": name, "triangles": len(g.v0), "bvh_depth": sc.bvh_depth, "casts": n, "size_over_extent": size,
                       "length_over_extent": length}
                m = min(args.count, n)
                checks = {}
                for key, mode, fn in (("first", drt.TRICAST_FIRST, lambda: cast(drt.TRICAST_FIRST)), ("any", drt.TRICAST_ANY, lambda: cast(drt.TRICAST_ANY)),
                                      ("tri_distance", None, tri_distance), ("sphere_cast", None, sphere_cast)):
                    ms, t_lo, t_hi = timed(fn, args.reps, args.warmup, args.calls)
                    row[key] = {"ms": round(ms, 4), "ms_min": round(t_lo, 4), "ms_max": round(t_hi, 4), "mcasts_per_s": round(n / ms / 1000.0, 1)}
                    if mode is not None:
                        torch.cuda.synchronize()
                        got = records[:m].cpu().numpy()
                        prim = records.view(torch.int32)[:, 7]
                        if mode == drt.TRICAST_FIRST:
                            row["hit"] = round(float((prim >= 0).double().mean().item()), 4)
                            row["start_overlap"] = round(float(((prim >= 0) & (records[:, 3] == 0)).double().mean().item()), 4)
                        checks[key] = same(got, tc.records(tc.cast(g, host_q[:m], host_d[:m], 1.0, mode)))
                for key in ("first", "any"):
                    row[key]["ratio_to_tri_distance"] = round(row["tri_distance"]["ms"] / row[key]["ms"], 3)
                    row[key]["ratio_to_sphere_cast"] = round(row["sphere_cast"]["ms"] / row[key]["ms"], 3)
                row["bit_equal_to_restatement"] = checks
                line = json.dumps(row)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()


if __name__ == "__main__":
    main()
