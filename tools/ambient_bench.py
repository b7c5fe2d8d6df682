"""Time of ambient occlusion (Renderer.ambientOcclusion, kernel_ambient.hip) next to its yardstick from the same process at the same
commit.  One JSON line per scene (cornell_box; the 10^6-triangle soup of the BVH build figure, built on the GPU), setting by setting:
--points points drawn by sampleSurface with their face normals, S = 16, 64 and 256 samples, max_dist = inf and 5 % of the scene's
diagonal.
  ambient      drt_renderer_ambient_occlusion: the rays made in registers, traced and reduced per point
  occluded     drt_renderer_occluded on the same N S rays, made beforehand (the restatement's rule, on the host) and read from memory: the
               traversal floor plus the ray reads the fused kernel saves; ratio = ambient ms / occluded ms
  composed     what a caller composes today: ray generation in torch (cosine-weighted directions from torch.randn: the cost of the
               renderer's sampler restated in torch, not its directions), occluded, and the reduction of the booleans and directions
  utilisation  lanes that took a traversal step / (64 x trips of the waves' loops) of the tile form, from the kernel's counting build
               (drt_debug_ambient_stats), in a call of its own
ms = device events around --calls back-to-back calls, median of --reps rounds after --warmup, per call, with the fastest and slowest
round; within a round ambient, occluded and composed alternate.  The first --count records of every setting are compared with the
restatement (tests/ambient_ref.py): on cornell_box all of it, on the soup its rays and its sums with the traversal by
Renderer.occluded (which tests/test_gpu_ray_query.py holds to the restatement).  Measurements, not pass marks.

  python tools/ambient_bench.py [--scenes cornell_box,soup] [--points 65536] [--reps 15] [--warmup 3] [--calls 4] [--count 64] [--out file.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import dustraytracer_amd as drt  # noqa: E402
import oracle  # noqa: E402
from tests import ambient_ref as ar  # noqa: E402
from tests.scenes import scene_path  # noqa: E402
from tools.intersect_bench import soup  # noqa: E402
from tools.overlap_bench import load  # noqa: E402

F = np.float32


def restated_rays(pts, samples, seed):
    """drt_ray [N S, 8] on the device: the rays the fused kernel makes, from the restatement's rule on the host (tests/ambient_ref.py)."""
    h = pts.cpu().numpy()
    o, d, _ = ar.rays(h[:, 0:3], h[:, 4:7], h[:, 7], samples, seed)
    rays = np.zeros((len(h) * samples, 8), F)
    rays[:, 0:3], rays[:, 4:7], rays[:, 7] = np.repeat(o, samples, axis=0), d.reshape(-1, 3), np.repeat(h[:, 3], samples)
    return torch.from_numpy(rays).to(pts.device)


def composed(r, sc, pts, samples, gen):
    """The three calls a caller makes today: rays in torch, occluded, the reduction."""
    n = pts.shape[0]
    fuzz = torch.nn.functional.normalize(torch.randn((n * samples, 3), dtype=torch.float32, device=pts.device, generator=gen), dim=1)
    d = torch.nn.functional.normalize(pts[:, 4:7].repeat_interleave(samples, dim=0) + fuzz, dim=1)
    o = (pts[:, 0:3] + pts[:, 4:7] * pts[:, 7:8]).repeat_interleave(samples, dim=0)
    occ = r.occluded(sc, o, d, 0.0, pts[:, 3].repeat_interleave(samples))
    is_open = ~occ.reshape(n, samples)
    return is_open.sum(dim=1), (d.reshape(n, samples, 3) * is_open[:, :, None]).sum(dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell_box,soup")
    ap.add_argument("--points", type=int, default=1 << 16)
    ap.add_argument("--triangles", type=int, default=1000000)
    ap.add_argument("--samples", default="16,64,256")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--count", type=int, default=64)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out_file = open(args.out, "a") if args.out else None
    n = args.points
    L = drt._lib
    for name in args.scenes.split(","):
        sc = soup(args.triangles) if name == "soup" else load(name)
        osc = None if name == "soup" else oracle.Scene.load_glb(scene_path(name)).build_bvh(20, 8)
        r = drt.Renderer(0)
        stream = torch.cuda.current_stream(dev).cuda_stream
        smp = r.sampleSurface(sc, n, seed=3, as_torch=True)
        surf = r.surface(sc, smp)
        lo, hi = surf.position.min(dim=0).values, surf.position.max(dim=0).values
        diagonal = float(torch.linalg.norm(hi - lo))
        row = {"scene": name, "triangles": int(L.drt_scene_triangle_count(sc._h)), "points": n, "diagonal": round(diagonal, 3), "settings": []}
        gen = torch.Generator(device=dev).manual_seed(5)
        for reach_name, reach in (("inf", float("inf")), ("5% of the diagonal", 0.05 * diagonal)):
            pts = torch.zeros((n, 8), dtype=torch.float32, device=dev)                      # drt_ao_point {p, max_dist, n, bias}
            pts[:, 0:3], pts[:, 3], pts[:, 4:7], pts[:, 7] = surf.position, reach, surf.normal, 0.001
            for samples in [int(x) for x in args.samples.split(",")]:
                rays = restated_rays(pts, samples, 9)
                result = torch.empty((n, 4), dtype=torch.int32, device=dev)
                occ = torch.empty(n * samples, dtype=torch.uint8, device=dev)
                params = (C.c_uint32 * 4)(samples, 9, 0, 0)

                def ambient():
                    assert L.drt_renderer_ambient_occlusion(r._h, sc._h, pts.data_ptr(), n, C.addressof(params), result.data_ptr(), stream) == drt.OK, L.drt_last_error()

                def occluded():
                    assert L.drt_renderer_occluded(r._h, sc._h, rays.data_ptr(), occ.data_ptr(), n * samples, stream) == drt.OK, L.drt_last_error()

                fns = (("ambient", ambient), ("occluded", occluded), ("composed", lambda: composed(r, sc, pts, samples, gen)))
                times = {key: [] for key, _ in fns}
                for rep in range(args.warmup + args.reps):
                    for key, fn in fns:                                                     # alternating within a round
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        for _ in range(args.calls):
                            fn()
                        b.record()
                        b.synchronize()
                        if rep >= args.warmup:
                            times[key].append(a.elapsed_time(b) / args.calls)
                item = {"samples": samples, "max_dist": reach_name}
                for key, t in times.items():
                    item[key] = {"ms": round(float(np.median(t)), 4), "ms_min": round(float(np.min(t)), 4), "ms_max": round(float(np.max(t)), 4)}
                item["ratio_to_occluded"] = round(item["ambient"]["ms"] / item["occluded"]["ms"], 3)
                item["ratio_composed_to_ambient"] = round(item["composed"]["ms"] / item["ambient"]["ms"], 2)
                item["grays_per_s"] = round(n * samples / item["ambient"]["ms"] / 1e6, 3)
                item["occluded_grays_per_s"] = round(n * samples / item["occluded"]["ms"] / 1e6, 3)
                # the records against the yardstick's booleans (all points) and against the restatement (the first --count)
                torch.cuda.synchronize()
                got = result.cpu().numpy()
                item["open_fraction"] = round(float(got[:, 0].sum()) / (n * samples), 4)
                item["open_equals_occluded_on_the_same_rays"] = bool((got[:, 0] == samples - occ.cpu().numpy().reshape(n, samples).sum(axis=1)).all())
                m = min(args.count, n)
                h = pts[:m].cpu().numpy()
                if osc is not None:
                    want = ar.ambient(osc, h[:, 0:3], h[:, 4:7], h[:, 3], h[:, 7], samples, 9)
                else:
                    o, d, _ = ar.rays(h[:, 0:3], h[:, 4:7], h[:, 7], samples, 9)
                    blocked = r.occluded(sc, np.repeat(o, samples, axis=0), np.ascontiguousarray(d.reshape(-1, 3)), 0.0, np.repeat(h[:, 3], samples)).reshape(m, samples)
                    want = np.concatenate([(~blocked).sum(axis=1)[:, None], (ar.bent_terms(d) * ~blocked[:, :, None]).sum(axis=1)], axis=1)
                item["first_records_equal_the_restatement"] = bool((got[:m] == want).all())
                # lane utilisation, from the counting build in a call of its own
                counts = (C.c_uint64 * 2)()
                assert L.drt_debug_ambient_stats(r._h, 1, None) == drt.OK
                ambient()
                assert L.drt_debug_ambient_stats(r._h, 0, C.addressof(counts)) == drt.OK
                item["utilisation"] = round(int(counts[1]) / max(64 * int(counts[0]), 1), 4)
                item["counting_build_same_records"] = bool((result.cpu().numpy() == got).all())
                row["settings"].append(item)
                del rays, occ
        line = json.dumps(row)
        print(line, flush=True)
        if out_file:
            out_file.write(line + "\n")
            out_file.flush()


if __name__ == "__main__":
    main()
