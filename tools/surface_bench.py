"""Time of the surface lookups and the area-weighted sampling (Renderer.surface / sampleSurface, kernel_surface.hip) next to their
yardsticks from the same process at the same commit.  One JSON line per scene (cornell_box; the 10^6-triangle soup of the BVH build
figure, built on the GPU):
  lookup_coherent    drt_renderer_surface_lookup on --refs references that are the closest hits of a camera's rays, pixel after pixel
  lookup_random      the same on a random permutation of them
  copy               a device-to-device copy of as many bytes as a lookup reads and writes at the least (16 B in, 96 B out per
                     reference: 56 B copied = 112 B of traffic), the yardstick; ratio_to_copy = the lookup's ms / the copy's ms
  trace_rays         drt_renderer_trace_rays on the rays that made the references: what a lookup adds to a query
  weights            drt_renderer_surface_weights alone (the amax pass and the three phases of the scan)
  sample             drt_renderer_sample_surface for --refs samples (weights + draw); draw = sample - weights
ms = device events around --calls back-to-back calls, median of --reps after --warmup, per call, with min and max.  The first
--count records of every timed set are compared with the restatement (tests/surface_ref.py), bit for bit.  Measurements, not pass marks.

  python tools/surface_bench.py [--scenes cornell_box,soup] [--refs 1048576] [--reps 15] [--warmup 3] [--calls 8] [--count 300] [--out file.jsonl]
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
from tests import surface_ref as sr  # noqa: E402
from tests.scenes import SCENES  # noqa: E402
from tools.intersect_bench import soup  # noqa: E402
from tools.nearest_bench import timed  # noqa: E402
from tools.overlap_bench import load  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell_box,soup")
    ap.add_argument("--refs", type=int, default=1 << 20)
    ap.add_argument("--triangles", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--count", type=int, default=300)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = open(args.out, "a") if args.out else None
    n = args.refs
    width = 1024
    height = (n + width - 1) // width
    for name in args.scenes.split(","):
        if name == "soup":
            sc = soup(args.triangles)
            cam = drt.Camera((0.0, 0.0, 30.0))
            cam.m_Forward_dir = np.array((0.0, 0.0, -1.0), np.float32)
        else:
            sc = load(name)
            cam = drt.Camera(SCENES[name][1])
            cam.m_Forward_dir = np.array(SCENES[name][2], np.float32)
        s = sr.from_product(sc)
        r = drt.Renderer(0)
        stream = torch.cuda.current_stream(dev).cuda_stream
        cr = r.cameraRays(cam, width, height, 1, as_torch=True)[0].reshape(-1, 8)[:n]
        rays = torch.zeros((n, 8), dtype=torch.float32, device=dev)                       # drt_ray {org, tmin = 0, dir, tmax}
        rays[:, 0:3], rays[:, 4:7], rays[:, 7] = cr[:, 0:3], cr[:, 4:7], drt.FLT_MAX
        hits = torch.empty((n, 4), dtype=torch.float32, device=dev)
        records = torch.empty((n, 24), dtype=torch.float32, device=dev)
        samples = torch.empty((n, 4), dtype=torch.float32, device=dev)
        table = torch.empty(len(s.v0), dtype=torch.int64, device=dev)
        src = torch.empty(n * 56 // 4, dtype=torch.float32, device=dev)
        dst = torch.empty_like(src)

        def trace():
            assert drt._lib.drt_renderer_trace_rays(r._h, sc._h, rays.data_ptr(), hits.data_ptr(), n, stream) == drt.OK, drt._lib.drt_last_error()

        trace()
        torch.cuda.synchronize()
        shuffled = hits[torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(1))].contiguous()

        def lookup(refs):
            assert drt._lib.drt_renderer_surface_lookup(r._h, sc._h, refs.data_ptr(), None, records.data_ptr(), n, stream) == drt.OK, drt._lib.drt_last_error()

        def weights():
            assert drt._lib.drt_renderer_surface_weights(r._h, sc._h, table.data_ptr(), stream) == drt.OK, drt._lib.drt_last_error()

        def sample():
            assert drt._lib.drt_renderer_sample_surface(r._h, sc._h, 7, 0, samples.data_ptr(), n, stream) == drt.OK, drt._lib.drt_last_error()

        row = {"scene": name, "triangles": len(s.v0), "textures": len(s.texs), "refs": n,
               "hit": round(float((hits.view(torch.int32)[:, 1] >= 0).double().mean().item()), 4)}
        m = min(args.count, n)
        checks = {}
        for key, fn in (("lookup_coherent", lambda: lookup(hits)), ("lookup_random", lambda: lookup(shuffled)), ("copy", lambda: dst.copy_(src)),
                        ("trace_rays", trace), ("weights", weights), ("sample", sample)):
            ms, t_lo, t_hi = timed(fn, args.reps, args.warmup, args.calls)
            row[key] = {"ms": round(ms, 4), "ms_min": round(t_lo, 4), "ms_max": round(t_hi, 4)}
            torch.cuda.synchronize()
            if key.startswith("lookup"):
                ref = (hits if key == "lookup_coherent" else shuffled)[:m].cpu().numpy()
                checks[key] = sr.same(records[:m].cpu().numpy(), sr.lookup(s, ref.view(np.int32)[:, 1], ref[:, 2], ref[:, 3]))
            elif key == "weights":
                cdf = sr.weights(s)
                checks[key] = [int(x) for x in table.cpu().numpy()] == cdf
            elif key == "sample":
                checks[key] = samples[:m].cpu().numpy().tobytes() == sr.sample(s, 7, 0, m, cdf).tobytes()
        for key in ("lookup_coherent", "lookup_random"):
            row[key]["ratio_to_copy"] = round(row[key]["ms"] / row["copy"]["ms"], 3)
            row[key]["ratio_to_trace_rays"] = round(row[key]["ms"] / row["trace_rays"]["ms"], 3)
            row[key]["gb_per_s"] = round(n * 112 / row[key]["ms"] / 1e6, 1)
        row["copy"]["gb_per_s"] = round(n * 112 / row["copy"]["ms"] / 1e6, 1)
        row["draw_ms"] = round(row["sample"]["ms"] - row["weights"]["ms"], 4)
        row["bit_equal_to_restatement"] = checks
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
