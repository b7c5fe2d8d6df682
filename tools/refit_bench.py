"""Device time of the BVH refit (Renderer.refit, kernel_refit.hip) next to the host refit (Scene.refit) and the device rebuild
(drt_scene_build_bvh_device) of the same scene.  One JSON line per scene:
  refit_ms          device events around one Renderer.refit (positions already on the device), median of --reps after --warmup
  refit_ms_per_height   the same with DRT_REFIT_TOP=0: one launch per height up to the root (no single-workgroup top launch)
  host_refit_ms     wall time of one Scene.refit, median of 5
  rebuild_device_ms / rebuild_call_ms   drt_scene_build_bvh_device: its device time and the wall time of the call, median of 3
Scenes: the five BASELINE scenes and cs16_dust (editor BVH: leaf 20, bins 8), and 100 k / 1 M triangle soups (ray_query_ref.soup,
leaf 2, bins 8).

  python tools/refit_bench.py [--scenes a,b] [--reps 20] [--warmup 3] [--out file.jsonl]
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
from tests import ray_query_ref as rq  # noqa: E402
from tests.scenes import scene_path  # noqa: E402

DEFAULT = "cornell_box,suzanne_plane,dense_monkey,room,cs16_dust,soup100k,soup1m"


def make(name):
    """(scene factory, load-order positions [n, 3, 3], leaf, bins)."""
    if name.startswith("soup"):
        n = 100000 if name == "soup100k" else 1000000
        s = rq.soup(n, 1, spread=10.0 * (n / 90000) ** (1 / 3))

        def factory():
            sc = drt.Scene()
            for tex in s[5]:
                sc.addTexture(tex)
            for alb, tex in s[4]:
                sc.addMaterial(alb, tex)
            sc.setGeometry(*s[:4])
            return sc
        return factory, s[0], 2, 8

    def factory():
        sc = drt.Scene()
        sc.loadGLTFmodel(scene_path(name))
        return sc
    return factory, np.ascontiguousarray(factory().m_PrimitivesBuffer["vertex"]["position"], np.float32), 20, 8


def median_wall(fn, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def device_refit_ms(sc, pos_dev, reps, warmup, top):
    if top is not None:
        os.environ["DRT_REFIT_TOP"] = str(top)
    r = drt.Renderer(0)                          # (DRT_REFIT_TOP is read when the renderer is created)
    os.environ.pop("DRT_REFIT_TOP", None)
    for _ in range(warmup):
        r.refit(sc, pos_dev)
    return float(np.median([r.refit(sc, pos_dev) for _ in range(reps)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=DEFAULT)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = open(args.out, "a") if args.out else None
    for name in args.scenes.split(","):
        factory, pos, leaf, bins = make(name)
        sc = factory()
        b = drt.BVHBuilder()
        b.m_TargetLeafPrimitivesCount, b.m_BinCount = leaf, bins
        b.buildIterative(sc)
        rng = np.random.default_rng(1)
        moved = (pos + rng.normal(0, 1e-3, pos.shape)).astype(np.float32)
        pos_dev = torch.from_numpy(moved).to(dev)
        line = {"scene": name, "triangles": int(len(pos)), "nodes": int(len(sc.m_BVHNodes)), "bvh_depth": sc.bvh_depth,
                "refit_ms": round(device_refit_ms(sc, pos_dev, args.reps, args.warmup, None), 4),
                "refit_ms_per_height": round(device_refit_ms(sc, pos_dev, args.reps, args.warmup, 0), 4),
                "host_refit_ms": round(median_wall(lambda: sc.refit(moved), 5), 3)}
        ms = []

        def rebuild():
            s2 = factory()
            t0 = time.perf_counter()
            b2 = drt.BVHBuilder()
            b2.m_TargetLeafPrimitivesCount, b2.m_BinCount, b2.m_BuildDevice = leaf, bins, 0
            b2.buildIterative(s2)
            ms.append(((time.perf_counter() - t0) * 1e3, b2.m_LastBuildDeviceMs))
        for _ in range(4):
            rebuild()
        ms = ms[1:]                              # the first call loads the builder's code object
        line["rebuild_device_ms"] = round(float(np.median([m[1] for m in ms])), 3)
        line["rebuild_call_ms"] = round(float(np.median([m[0] for m in ms])), 3)
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()


if __name__ == "__main__":
    main()
