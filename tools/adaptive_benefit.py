"""Scores the adaptive-sampling rule of include/drt.h on the CPU oracle (no GPU): MSE against a many-sample image of K adaptive
calls that spend S samples in all, versus the uniform renderer's S / pixels frames.  The rule is tests/adaptive_ref.py's
restatement; a pixel's k-th sample is the oracle's frame-k sample of that pixel (what drt_renderer_radiance returns for the
renderer's own primary rays), so the simulated state is the state the GPU call would hold.

    python tools/adaptive_benefit.py [--size 80 60] [--spp 4] [--calls 8] [--ref 512] [--scenes cornell_box uv_texture_test]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle  # noqa: E402
from tests import adaptive_ref as ar  # noqa: E402
from tests.scenes import SCENES, scene_path  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[80, 60])
    ap.add_argument("--spp", type=float, default=4.0)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--max-spp", type=int, default=64)
    ap.add_argument("--ref", type=int, default=512)
    ap.add_argument("--scenes", nargs="+", default=["cornell_box", "uv_texture_test"])
    a = ap.parse_args()
    W, H = a.size
    px = W * H
    budget = int(a.spp * px)
    for name in a.scenes:
        _, pos, fwd, depth = SCENES[name]
        osc = oracle.Scene.load_glb(scene_path(name)).build_bvh(20, 8)
        cam, st = oracle.default_camera(position=pos, forward=fwd), oracle.default_settings(ray_bounce_limit=depth, max_samples=1 << 30)
        cache = {}

        def sample(k):
            if k not in cache:
                cache[k] = oracle.render(osc, cam, st, W, H, k, 1)[1].reshape(-1, 3)
            return cache[k]

        ref = oracle.render(osc, cam, st, W, H, 1, a.ref)[0][..., :3].reshape(-1, 3).astype(np.float64)
        state, spent = ar.empty_state(px), 0
        for _ in range(a.calls):
            _, c = ar.plan(state, budget, max_spp=a.max_spp)
            state = ar.fold(state, c, sample)
            spent += int(c.sum())
        frames = max(1, round(spent / px))
        uniform = oracle.render(osc, cam, st, W, H, 1, frames)[0][..., :3].reshape(-1, 3).astype(np.float64)
        adaptive = ar.image(state)[:, :3].astype(np.float64)
        print(json.dumps(dict(scene=name, width=W, height=H, depth=depth, calls=a.calls, spp_per_call=a.spp, samples=spent,
                              samples_per_pixel=spent / px, uniform_frames=frames, n_min=int(state.n.min()), n_max=int(state.n.max()),
                              mse_adaptive=float(((adaptive - ref) ** 2).mean()), mse_uniform=float(((uniform - ref) ** 2).mean()),
                              reference_spp=a.ref)))


if __name__ == "__main__":
    main()
