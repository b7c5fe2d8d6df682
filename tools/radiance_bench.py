"""Throughput of the radiance query (Renderer.radiance / cameraRays / renderViews, kernel_radiance.hip) next to path_pool, the
renderer's own kernel, on the same configuration in the same process.  One JSON line per scene and form:
  camera      1920x1080 primary rays of frame 1 (cameraRays), bounce limit of the scene's BASELINE config:
              radiance_ms (the radiance launch alone), frame_ms (cameraRays + radiance), msamples_s = pixels / radiance_ms,
              path_pool_ms / path_pool_msamples_s = one RenderBatch frame at 1080p (its device time), ratio = radiance / path_pool rate
  multiview   8 cameras at 480x270, 4 spp: renderViews (8 x camera_rays + 4 radiance launches over 8 views) vs 8 sequential
              single-renderer RenderBatch calls (resize, reset, 4 frames each), wall time around each with a device synchronise
  incoherent  1920*1080 rays from random points on random triangles in random directions (ray_query_ref.surface_rays)
Times: device events (torch.cuda.Event) on the current stream, median of --reps after --warmup.

  python tools/radiance_bench.py [--scenes a,b] [--reps 20] [--warmup 3] [--out profiles/r07_radiance_bench.jsonl]
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
import oracle  # noqa: E402
from tests import ray_query_ref as rq  # noqa: E402
from tests.scenes import SCENES, scene_path  # noqa: E402

DEFAULT = "cornell_box,suzanne_plane,dense_monkey,room,cs16_dust"
W, H = 1920, 1080


def event_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def wall_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def camera(name, i=0):
    _, pos, fwd, _ = SCENES[name]
    c = drt.Camera((pos[0] + 0.05 * i, pos[1], pos[2] - 0.05 * i))
    c.m_Forward_dir = np.array((fwd[0] + 0.02 * i, fwd[1], fwd[2]), np.float32)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=DEFAULT)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_radiance_bench.jsonl"))
    args = ap.parse_args()
    lines = []
    for name in args.scenes.split(","):
        depth = SCENES[name][3]
        sc = drt.Scene()
        sc.loadGLTFmodel(scene_path(name))
        b = drt.BVHBuilder()
        b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
        b.buildIterative(sc)
        r = drt.Renderer(0)
        r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=depth)
        cam = camera(name)
        # ---- camera rays at 1080p vs path_pool on the same frame
        rays = r.cameraRays(cam, W, H, 1, as_torch=True)
        out = torch.empty(tuple(rays.shape[:-1]) + (4,), dtype=torch.float32, device=rays.device)
        rad_ms = event_ms(lambda: r.radiance(sc, rays, out=out), args.reps, args.warmup)
        frame_ms = event_ms(lambda: r.radiance(sc, r.cameraRays(cam, W, H, 1, as_torch=True), out=out), args.reps, args.warmup)
        pp = drt.Renderer(0)
        pp.m_RendererSettings = r.m_RendererSettings
        pp.ResizeBuffer(W, H)
        for _ in range(args.warmup):
            pp.RenderBatch(cam, sc, 1)
        pp_ms = []
        for _ in range(args.reps):
            pp.resetAccumulationBuffer()
            pp_ms.append(pp.RenderBatch(cam, sc, 1))
        pp_ms = float(np.median(pp_ms))
        px = W * H
        line = {"scene": name, "form": "camera", "width": W, "height": H, "depth": depth, "radiance_ms": round(rad_ms, 3),
                "frame_ms": round(frame_ms, 3), "msamples_s": round(px / rad_ms / 1e3, 1), "path_pool_ms": round(pp_ms, 3),
                "path_pool_msamples_s": round(px / pp_ms / 1e3, 1), "ratio_vs_path_pool": round(pp_ms / rad_ms, 3),
                "path_pool_kernel": pp.kernelInfo()}
        lines.append(line)
        print(json.dumps(line), flush=True)
        # ---- multi-view: 8 cameras at 480x270, 4 spp
        cams = [camera(name, i) for i in range(8)]
        vw, vh, spp = 480, 270, 4
        views_ms = wall_ms(lambda: r.renderViews(cams, sc, vw, vh, spp, as_torch=True), max(5, args.reps // 4), 1)
        seq = drt.Renderer(0)
        seq.m_RendererSettings = r.m_RendererSettings

        def sequential():
            for c in cams:
                seq.ResizeBuffer(vw, vh)
                seq.resetAccumulationBuffer()
                seq.RenderBatch(c, sc, spp)
        seq_ms = wall_ms(sequential, max(5, args.reps // 4), 1)
        line = {"scene": name, "form": "multiview", "views": 8, "width": vw, "height": vh, "spp": spp, "depth": depth,
                "render_views_ms": round(views_ms, 3), "sequential_renders_ms": round(seq_ms, 3),
                "msamples_s": round(8 * vw * vh * spp / views_ms / 1e3, 1), "sequential_msamples_s": round(8 * vw * vh * spp / seq_ms / 1e3, 1)}
        lines.append(line)
        print(json.dumps(line), flush=True)
        # ---- incoherent rays from surfaces
        osc = oracle.Scene.load_glb(scene_path(name))
        rng = np.random.default_rng(1)
        org, dirs = rq.surface_rays(osc, px, rng)
        seeds = rng.integers(0, 2 ** 32, px, dtype=np.uint64).astype(np.uint32)
        packed = np.concatenate([org, seeds.view(np.float32)[:, None], dirs, np.ones((px, 1), np.float32)], axis=1)
        inc = torch.from_numpy(packed).to(rays.device)
        out1 = torch.empty((px, 4), dtype=torch.float32, device=rays.device)
        inc_ms = event_ms(lambda: r.radiance(sc, inc, out=out1), args.reps, args.warmup)
        line = {"scene": name, "form": "incoherent", "rays": px, "depth": depth, "radiance_ms": round(inc_ms, 3),
                "msamples_s": round(px / inc_ms / 1e3, 1)}
        lines.append(line)
        print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
