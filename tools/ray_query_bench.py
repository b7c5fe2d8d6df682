"""Throughput of the batched ray queries (Renderer.traceRays / occluded, kernel_ray_query.hip).  One JSON line per
scene x ray set x query (x refill threshold):
  coherent    1920x1080 frame-1 camera rays
  incoherent  2 M rays from the primary hit points in seeded random hemisphere directions (about the face normal, turned
              towards the camera)
  short       the same rays with tmax at 1 % of the scene's diagonal
ms = device events around one query, median of --reps after --warmup; Mrays/s = rays / ms / 1000.  For context each scene also
gets one line with the renderer's own traced rays per second (counters.rays of a counting run over the kernel time of a plain
run, same frame and path depth).

  python tools/ray_query_bench.py [--scenes a,b] [--refill 16,64] [--reps 20] [--warmup 3] [--out file.jsonl]
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
from tests.scenes import SCENES, scene_path  # noqa: E402

W, H, N_INCOHERENT = 1920, 1080, 2 * 1024 * 1024


def camera_rays(cam, dev):
    """Frame-1 camera rays, computed on the host with the renderer's own camera KAT entry (drt_debug_kat which=4)."""
    y, x = np.mgrid[0:H, 0:W]
    x, y = x.ravel().astype(np.uint32), y.ravel().astype(np.uint32)
    inp = np.zeros((len(x), 3), np.uint32)
    inp[:, 0] = ((x.astype(np.float32) / np.float32(W)) * np.float32(2) - np.float32(1)).view(np.uint32)
    inp[:, 1] = ((y.astype(np.float32) / np.float32(H)) * np.float32(2) - np.float32(1)).view(np.uint32)
    inp[:, 2] = x + y * np.uint32(W)
    out = drt.debug_kat(4, inp, cam=cam, width=W, height=H)         # orig3, dir3, seed as uint32 words
    f = np.ascontiguousarray(out[:, :6]).view(np.float32)
    return torch.from_numpy(np.ascontiguousarray(f[:, :3])).to(dev), torch.from_numpy(np.ascontiguousarray(f[:, 3:6])).to(dev)


def timed(fn, reps, warmup):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell_box,suzanne_plane,dense_monkey,cs16_dust,room")
    ap.add_argument("--refill", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-render", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    refills = [int(v) for v in args.refill.split(",") if v] or [None]
    out = open(args.out, "a") if args.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for name in args.scenes.split(","):
        _, pos, fwd, depth = SCENES[name]
        sc = drt.Scene()
        sc.loadGLTFmodel(scene_path(name))
        b = drt.BVHBuilder()
        b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
        b.buildIterative(sc)
        cam = drt.Camera(pos)
        cam.m_Forward_dir = np.array(fwd, np.float32)
        r0 = drt.Renderer(0)
        org, dirs = camera_rays(cam, dev)
        hits = r0.traceRays(sc, org, dirs)
        hit = hits.prim >= 0
        # incoherent: hemisphere about the face normal turned against the primary ray
        tris = sc.m_PrimitivesBuffer
        fn = torch.from_numpy(np.ascontiguousarray(tris["face_normal"], np.float32)).to(dev)
        idx = torch.nonzero(hit).squeeze(1)
        g = torch.Generator(device=dev)
        g.manual_seed(1234)
        pick = idx[torch.randint(0, len(idx), (N_INCOHERENT,), device=dev, generator=g)]
        p = org[pick] + dirs[pick] * hits.t[pick].unsqueeze(1)
        nrm = fn[hits.prim[pick].long()]
        nrm = torch.where(((nrm * dirs[pick]).sum(1, keepdim=True) > 0), -nrm, nrm)
        v = torch.randn((N_INCOHERENT, 3), device=dev, generator=g)
        v = torch.where(((v * nrm).sum(1, keepdim=True) < 0), -v, v)
        inc_org = (p + nrm * 1e-3).contiguous()
        inc_dir = v.contiguous()
        allp = tris["vertex"]["position"].reshape(-1, 3)
        diag = float(np.linalg.norm(allp.max(0) - allp.min(0)))
        sets = {"coherent": (org, dirs, None), "incoherent": (inc_org, inc_dir, None), "short": (inc_org, inc_dir, 0.01 * diag)}
        for refill in refills:
            if refill is not None:
                os.environ["DRT_RQ_REFILL"] = str(refill)
            r = drt.Renderer(0)
            for set_name, (o, d, tmax) in sets.items():
                for q in ("closest", "occluded"):
                    if set_name == "short" and q == "closest":
                        f = lambda: r.traceRays(sc, o, d, 0.0, tmax)          # noqa: E731
                    elif q == "closest":
                        f = lambda: r.traceRays(sc, o, d)                     # noqa: E731
                    else:
                        f = (lambda: r.occluded(sc, o, d, 0.0, tmax)) if tmax is not None else (lambda: r.occluded(sc, o, d))   # noqa: E731
                    ms = timed(f, args.reps, args.warmup)
                    n = o.shape[0]
                    emit({"scene": name, "rays_set": set_name, "query": q, "refill_min": refill, "rays": n, "ms": round(ms, 4),
                          "mrays_per_s": round(n / ms / 1000.0, 1), "bvh_depth": sc.bvh_depth})
            del r
        if not args.no_render:
            rr = drt.Renderer(0)
            rr.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=depth, max_samples=100)
            rr.ResizeBuffer(W, H)
            rr.RenderBatch(cam, sc, 1)
            rr.resetAccumulationBuffer()
            ms = rr.RenderBatch(cam, sc, 2) / 2
            rc = drt.Renderer(0)
            rc.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=depth, max_samples=100)
            rc.ResizeBuffer(W, H)
            rc.setCounting(True)
            rc.RenderBatch(cam, sc, 1)
            rays = int(rc.getCounters().rays + rc.getCounters().shadow_rays)
            emit({"scene": name, "rays_set": "renderer", "query": "render", "kernel": rr.kernelInfo(), "rays": rays, "ms": round(ms, 4),
                  "mrays_per_s": round(rays / ms / 1000.0, 1), "bounce_limit": depth})


if __name__ == "__main__":
    main()
