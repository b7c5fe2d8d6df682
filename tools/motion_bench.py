"""Device time of a temporal call with motion tracking (Renderer.trackMotion, kernel_motion.hip), of the refit's snapshot copy and
of the motion-vector pass, in one process.  One JSON line per scene x size:
  call_ms[variant]   TemporalDenoise(iterations=0)'s own device time (guide pass + reprojection + variance + copy) after a device
                     refit, with a history longer than 3 in place.  Variants: "off" (tracking off: the kernels of kernel_temporal.hip),
                     "none" (tracking on, the refit moved nothing: the snapshot is armed and equal), "some" (--fraction of the
                     triangles moved), "all" (every triangle moved).  A library without drt_renderer_track_motion (an older build
                     given with --package-root) runs "off" alone and reports it as "parent".
  extra_ms[variant]  call_ms[variant] - call_ms["off"]
  refit_ms[variant]  drt_renderer_refit's device time in that variant ("off": no snapshot copy; the others copy 48 B per triangle
                     first), snapshot_ms = refit_ms["some"] - refit_ms["off"]
  guide_ms, vectors_ms   device events around one guide pass and around motionVectors (which runs one guide pass first)
Medians of --reps after --warmup, the variants alternating inside every repetition; --label names the run.
call_ms contains the guide pass, which traces the refitted tree, and the variants refit to different positions ("off" and "some"
alternate between the rest pose and the moved one, "all" between rest and all moved, "none" stays where the last variant left
it): a difference between two variants mixes the tracing of another geometry with the reprojection's code path.  For the
kernels by themselves run one variant per process under a kernel trace (rocprofv3 --kernel-trace --stats -- python
tools/motion_bench.py --variants some ...): temporal_reproject_kernel, motion_reproject_kernel and motion_vectors_kernel then
have their own lines, and guide_kernel's shows what the geometry costs.

  python tools/motion_bench.py [--scenes a,b] [--sizes 1920x1080,3840x2160] [--fraction 0.05] [--reps 10] [--warmup 3]
                               [--variants off,none,some,all] [--label text] [--package-root dir] [--out file.jsonl]
--variants off makes a run comparable with an older build's; extra_ms and snapshot_ms need "off" among the variants.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell_box,suzanne_plane,dense_monkey,cs16_dust,room")
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--fraction", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--variants", default="off,none,some,all")
    ap.add_argument("--label", default="")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    if ROOT not in sys.path:
        sys.path.append(ROOT)                    # (tests.scenes)

    import torch

    import dustraytracer_amd as drt
    from tests.scenes import SCENES, scene_path

    dev = torch.device("cuda", 0)
    tracks = hasattr(drt.Renderer, "trackMotion")
    variants = args.variants.split(",") if tracks else ["off"]
    out = open(args.out, "a") if args.out else None
    for name in args.scenes.split(","):
        _, pos, fwd, depth = SCENES[name]
        sc = drt.Scene()
        sc.loadGLTFmodel(scene_path(name))
        pos0 = np.ascontiguousarray(sc.m_PrimitivesBuffer["vertex"]["position"], np.float32).copy()      # load order: before the build
        b = drt.BVHBuilder()
        b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
        b.buildIterative(sc)
        n = len(pos0)
        rng = np.random.default_rng(5)
        some = rng.permutation(n)[:max(1, int(round(args.fraction * n)))]
        shift = np.float32([0.01, 0.005, 0.0])

        def moved(sel):
            p = pos0.copy()
            p[sel] += shift
            return torch.from_numpy(p).to(dev)
        rest = torch.from_numpy(pos0).to(dev)
        targets = {"none": rest, "some": moved(some), "all": moved(np.arange(n))}
        targets["off"] = targets["some"]
        cam = drt.Camera(pos)
        cam.m_Forward_dir = np.array(fwd, np.float32)
        for size in args.sizes.split(","):
            W, H = (int(v) for v in size.split("x"))
            r = drt.Renderer(0)
            r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=depth)
            r.ResizeBuffer(W, H)
            r.Render(cam, sc)

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1)

            def call(v):
                """One refit + TemporalDenoise in variant v: (refit ms, call ms).  The geometry alternates between the rest pose
                and the variant's target, so that every call of "off" / "some" / "all" finds moved triangles."""
                if tracks:
                    r.trackMotion(v != "off")
                if v == "none":
                    target = cur[0]
                else:
                    target = targets[v] if cur[0] is not targets[v] and (v == "all" or cur[0] is rest) else rest
                ms_refit = r.refit(sc, target)
                cur[0] = target
                r.TemporalDenoise(cam, sc, iterations=0)
                return ms_refit, r.m_LastTemporalMs

            cur = [rest]
            for _ in range(4):                   # (a history longer than 3 before anything is timed)
                call("off")
            samples = {v: ([], []) for v in variants}
            extra = {"guide": [], "vectors": []}
            for i in range(args.warmup + args.reps):
                for v in variants:
                    a, c = call(v)
                    if i >= args.warmup:
                        samples[v][0].append(a)
                        samples[v][1].append(c)
                g = timed(lambda: r.renderGuides(cam, sc, 1, as_torch=True))
                if tracks:
                    r.trackMotion(True)
                    r.refit(sc, rest)
                    r.advanceMotion()
                    r.refit(sc, targets["some"])
                    cur[0] = targets["some"]
                    m = timed(lambda: r.motionVectors(cam, sc, as_torch=True))
                    r.advanceMotion()
                if i >= args.warmup:
                    extra["guide"].append(g)
                    if tracks:
                        extra["vectors"].append(m)
            rec = dict(scene=name, width=W, height=H, triangles=n, moved=len(some), device=torch.cuda.get_device_name(dev), reps=args.reps,
                       label=args.label or ("tree" if tracks else "parent"))
            key = (lambda v: v) if tracks else (lambda v: "parent")
            rec["refit_ms"] = {key(v): float(np.median(samples[v][0])) for v in variants}
            rec["call_ms"] = {key(v): float(np.median(samples[v][1])) for v in variants}
            rec["guide_ms"] = float(np.median(extra["guide"]))
            if tracks:
                if "off" in variants:
                    rec["extra_ms"] = {v: rec["call_ms"][v] - rec["call_ms"]["off"] for v in variants}
                if "some" in variants and "off" in variants:
                    rec["snapshot_ms"] = rec["refit_ms"]["some"] - rec["refit_ms"]["off"]
                rec["vectors_ms"] = float(np.median(extra["vectors"]))
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del r
    if out:
        out.close()


if __name__ == "__main__":
    main()
