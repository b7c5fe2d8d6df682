"""Restatement of the guide buffers and the a-trous filter of include/drt.h (drt_renderer_render_guides / drt_renderer_denoise),
for the tests.  No tests of its own.

Guides of frame f come from the oracle: albedo = the accumulation of a one-frame ALBEDO debug render (tone mapping and gamma
off), normal = that of a NORMAL debug render on hit pixels and 0 elsewhere (a zeroed sum + the frame, RenderKernel.cu:29, is
what the views show), t and prim = ray_query_ref.closest on the frame's camera rays.  atrous() is the filter loop of drt.h in
float32 numpy, with the kernel's constants: k_color = 2^i * (1 / sigma_color^2), k_normal = 1 / sigma_normal^2, k_albedo =
1 / sigma_albedo^2.
"""
import collections

import numpy as np

import oracle
from tests import ray_query_ref as rq

Guides = collections.namedtuple("Guides", "albedo normal t prim")
B3 = np.float32([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
DEFAULTS = dict(iterations=5, sigma_color=0.5, sigma_normal=0.1, sigma_albedo=0.1)


def camera_rays(cam, W, H, frame=1):
    """The primary rays of frame `frame`, row-major from y = 0: uv ((float)x/W)*2-1, seed (x + y*W) * frame (RayGen.cuh:65-75)."""
    y, x = np.mgrid[0:H, 0:W]
    x, y = x.ravel().astype(np.uint32), y.ravel().astype(np.uint32)
    uv = np.stack([(x.astype(np.float32) / np.float32(W)) * np.float32(2) - np.float32(1),
                   (y.astype(np.float32) / np.float32(H)) * np.float32(2) - np.float32(1)], axis=1).astype(np.float32)
    seeds = ((x + y * np.uint32(W)).astype(np.uint64) * np.uint64(frame) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    r6, _ = oracle.kat_getray(cam, W, H, uv, seeds)
    return r6[:, :3].copy(), r6[:, 3:].copy()


def guides(osc, cam, W, H, frame=1, **settings):
    """Guides(albedo [H, W, 3], normal [H, W, 3], t [H, W], prim [H, W]) of frame `frame`; `settings` = the renderer's (sky)."""
    st = oracle.default_settings(**dict(settings, render_mode=1, debug_mode=0, tone_mapping=0, gamma_correction=0))
    _, albedo, _ = oracle.render(osc, cam, st, W, H, frame, 1)
    st = oracle.default_settings(**dict(settings, render_mode=1, debug_mode=1))
    _, normal, _ = oracle.render(osc, cam, st, W, H, frame, 1)
    org, dirs = camera_rays(cam, W, H, frame)
    hits = rq.closest(osc, org, dirs, np.float32(0), rq.FLT_MAX)
    prim, t = hits.prim.reshape(H, W), hits.t.reshape(H, W)
    normal = np.where((prim >= 0)[..., None], normal, np.float32(0)).astype(np.float32)
    return Guides(albedo, normal, t, prim)


def _sq(d):
    """|d|^2 summed over x, y, z in that order, float32."""
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def atrous_passes(rgba, albedo, normal, iterations=5, sigma_color=0.5, sigma_normal=0.1, sigma_albedo=0.1, dtype=np.float32):
    """The colour [H, W, 3] after each pass of the filter of drt_renderer_denoise in turn (a generator: c_1, c_2, ... c_K).  dtype =
    np.float32: the kernel's own operations and order, one float32 rounding each.  dtype = np.float64: the same formulas of drt.h
    with every array and constant in float64 and np.exp in float64 -- the filter evaluated (to float32's eyes) exactly."""
    f = dtype
    rgba = np.ascontiguousarray(rgba, f)
    alb, nrm = np.ascontiguousarray(albedo, f), np.ascontiguousarray(normal, f)
    H, W = rgba.shape[:2]
    c = rgba[..., :3].copy()
    # (the sigmas are the float parameters of drt_denoise_params in either dtype)
    inv_sc2 = f(1) / (f(np.float32(sigma_color)) * f(np.float32(sigma_color)))
    k_normal = f(1) / (f(np.float32(sigma_normal)) * f(np.float32(sigma_normal)))
    k_albedo = f(1) / (f(np.float32(sigma_albedo)) * f(np.float32(sigma_albedo)))
    ys, xs = np.arange(H), np.arange(W)
    for i in range(iterations):
        s = 1 << i
        k_color = f(s) * inv_sc2
        wsum = np.zeros((H, W), f)
        csum = np.zeros((H, W, 3), f)
        for b in range(5):
            qy = np.clip(ys + (b - 2) * s, 0, H - 1)
            for a in range(5):
                qx = np.clip(xs + (a - 2) * s, 0, W - 1)
                cq, nq, aq = c[qy][:, qx], nrm[qy][:, qx], alb[qy][:, qx]
                e = (_sq(c - cq) * k_color + _sq(nrm - nq) * k_normal) + _sq(alb - aq) * k_albedo
                w = (f(B3[a]) * f(B3[b])) * np.exp(-e).astype(f)
                wsum = wsum + w
                csum = csum + cq * w[..., None]
        c = (csum / wsum[..., None]).astype(f)
        yield c


def atrous(rgba, albedo, normal, iterations=5, sigma_color=0.5, sigma_normal=0.1, sigma_albedo=0.1, dtype=np.float32):
    """The filter of drt_renderer_denoise on rgba [H, W, 4] with guides albedo / normal [H, W, 3]: (c_K, the input's alpha), in
    `dtype` (atrous_passes)."""
    rgba = np.ascontiguousarray(rgba, dtype)
    c = rgba[..., :3]
    for c in atrous_passes(rgba, albedo, normal, iterations, sigma_color, sigma_normal, sigma_albedo, dtype):
        pass
    return np.concatenate([c, rgba[..., 3:4]], axis=-1)


def mse(a, b):
    d = np.asarray(a, np.float64)[..., :3] - np.asarray(b, np.float64)[..., :3]
    return float((d * d).mean())
