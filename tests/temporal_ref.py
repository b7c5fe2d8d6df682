"""Restatement of drt_renderer_temporal_denoise (include/drt.h) in float32 numpy, for the tests.  No tests of its own.

Stage (b), reproject(): reprojection through the first-hit geometry, accumulation of colour and luminance moments, the temporal or
7x7 spatial variance -- every operation in the order the header fixes, one float32 rounding each, so that the GPU result can be
compared bit for bit.  Stage (c), atrous_var(): the a-trous filter of tests/denoise_ref.py with the luminance term divided by
the prefiltered variance and the variance filtered alongside.  The guides come from denoise_ref.guides() on the CPU or from
Renderer.renderGuides on the GPU (the same bits: test_gpu_denoise.py); the camera's host constants use libm's tanf, as the
library's host code does.
"""
import collections
import ctypes as C
import ctypes.util

import numpy as np

from tests.denoise_ref import B3, _sq

F = np.float32
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.tanf.restype = C.c_float
_libm.tanf.argtypes = [C.c_float]

DEFAULTS = dict(iterations=5, max_history=32, alpha_min=0.0, normal_cos_min=0.9, sigma_luma=4.0, sigma_normal=0.1, sigma_albedo=0.1)
History = collections.namedtuple("History", "color length normal prim m1 m2 variance weight pinhole")
Pinhole = collections.namedtuple("Pinhole", "pos forward right up focus plane_w plane_h")


def _dot3(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(F)


def _normalize(v):
    v = np.asarray(v, F)
    inv = (F(1) / np.sqrt(_dot3(v, v))).astype(F)
    return (v * inv[..., None]).astype(F)


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)


def pinhole(position, forward, W, H, vfov_rad=1.0471975511965976, focus_dist=10.0):
    """The camera constants of Camera.cu:82 the reprojection uses (the tan(vfov / 4) quirk included)."""
    fov_factor = F(_libm.tanf(F(F(vfov_rad) / F(2)) / F(2)))
    focus = F(focus_dist)
    plane_h = F(F(2) * fov_factor) * focus
    plane_w = plane_h * (F(W) / F(H))
    f = _normalize(np.asarray(forward, F))
    right = _normalize(_cross(f, np.array([0, 1, 0], F)))
    up = _cross(right, f)
    return Pinhole(np.asarray(position, F), f, right, up, focus, F(plane_w), F(plane_h))


def primary_directions(ph, W, H):
    """d0 [H, W, 3]: normalize(fwd_focus + u * horizontal + v * vertical), uv of RayGen.cuh:65-66, no jitter, no defocus."""
    y, x = np.mgrid[0:H, 0:W]
    u = ((x.astype(F) / F(W)) * F(2) - F(1)).astype(F)
    v = ((y.astype(F) / F(H)) * F(2) - F(1)).astype(F)
    fwd_focus = (ph.forward * ph.focus).astype(F)
    horizontal, vertical = (ph.plane_w * ph.right).astype(F), (ph.plane_h * ph.up).astype(F)
    d = (fwd_focus + u[..., None] * horizontal).astype(F) + (v[..., None] * vertical).astype(F)
    return _normalize(d.astype(F))


def project(ph, P, W, H):
    """World points P [..., 3] into the pinhole `ph`: (fx, fy, ok) with ok = z > 0 and -1 < fx < W, -1 < fy < H."""
    with np.errstate(all="ignore"):
        pv = (np.asarray(P, F) - ph.pos).astype(F)
        z = _dot3(pv, ph.forward)
        su = ((_dot3(pv, ph.right) * ph.focus) / (z * ph.plane_w)).astype(F)
        sv = ((_dot3(pv, ph.up) * ph.focus) / (z * ph.plane_h)).astype(F)
        fx = (((su + F(1)) * F(0.5)) * F(W)).astype(F)
        fy = (((sv + F(1)) * F(0.5)) * F(H)).astype(F)
        ok = (z > 0) & (fx > F(-1)) & (fx < F(W)) & (fy > F(-1)) & (fy < F(H))
    return fx, fy, ok


def luminance(c, T=F):
    return ((T(0.2126) * c[..., 0] + T(0.7152) * c[..., 1]) + T(0.0722) * c[..., 2]).astype(T)


def reproject(prev, rgba, guides, ph, max_history=32, alpha_min=0.0, normal_cos_min=0.9, **_):
    """Stage (b): the History after one call.  prev = the History of the previous call or None; rgba = the framebuffer [H, W, 4];
    guides = Guides(albedo, normal, t, prim) of frame 1 for this call's camera; ph = pinhole() of this call's camera."""
    c = np.ascontiguousarray(rgba, F)[..., :3]
    H, W = c.shape[:2]
    prim, normal, t = np.asarray(guides.prim, np.int32), np.asarray(guides.normal, F), np.asarray(guides.t, F)
    l = luminance(c)
    S = np.zeros((H, W), F)
    hN, h1, h2, hc = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W, 3), F)
    if prev is not None:
        d0 = primary_directions(ph, W, H)
        with np.errstate(all="ignore"):
            P = (ph.pos + d0 * t[..., None]).astype(F)
        fx, fy, ok = project(prev.pinhole, P, W, H)
        ok &= prim >= 0
        fx, fy = np.where(ok, fx, F(0)), np.where(ok, fy, F(0))
        flx, fly = np.floor(fx), np.floor(fy)
        ix, iy = flx.astype(np.int64), fly.astype(np.int64)
        wx = [None, (fx - flx).astype(F)]
        wy = [None, (fy - fly).astype(F)]
        wx[0], wy[0] = (F(1) - wx[1]).astype(F), (F(1) - wy[1]).astype(F)
        for j in range(2):
            for i in range(2):
                qx, qy = ix + i, iy + j
                valid = ok & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                valid &= prev.length[cy, cx] >= 1
                valid &= prev.prim[cy, cx] == prim
                valid &= _dot3(prev.normal[cy, cx], normal) >= F(normal_cos_min)
                w = np.where(valid, (wx[i] * wy[j]).astype(F), F(0))
                # (an invalid tap adds nothing: x + 0 = x exactly for the sums below, which never hold -0)
                S = (S + w).astype(F)
                hc = (hc + prev.color[cy, cx] * w[..., None]).astype(F)
                hN = (hN + prev.length[cy, cx] * w).astype(F)
                h1 = (h1 + prev.m1[cy, cx] * w).astype(F)
                h2 = (h2 + prev.m2[cy, cx] * w).astype(F)
    has = S >= F(0.01)
    Ss = np.where(has, S, F(1))
    N = np.where(has, np.minimum(np.floor((hN / Ss).astype(F) + F(0.5)) + F(1), F(max_history)), F(1)).astype(F)
    a = np.maximum((F(1) / N).astype(F), F(alpha_min)).astype(F)
    om = (F(1) - a).astype(F)
    color = np.where(has[..., None], ((hc / Ss[..., None]).astype(F) * om[..., None]).astype(F) + (c * a[..., None]).astype(F), c).astype(F)
    l2 = (l * l).astype(F)
    m1 = np.where(has, ((h1 / Ss).astype(F) * om).astype(F) + (l * a).astype(F), l).astype(F)
    m2 = np.where(has, ((h2 / Ss).astype(F) * om).astype(F) + (l2 * a).astype(F), l2).astype(F)
    var_t = np.maximum(F(0), (m2 - (m1 * m1).astype(F)).astype(F)).astype(F)
    # the spatial estimate: 7x7, clamped, same prim, dy outer, dx inner
    lc = luminance(color)
    s1, s2, n = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F)
    ys, xs = np.arange(H), np.arange(W)
    for dy in range(-3, 4):
        qy = np.clip(ys + dy, 0, H - 1)
        for dx in range(-3, 4):
            qx = np.clip(xs + dx, 0, W - 1)
            same = prim[qy][:, qx] == prim
            lq = lc[qy][:, qx]
            s1 = np.where(same, (s1 + lq).astype(F), s1)
            s2 = np.where(same, (s2 + (lq * lq).astype(F)).astype(F), s2)
            n = np.where(same, n + F(1), n).astype(F)
    e1, e2 = (s1 / n).astype(F), (s2 / n).astype(F)
    var_s = (np.maximum(F(0), (e2 - (e1 * e1).astype(F)).astype(F)) * (F(4) / N).astype(F)).astype(F)
    variance = np.where(N >= F(4), var_t, var_s).astype(F)
    return History(color, N, normal.copy(), prim.copy(), m1, m2, variance, S, ph)


def atrous_var_passes(color, variance, albedo, normal, iterations=5, sigma_luma=4.0, sigma_normal=0.1, sigma_albedo=0.1, dtype=F, **_):
    """Stage (c), pass by pass (a generator): the colour [H, W, 3] after passes 1, 2, ... K.  dtype = float32: the kernel's own
    operations and order, one float32 rounding each.  dtype = float64: the same formulas of drt.h with every array and constant in
    float64 and np.exp in float64 -- the filter evaluated (to float32's eyes) exactly."""
    T = dtype
    c, var = np.ascontiguousarray(color, T).copy(), np.ascontiguousarray(variance, T).copy()
    alb, nrm = np.ascontiguousarray(albedo, T), np.ascontiguousarray(normal, T)
    H, W = var.shape
    # (the sigmas are the float parameters of drt_temporal_params in either dtype)
    k_normal = T(1) / (T(F(sigma_normal)) * T(F(sigma_normal)))
    k_albedo = T(1) / (T(F(sigma_albedo)) * T(F(sigma_albedo)))
    ys, xs = np.arange(H), np.arange(W)
    g3 = np.array([0.25, 0.5, 0.25], T)
    for i in range(iterations):
        s = 1 << i
        gv = np.zeros((H, W), T)
        for dy in range(-1, 2):
            qy = np.clip(ys + dy, 0, H - 1)
            for dx in range(-1, 2):
                qx = np.clip(xs + dx, 0, W - 1)
                gv = (gv + (g3[dy + 1] * g3[dx + 1]) * var[qy][:, qx]).astype(T)
        r = (T(1) / ((T(F(sigma_luma)) * np.sqrt(gv)).astype(T) + T(1e-4)).astype(T)).astype(T)
        lum = luminance(c, T)
        wsum, vsum, csum = np.zeros((H, W), T), np.zeros((H, W), T), np.zeros((H, W, 3), T)
        for b in range(5):
            qy = np.clip(ys + (b - 2) * s, 0, H - 1)
            for a in range(5):
                qx = np.clip(xs + (a - 2) * s, 0, W - 1)
                cq, nq, aq = c[qy][:, qx], nrm[qy][:, qx], alb[qy][:, qx]
                e = ((np.abs(lum - lum[qy][:, qx]) * r).astype(T) + _sq(nrm - nq) * k_normal).astype(T) + (_sq(alb - aq) * k_albedo).astype(T)
                w = ((T(B3[a]) * T(B3[b])) * np.exp(-e).astype(T)).astype(T)
                wsum = (wsum + w).astype(T)
                csum = (csum + cq * w[..., None]).astype(T)
                vsum = (vsum + (w * w).astype(T) * var[qy][:, qx]).astype(T)
        c = (csum / wsum[..., None]).astype(T)
        var = (vsum / (wsum * wsum).astype(T)).astype(T)
        yield c


def atrous_var(color, variance, albedo, normal, iterations=5, sigma_luma=4.0, sigma_normal=0.1, sigma_albedo=0.1, dtype=F, **_):
    """Stage (c): (c_K, 1) [H, W, 4] from the integrated colour [H, W, 3] and its variance [H, W], in `dtype` (atrous_var_passes)."""
    c = np.ascontiguousarray(color, dtype)
    for c in atrous_var_passes(color, variance, albedo, normal, iterations, sigma_luma, sigma_normal, sigma_albedo, dtype):
        pass
    return np.concatenate([c, np.ones(c.shape[:2] + (1,), dtype)], axis=-1)


def temporal_denoise(prev, rgba, guides, ph, **params):
    """One call: (History, filtered [H, W, 4])."""
    p = dict(DEFAULTS, **params)
    hist = reproject(prev, rgba, guides, ph, **p)
    return hist, atrous_var(hist.color, hist.variance, guides.albedo, guides.normal, **p)


def rmse(a, b):
    d = np.asarray(a, np.float64)[..., :3] - np.asarray(b, np.float64)[..., :3]
    return float(np.sqrt((d * d).mean()))


def pinhole_of(cam, W, H):
    """pinhole() of a camera object with m_Position, m_Forward_dir, vfov_rad and focus_dist (dustraytracer_amd.Camera)."""
    return pinhole(np.asarray(cam.m_Position, F), np.asarray(cam.m_Forward_dir, F), W, H, cam.vfov_rad, cam.focus_dist)


def two_quads():
    """A 2 x 2 foreground quad at z = 2 in front of an 8 x 6 background quad at z = 0, both facing +z, two flat materials:
    (pos, nrm, uv, mat, materials, textures) for ray_query_ref.programmatic_scene.  Triangles 0, 1 = background, 2, 3 = foreground
    in load order."""
    def quad(hx, hy, z):
        a, b, c, d = (-hx, -hy, z), (hx, -hy, z), (hx, hy, z), (-hx, hy, z)
        return [[a, b, c], [a, c, d]]
    pos = np.array(quad(4.0, 3.0, 0.0) + quad(1.0, 1.0, 2.0), F)
    nrm = np.tile(F([0, 0, 1]), (4, 3, 1))
    uv = np.zeros((4, 3, 2), F)
    mat = np.array([0, 0, 1, 1], np.int32)
    return pos, nrm, uv, mat, [((0.8, 0.7, 0.3), -1), ((0.2, 0.4, 0.9), -1)], []
