"""Restatement of the guide-driven upscaler of include/drt.h (drt_renderer_upscale), for the tests.  No tests of its own.

upscale() is the rule of drt.h operation by operation, vectorised over the output pixels: dtype = np.float32 gives the kernel's own
operations and order, one float32 rounding each (np.exp in float32 stands for expf); dtype = np.float64 evaluates the same
formulas on the same float32 inputs and parameters exactly, to float32's eyes.  Guides are Guides(albedo [H, W, 3], normal
[H, W, 3], t [H, W], prim [H, W] int32), row 0 = bottom -- what Renderer.renderGuides returns.
"""
import collections

import numpy as np

Guides = collections.namedtuple("Guides", "albedo normal t prim")
# upscale(details=True): the image, the stage map, and per tap in tap order (leading axis: 4 taps of stage 1, 16 of stage 2) the
# validity, the distance e, and for stage 1 the bilinear weight b and whether the tap was accepted
Details = collections.namedtuple("Details", "out stage valid1 e1 b1 accepted1 valid2 e2")
DEFAULTS = dict(demodulate=0, sigma_normal=0.1, sigma_depth=0.05, sigma_albedo=0.1, albedo_floor=0.01)
FLT_MAX = np.float32(3.4028234663852886e38)


def pack_guides(g):
    """Guides -> float32 [H, W, 8] as drt_guide lays a record out: albedo rgb, t, normal xyz, prim (int32 bits)."""
    H, W = g.t.shape
    out = np.zeros((H, W, 8), np.float32)
    out[..., 0:3], out[..., 3], out[..., 4:7] = g.albedo, g.t, g.normal
    out.view(np.int32)[..., 7] = g.prim
    return out


def _sq(d):
    """|d|^2 summed over x, y, z in that order."""
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def source_position(n_out, n_src, f):
    """Step 1 along one axis: (x0 as int, w0, w1) for every output coordinate."""
    fx = (np.arange(n_out).astype(f) * f(n_src)) / f(n_out)
    x0 = np.floor(fx)
    w1 = (fx - x0).astype(f)
    return x0.astype(np.int64), (f(1) - w1).astype(f), w1


def upscale(colour, lo, hi, demodulate=0, sigma_normal=0.1, sigma_depth=0.05, sigma_albedo=0.1, albedo_floor=0.01, dtype=np.float32,
            stages=False, details=False):
    """colour [H, W, 4] with guides `lo` [H, W] -> [Ho, Wo, 4] at the size of guides `hi`.  stages=True: (image, stage map
    [Ho, Wo] of 1 / 2 / 3) -- which of the rule's stages gave each pixel its value."""
    f = dtype
    c = np.ascontiguousarray(colour, np.float32)[..., :3].astype(f)
    H, W = c.shape[:2]
    Ho, Wo = hi.t.shape
    assert lo.t.shape == (H, W) and Wo >= W and Ho >= H
    alb_l, nrm_l, t_l = lo.albedo.astype(f), lo.normal.astype(f), lo.t.astype(f)
    alb_h, nrm_h, t_h = hi.albedo.astype(f), hi.normal.astype(f), hi.t.astype(f)
    miss_l, miss_h = lo.prim < 0, hi.prim < 0
    # (the parameters are the float fields of drt_upscale_params in either dtype)
    k_normal = f(1) / (f(np.float32(sigma_normal)) * f(np.float32(sigma_normal)))
    k_albedo = f(1) / (f(np.float32(sigma_albedo)) * f(np.float32(sigma_albedo)))
    floor = f(np.float32(albedo_floor))
    x0, wx0, wx1 = source_position(Wo, W, f)
    y0, wy0, wy1 = source_position(Ho, H, f)
    x0, y0 = np.broadcast_to(x0[None, :], (Ho, Wo)), np.broadcast_to(y0[:, None], (Ho, Wo))

    with np.errstate(all="ignore"):
        inv_dz = f(1) / (f(np.float32(sigma_depth)) * t_h)
        v_all = c / np.fmax(alb_l, floor) if demodulate else c

        def tap(qx, qy):
            """(valid, v, e) of the clamped tap (qx, qy) for every output pixel"""
            valid = miss_l[qy, qx] == miss_h
            dz = (t_l[qy, qx] - t_h) * inv_dz
            e = _sq(nrm_h - nrm_l[qy, qx]) * k_normal + dz * dz
            if not demodulate:
                e = e + _sq(alb_h - alb_l[qy, qx]) * k_albedo
            return valid, v_all[qy, qx], np.where(miss_h, f(0), e).astype(f)

        # stage 1
        S, A = np.zeros((Ho, Wo), f), np.zeros((Ho, Wo, 3), f)
        accepted_any = np.zeros((Ho, Wo), bool)
        log1, log2 = [], []
        for j in range(2):
            for i in range(2):
                b = ((wx1 if i else wx0)[None, :] * (wy1 if j else wy0)[:, None]).astype(f)
                valid, v, e = tap(np.minimum(x0 + i, W - 1), np.minimum(y0 + j, H - 1))
                acc = valid & (b > 0) & (e <= 16)
                w = (b * np.exp(-e).astype(f)).astype(f)
                S = np.where(acc, S + w, S)
                A = np.where(acc[..., None], A + v * w[..., None], A)
                accepted_any |= acc
                log1.append((valid, e, b, acc))
        o = (A / S[..., None]).astype(f)
        # stage 2
        best, have = np.zeros((Ho, Wo), f), np.zeros((Ho, Wo), bool)
        o2 = np.zeros((Ho, Wo, 3), f)
        for dy in range(-1, 3):
            for dx in range(-1, 3):
                valid, v, e = tap(np.clip(x0 + dx, 0, W - 1), np.clip(y0 + dy, 0, H - 1))
                take = valid & np.where(have, e < best, e == e)
                best = np.where(take, e, best)
                o2 = np.where(take[..., None], v, o2)
                have |= take
                log2.append((valid, e))
        # stage 3
        nx = np.minimum(x0 + (wx1 > f(0.5))[None, :], W - 1)
        ny = np.minimum(y0 + (wy1 > f(0.5))[:, None], H - 1)
        o3 = v_all[ny, nx]
        stage = np.where(accepted_any, 1, np.where(have, 2, 3))
        o = np.where((stage == 1)[..., None], o, np.where((stage == 2)[..., None], o2, o3))
        if demodulate:
            o = o * np.fmax(alb_h, floor)
    out = np.concatenate([o.astype(f), np.ones((Ho, Wo, 1), f)], axis=-1)
    if details:
        return Details(out, stage, *(np.stack(x) for x in zip(*log1)), *(np.stack(x) for x in zip(*log2)))
    return (out, stage) if stages else out


# ---- made-up inputs for the kernel tests ----
MADE_UP_SIZES = [(1, 1, 1, 1), (1, 1, 3, 2), (7, 3, 16, 9), (5, 4, 5, 4), (8, 8, 16, 16)]
# sigmas whose reciprocal squares are exact in float32 (4, 16, 4): with the palettes below every e is exact, so "e == 16" is
EXACT = dict(sigma_normal=0.5, sigma_depth=0.25, sigma_albedo=0.5, albedo_floor=0.01)
_NORMALS = np.float32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [-1.000001, 0, 0]])
_DEPTHS = np.float32([1, 2, 4])
_ALBEDOS = np.float32([[0.25, 0.5, 0.75], [0.75, 0.25, 0.5], [0.5, 0.5, 0.5], [0.0078125, 0.5, 1.0]])      # (one component under the floor; all exact in binary)


def made_up(W, H, Wo, Ho, seed=1):
    """(colour [H, W, 4], lo, hi): guides from small palettes (so that distances tie and hit 16 exactly), hits left of a vertical
    boundary and misses right of it, the boundary three output pixels further right at the output size (taps of the other class:
    stages 2 and 3), half of the output pixels copying the source pixel under them, a hit deep among misses and a miss deep among
    hits, NaNs in both sizes' guides, and where Wo == 2 W an output pixel exactly on a source pixel at e == 16 and one just above."""
    rng = np.random.default_rng(seed)

    def draw(h, w):
        return Guides(_ALBEDOS[rng.integers(0, len(_ALBEDOS), (h, w))].copy(), _NORMALS[rng.integers(0, 6, (h, w))].copy(),
                      _DEPTHS[rng.integers(0, len(_DEPTHS), (h, w))].copy(), rng.integers(0, 1000, (h, w)).astype(np.int32))

    def finish(g, hit):
        g.normal[~hit], g.t[~hit], g.prim[~hit] = 0, FLT_MAX, -1
        return g

    colour = np.concatenate([rng.random((H, W, 3), np.float32), np.ones((H, W, 1), np.float32)], axis=-1)
    lo, hi = draw(H, W), draw(Ho, Wo)
    x0 = (np.arange(Wo) * W) // Wo
    y0 = (np.arange(Ho) * H) // Ho
    copy = rng.random((Ho, Wo)) < 0.5
    for dst, src in zip(hi[:3], lo[:3]):
        dst[copy] = src[y0][:, x0][copy]
    hit_lo = np.broadcast_to(np.arange(W)[None, :] < (W + 1) // 2, (H, W)).copy()
    hit_hi = np.broadcast_to(np.arange(Wo)[None, :] < ((W + 1) // 2 * Wo) // W + (3 if Wo > W else 0), (Ho, Wo)).copy()
    if Wo >= 16:
        hit_hi[Ho // 2, 2] = False
        hit_hi[Ho // 2, Wo - 2] = True
    if Wo == 2 * W and Ho == 2 * H and W >= 4:
        for (x, y), n in (((1, 1), _NORMALS[1]), ((2, 2), _NORMALS[6])):
            lo.normal[y, x], hi.normal[2 * y, 2 * x] = _NORMALS[0], n
            hi.t[2 * y, 2 * x], hi.albedo[2 * y, 2 * x] = lo.t[y, x], lo.albedo[y, x]
            hit_hi[2 * y, 2 * x] = hit_lo[y, x] = True
    lo, hi = finish(lo, hit_lo), finish(hi, hit_hi)
    if W * H > 1:
        lo.normal[0, 0, 1] = np.nan
        lo.albedo[H - 1, 0, 0] = np.nan
        hi.t[Ho - 1, 0] = np.nan
        hi.albedo[0, 1] = np.nan
        hi.normal[Ho - 1, 1, 2] = np.nan
    return colour, lo, hi


def bilinear(colour, Wo, Ho, dtype=np.float32):
    """Plain bilinear interpolation of colour [H, W, 4] to [Ho, Wo, 4] with the source positions, taps and tap order of stage 1 and
    no guides: what upscale() gives where every pixel of both sizes is a miss (demodulate 0)."""
    f = dtype
    c = np.ascontiguousarray(colour, np.float32)[..., :3].astype(f)
    H, W = c.shape[:2]
    x0, wx0, wx1 = source_position(Wo, W, f)
    y0, wy0, wy1 = source_position(Ho, H, f)
    S, A = np.zeros((Ho, Wo), f), np.zeros((Ho, Wo, 3), f)
    for j in range(2):
        for i in range(2):
            b = ((wx1 if i else wx0)[None, :] * (wy1 if j else wy0)[:, None]).astype(f)
            v = c[np.minimum(y0 + j, H - 1)][:, np.minimum(x0 + i, W - 1)]
            S = np.where(b > 0, S + b, S)
            A = np.where((b > 0)[..., None], A + v * b[..., None], A)
    return np.concatenate([(A / S[..., None]).astype(f), np.ones((Ho, Wo, 1), f)], axis=-1)


def mse(a, b):
    d = np.asarray(a, np.float64)[..., :3] - np.asarray(b, np.float64)[..., :3]
    return float((d * d).mean())
