"""Restatement of the motion rule of include/drt.h (drt_renderer_track_motion, drt_renderer_motion_vectors) in float32 numpy, on
top of tests/temporal_ref.py.  No tests of its own.

previous_points(): P' and n' per pixel from the current TriHot records and the snapshot's, operation by operation as the header
writes them.  reproject_motion(): stage (b) of temporal_ref.reproject with P' in place of P and the tap's normal test against n'
(that function computes P inside itself, so its body is restated here; with nothing moved the two agree bit for bit, which
tests/test_motion_ref.py checks).  motion_vectors(): the projection of P' alone.

`hot` / `hot_prev` are TriHot arrays as Scene.debugPack() and Renderer.debugReadDeviceScene() return them (uint8 [n, 48]) or
float32 [n, 12]: v0, e1, e2, fn.
"""
import numpy as np

import oracle
from tests import refit_ref as rf
from tests import temporal_ref as tp
from tests.temporal_ref import F, History, _dot3, luminance, primary_directions

STATIC, MOVED = 1, 2


def records(hot):
    """TriHot records as float32 [n, 12]."""
    hot = np.ascontiguousarray(hot)
    return hot.view(np.float32).reshape(-1, 12) if hot.dtype == np.uint8 else np.ascontiguousarray(hot, F).reshape(-1, 12)


def moved_triangles(hot, hot_prev):
    """bool [n]: the nine words v0, e1, e2 differ bitwise."""
    a, b = records(hot).view(np.uint32)[:, :9], records(hot_prev).view(np.uint32)[:, :9]
    return (a != b).any(axis=1)


def previous_points(guides, ph, hot, hot_prev):
    """(P' [H, W, 3], n' [H, W, 3], rule [H, W]) -- rule 0 where prim < 0 (P' = P, n' = the guide's normal there), STATIC or MOVED."""
    prim, normal, t = np.asarray(guides.prim, np.int32), np.asarray(guides.normal, F), np.asarray(guides.t, F)
    H, W = prim.shape
    with np.errstate(all="ignore"):
        P = (ph.pos + primary_directions(ph, W, H) * t[..., None]).astype(F)
    rule = np.where(prim >= 0, STATIC, 0).astype(np.int32)
    if hot_prev is None:
        return P, normal.copy(), rule
    cur, old = records(hot), records(hot_prev)
    k = np.clip(prim, 0, len(cur) - 1)
    moved = moved_triangles(cur, old)[k] & (prim >= 0)
    v0, e1, e2, fn = cur[k, 0:3], cur[k, 3:6], cur[k, 6:9], cur[k, 9:12]
    pv0, pe1, pe2, pfn = old[k, 0:3], old[k, 3:6], old[k, 6:9], old[k, 9:12]
    with np.errstate(all="ignore"):
        w = (P - v0).astype(F)
        d11, d12, d22 = _dot3(e1, e1), _dot3(e1, e2), _dot3(e2, e2)
        w1, w2 = _dot3(w, e1), _dot3(w, e2)
        den = ((d11 * d22).astype(F) - (d12 * d12).astype(F)).astype(F)
        moved &= den > 0
        b1 = (((d22 * w1).astype(F) - (d12 * w2).astype(F)).astype(F) / den).astype(F)
        b2 = (((d11 * w2).astype(F) - (d12 * w1).astype(F)).astype(F) / den).astype(F)
        Pm = ((pv0 + (pe1 * b1[..., None]).astype(F)).astype(F) + (pe2 * b2[..., None]).astype(F)).astype(F)
        nm = np.where((_dot3(fn, normal) < 0)[..., None], -pfn, pfn).astype(F)
    m3 = moved[..., None]
    return np.where(m3, Pm, P).astype(F), np.where(m3, nm, normal).astype(F), np.where(moved, MOVED, rule).astype(np.int32)


def motion_vectors(guides, ph, ph_prev, hot=None, hot_prev=None):
    """float32 [H, W, 4]: (fx - x, fy - y, z, flag) of drt_renderer_motion_vectors."""
    prim = np.asarray(guides.prim, np.int32)
    H, W = prim.shape
    Pp, _, rule = previous_points(guides, ph, hot, hot_prev)
    with np.errstate(all="ignore"):
        pv = (Pp - ph_prev.pos).astype(F)
        z = _dot3(pv, ph_prev.forward)
        fx, fy, _ = tp.project(ph_prev, Pp, W, H)
        y, x = np.mgrid[0:H, 0:W]
        out = np.stack([(fx - x.astype(F)).astype(F), (fy - y.astype(F)).astype(F), z, rule.astype(F)], axis=-1).astype(F)
    ok = (prim >= 0) & (z > 0)
    return np.where(ok[..., None], out, F(0)).astype(F)


def reproject_motion(prev, rgba, guides, ph, hot=None, hot_prev=None, max_history=32, alpha_min=0.0, normal_cos_min=0.9, **_):
    """Stage (b) with the motion rule: the History after one call.  Arguments as temporal_ref.reproject, plus the current TriHot
    records and the snapshot's (None = nothing armed: the static rule everywhere)."""
    c = np.ascontiguousarray(rgba, F)[..., :3]
    H, W = c.shape[:2]
    prim, normal = np.asarray(guides.prim, np.int32), np.asarray(guides.normal, F)
    l = luminance(c)
    S = np.zeros((H, W), F)
    hN, h1, h2, hc = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W, 3), F)
    if prev is not None:
        Pp, n_tap, _ = previous_points(guides, ph, hot, hot_prev)
        fx, fy, ok = tp.project(prev.pinhole, Pp, W, H)
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
                with np.errstate(all="ignore"):
                    valid &= _dot3(prev.normal[cy, cx], n_tap) >= F(normal_cos_min)
                w = np.where(valid, (wx[i] * wy[j]).astype(F), F(0))
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


FIELDS = ("color", "length", "m1", "m2", "variance", "weight")


def history_differences(a, b):
    """{field: number of pixels whose uint32 words differ} over the fields of two Histories that differ."""
    out = {}
    for f in FIELDS:
        x, y = np.ascontiguousarray(getattr(a, f), F).view(np.uint32), np.ascontiguousarray(getattr(b, f), F).view(np.uint32)
        bad = x != y
        if bad.any():
            out[f] = int(bad.reshape(bad.shape[0], bad.shape[1], -1).any(axis=-1).sum())
    return out


def oracle_scene(sc, st, mats, texs, pos):
    """The oracle's scene after a refit of the product scene `sc` (its tree as built) to load-order positions `pos`: st = the
    load-order streams (refit_ref.streams before the build), mats = [(albedo, tex)], texs = the oracle's textures."""
    order = sc.triangleOrder()
    osc = oracle.Scene(rf.triangles(pos, st[1], st[2], st[3], order=order), mats, texs)
    osc.nodes = rf.oracle_tree(rf.nodes(sc.m_BVHNodes, np.asarray(pos, F)[order]))
    return osc


def rotate_about(points, origin, axis, angle):
    """points [..., 3] rotated by `angle` about the line through `origin` along `axis` (Rodrigues, float64 -> float32)."""
    k = np.float64(axis) / np.linalg.norm(axis)
    v = np.float64(points) - np.float64(origin)
    co, si = np.cos(angle), np.sin(angle)
    out = v * co + np.cross(k, v) * si + k * (v @ k)[..., None] * (1 - co)
    return (out + np.float64(origin)).astype(F)
