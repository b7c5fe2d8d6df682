"""Restatement of adaptive sampling's rule (include/drt.h, drt_renderer_render_adaptive), for the tests.  No tests of its own.

Everything is the rule operation by operation in numpy: float32 with one rounding per operation for the weights and the fold,
integer arithmetic (uint64 where the rule says so) for the counts.  A state is State(sum [P, 3] float32, n [P] uint32, m1 [P],
m2 [P] float32) over the pixels p = x + y * width.
"""
import collections

import numpy as np

F = np.float32
CAP = np.uint32(16777215)
State = collections.namedtuple("State", "sum n m1 m2")
DEFAULTS = dict(min_spp=1, max_spp=64, target_error=0.0, luma_floor=0.01)


def empty_state(pixels):
    return State(np.zeros((pixels, 3), F), np.zeros(pixels, np.uint32), np.zeros(pixels, F), np.zeros(pixels, F))


def lum(c):
    """drt.h's lum(): 0.2126f r + 0.7152f g + 0.0722f b, left to right."""
    c = np.asarray(c, F)
    return ((F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]).astype(F)


def weights(state, target_error=0.0, luma_floor=0.01):
    """q uint32 [P]: 16777215 where n < 2 or w is NaN / infinite / too large, 0 where the pixel is converged."""
    te, lf = F(target_error), F(luma_floor)
    n = state.n.astype(np.uint32)
    with np.errstate(all="ignore"):
        fn = n.astype(F)
        mean = (state.m1.astype(F) / fn).astype(F)
        var = np.fmax((state.m2.astype(F) / fn).astype(F) - (mean * mean).astype(F), F(0)).astype(F)
        w = (np.sqrt((var / fn).astype(F)).astype(F) / (mean + lf).astype(F)).astype(F)
        s = (w * F(65536.0)).astype(F)
        below = s < F(16777215.0)                        # (False for NaN and +inf)
        q = np.where(below, np.where(below, s, F(0)).astype(np.uint32), CAP).astype(np.uint32)
        if te > 0:
            q = np.where(w <= te, np.uint32(0), q)
    return np.where(n < 2, CAP, q).astype(np.uint32)


def counts(q, budget, min_spp=1, max_spp=64, thresholded=False):
    """(counts uint32 [P], Q) from the weights: integer arithmetic, (uint64)extra * q / Q floored."""
    q = np.asarray(q, np.uint32)
    pixels = len(q)
    assert min_spp * pixels <= budget < 2 ** 31 and 1 <= max_spp >= min_spp
    Q = int(q.astype(np.uint64).sum(dtype=np.uint64))
    extra = budget - min_spp * pixels
    if Q == 0 and not thresholded:
        return np.full(pixels, min(max_spp, min_spp + extra // pixels), np.uint32), Q
    if Q == 0:
        return np.zeros(pixels, np.uint32), Q
    share = (np.uint64(extra) * q.astype(np.uint64)) // np.uint64(Q)        # < 2^55: exact in uint64
    c = np.minimum(np.uint64(max_spp), np.uint64(min_spp) + share).astype(np.uint32)
    return np.where(q == 0, np.uint32(0 if thresholded else min_spp), c).astype(np.uint32), Q


def plan(state, budget, min_spp=1, max_spp=64, target_error=0.0, luma_floor=0.01):
    """(q, counts) of a call on `state`."""
    q = weights(state, target_error, luma_floor)
    c, _ = counts(q, budget, min_spp, max_spp, thresholded=F(target_error) > 0)
    return q, c


def offsets(c):
    """The exclusive prefix sum of the counts, uint32."""
    c = np.asarray(c, np.uint32)
    out = np.zeros(len(c), np.uint64)
    np.cumsum(c[:-1], dtype=np.uint64, out=out[1:])
    return out.astype(np.uint32)


def fold(state, c, sample):
    """The state after a call with counts c: sample(k) -> float32 [P, 3] is every pixel's sample of FRAME k (k >= 1); pixel p takes
    frames n[p] + 1 .. n[p] + c[p], in that order."""
    s, n, m1, m2 = state.sum.copy(), state.n.copy(), state.m1.copy(), state.m2.copy()
    c = np.asarray(c, np.uint32)
    frames = n.astype(np.int64)
    last = (frames + c).astype(np.int64)
    for k in range(int(frames[c > 0].min()) + 1 if (c > 0).any() else 1, int(last.max()) + 1 if (c > 0).any() else 1):
        take = (frames < k) & (k <= last)
        if not take.any():
            continue
        col = np.asarray(sample(k), F).reshape(-1, 3)[take]
        y = lum(col)
        s[take] = (s[take] + col).astype(F)
        m1[take] = (m1[take] + y).astype(F)
        m2[take] = (m2[take] + (y * y).astype(F)).astype(F)
    return State(s, (n + c).astype(np.uint32), m1, m2)


def image(state):
    """[P, 4]: sum / (float)n with alpha 1, (0, 0, 0, 1) where n == 0."""
    out = np.zeros((len(state.n), 4), F)
    out[:, 3] = 1
    has = state.n > 0
    out[has, :3] = (state.sum[has] / state.n[has].astype(F)[:, None]).astype(F)
    return out
