"""Restatement of the triangle distance query (include/drt.h drt_renderer_triangle_distance) in float32 numpy over nearest_ref.Geometry,
for the tests.  No tests of its own.

Every operation is one numpy operation in the arrays' dtype, in the order the header writes it (numpy rounds each one on its own; / is
the correctly rounded division; np.fmin / np.fmax drop a NaN operand as fminf / fmaxf do).  float32 is the rule; the same candidates and
the same predicate in float64 are the yardstick of the accuracy bound.  The point-triangle routine and the scenes are nearest_ref's,
the validity, the bounds, the predicate and pack are tri_overlap_ref's, by import.  The traversal is nearest_ref.nearest's with the
query's interval in the box distance and the pair test at the leaves; brute_force is the same pair test over ALL triangles.
"""
import collections

import numpy as np

from tests import nearest_ref as nr
from tests import tri_overlap_ref as tv
from tests.nearest_ref import Geometry, closest_on_triangle, dot  # noqa: F401  (re-exported)
from tests.tri_overlap_ref import pack, unpack  # noqa: F401  (re-exported)

NEAREST, ANY = 0, 1
TriNear = collections.namedtuple("TriNear", "point_q d2 point_t prim u v feature")
Pair = collections.namedtuple("Pair", "d2 feature candidates_d2 c_query c_scene u v")


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def clamp(x):
    """drt.h: fminf(fmaxf(x, 0), 1) + 0 -- a NaN gives 0, and a zero result is +0."""
    t = x.dtype.type
    return np.fmin(np.fmax(x, t(0)), t(1)) + t(0)


def segments(P1, d1, P2, d2):
    """drt.h "edge pair": (dist2, s, t, c1, c2) of the clamped closest points of P1 + d1 s and P2 + d2 t.  Every case's formula is
    evaluated, the header's case is selected."""
    with np.errstate(all="ignore"):
        r = P1 - P2
        a, e, f, c, b = dot(d1, d1), dot(d2, d2), dot(d2, r), dot(d1, r), dot(d1, d2)
        den = a * e - b * b
        zero, one = np.zeros_like(a), np.ones_like(a)
        s = np.where(den > 0, clamp((b * f - c * e) / den), zero)                # otherwise
        t = (b * s + f) / e
        lo, hi = t < 0, t > 1
        s = np.where(lo, clamp(-c / a), np.where(hi, clamp((b - c) / a), s))
        t = np.where(lo, zero, np.where(hi, one, t))
        s, t = np.where(e <= 0, clamp(-c / a), s), np.where(e <= 0, zero, t)      # e <= 0
        s, t = np.where(a <= 0, zero, s), np.where(a <= 0, clamp(f / e), t)       # a <= 0
        both = (a <= 0) & (e <= 0)
        s, t = np.where(both, zero, s), np.where(both, zero, t)
        c1, c2 = P1 + d1 * s[..., None], P2 + d2 * t[..., None]
        diff = c1 - c2
        return dot(diff, diff), s, t, c1, c2


def candidates(q0, q1, q2, v0, e1, e2):
    """drt.h "fifteen candidates" on (query, triangle) pairs, relative to q0, in order: (dist2, c_query, c_scene, u, v) each."""
    q0, q1, q2, v0, e1, e2 = np.broadcast_arrays(q0, q1, q2, v0, e1, e2)
    with np.errstate(all="ignore"):
        a1, a2 = q1 - q0, q2 - q0
        g = a2 - a1
        p0 = v0 - q0
        p1, p2 = p0 + e1, p0 + e2
        h = e2 - e1
        zero3 = np.zeros_like(a1)
        z, o = np.zeros_like(a1[..., 0]), np.ones_like(a1[..., 0])
        for P in (zero3, a1, a2):                                               # 0..2
            d, u, v, c = closest_on_triangle(P, p0, e1, e2)
            yield d, P, c, u, v
        for P, (u, v) in zip((p0, p1, p2), ((z, z), (o, z), (z, o))):             # 3..5
            d, _, _, c = closest_on_triangle(P, zero3, a1, a2)
            yield d, c, P, u, v
        for Q1, D1 in ((zero3, a1), (a1, g), (a2, -a2)):                          # 6..14
            for j, (P2, D2) in enumerate(((p0, e1), (p1, h), (p2, -e2))):
                d, s, t, c1, c2 = segments(Q1, D1, P2, D2)
                u, v = ((t, z), (o - t, t), (z, o - t))[j]
                yield d, c1, c2, u, v


def pair(q0, q1, q2, v0, e1, e2, witness=False):
    """drt.h "pair distance": Pair(d2, feature, the candidates' own minimum, and with `witness` the winning candidate's c_query,
    c_scene (relative to q0), u, v)."""
    best = cand = cq = ct = bu = bv = None
    for k, (d, c_query, c_scene, u, v) in enumerate(candidates(q0, q1, q2, v0, e1, e2)):
        if best is None:
            best, cand = np.full(d.shape, np.inf, d.dtype), np.zeros(d.shape, np.int32)
            if witness:
                cq, ct, bu, bv = (np.zeros(d.shape + (3,), d.dtype), np.zeros(d.shape + (3,), d.dtype), np.zeros(d.shape, d.dtype),
                                  np.zeros(d.shape, d.dtype))
        win = d < best                                                           # strict: the first wins a tie, a NaN never wins
        best, cand = np.where(win, d, best), np.where(win, np.int32(k), cand)
        if witness:
            cq, ct = np.where(win[..., None], c_query, cq), np.where(win[..., None], c_scene, ct)
            bu, bv = np.where(win, u, bu), np.where(win, v, bv)
    touch = tv.triangle_listed(q0, q1, q2, v0, e1, e2)
    d2 = np.where(touch, best.dtype.type(0), best)
    return Pair(d2, np.where(touch, cand | 16, cand).astype(np.int32), best, cq, ct, bu, bv)


def witness_of(q0, q1, q2, v0, e1, e2, cand):
    """(c_query, c_scene, u, v) of candidate `cand` [n] of each pair, as drt.h "result" takes them."""
    cq = ct = bu = bv = None
    for k, (d, c_query, c_scene, u, v) in enumerate(candidates(q0, q1, q2, v0, e1, e2)):
        if cq is None:
            cq, ct, bu, bv = np.zeros_like(c_query), np.zeros_like(c_query), np.zeros_like(d), np.zeros_like(d)
        sel = cand == k
        cq, ct, bu, bv = np.where(sel[..., None], c_query, cq), np.where(sel[..., None], c_scene, ct), np.where(sel, u, bu), np.where(sel, v, bv)
    return cq, ct, bu, bv


def box_dist2(bmin, bmax, qmin, qmax):
    """drt.h "node bound"."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.fmax(np.fmax(bmin - qmax, nr.F0), qmin - bmax)
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _best_of(max_dist, n):
    md = _f32(np.broadcast_to(np.float32(np.inf) if max_dist is None else np.asarray(max_dist, np.float32), n))
    with np.errstate(all="ignore"):
        return (md * md).astype(np.float32)


def _result(g, q, best, prim, feature):
    """The records of drt.h "result" from the winning (prim, candidate)."""
    n = len(q)
    hit = prim >= 0
    point_q, point_t = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    u, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    if hit.any():
        k = np.where(hit, prim, 0)
        with np.errstate(all="ignore"):
            cq, ct, bu, bv = witness_of(q[:, 0], q[:, 1], q[:, 2], g.v0[k], g.e1[k], g.e2[k], feature & 15)
            pq, pt = q[:, 0] + cq, q[:, 0] + ct
        point_q, point_t = np.where(hit[:, None], pq, nr.F0).astype(np.float32), np.where(hit[:, None], pt, nr.F0).astype(np.float32)
        u, v = np.where(hit, bu, nr.F0).astype(np.float32), np.where(hit, bv, nr.F0).astype(np.float32)
    return TriNear(point_q, best, point_t, prim.astype(np.int32), u, v, np.where(hit, feature, 0).astype(np.int32))


def records(res):
    """drt_tri_near records [N, 12] float32 of a TriNear: the bytes the entry point writes."""
    n = len(res.d2)
    out = np.zeros((n, 12), np.float32)
    out[:, 0:3], out[:, 3], out[:, 4:7], out[:, 8], out[:, 9] = res.point_q, res.d2, res.point_t, res.u, res.v
    out.view(np.int32)[:, 7], out.view(np.int32)[:, 10] = res.prim, res.feature
    return out


def distance(g, tris, max_dist=None, mode=NEAREST, visits=None, tests=None, depth=None):
    """drt.h "traversal" for queries [N, 3, 3] (or packed [N, 12]) with max_dist None (infinite), a scalar or [N]: TriNear.  visits /
    tests / depth: int64 [N] arrays that receive the nodes each query visited (popped and not dropped), the pairs it tested and the most
    entries its stack held."""
    q = unpack(tris)
    n = len(q)
    best = _best_of(max_dist, n)
    prim = np.full(n, -1, np.int64)
    feature = np.zeros(n, np.int32)
    if len(g.bmin) == 0 or n == 0:
        return _result(g, q, best, prim, feature)
    qmin, qmax = tv.bounds_of(q)
    root = len(g.bmin) - 1                                                     # the root is the last node
    st_node = np.zeros((n, nr.MAX_STACK), np.int64)
    st_box2 = np.zeros((n, nr.MAX_STACK), np.float32)
    st_node[:, 0] = root
    st_box2[:, 0] = box_dist2(g.bmin[root], g.bmax[root], qmin, qmax)
    sp = tv.valid(q).astype(np.int64)                                          # an invalid query pushes nothing
    while True:
        act = np.nonzero(sp > 0)[0]
        if len(act) == 0:
            break
        sp[act] -= 1
        node, box2 = st_node[act, sp[act]], st_box2[act, sp[act]]
        keep = box2 < best[act]                                                 # dropped unless box2 < best
        act, node = act[keep], node[keep]
        if visits is not None:
            visits[act] += 1
        leaf = g.is_leaf[node]
        la, ln = act[leaf], node[leaf]
        start, count = g.start[ln], g.count[ln]
        done = np.zeros(len(la), bool)                                          # mode ANY: the query has its pair
        for k in range(int(count.max()) if len(ln) else 0):                    # a leaf's triangles in order, strict <
            sel = (count > k) & ~done
            r, t = la[sel], start[sel] + k
            if tests is not None:
                tests[r] += 1
            p = pair(q[r, 0], q[r, 1], q[r, 2], g.v0[t], g.e1[t], g.e2[t])
            win = p.d2 < best[r]
            if mode == ANY:
                done[np.nonzero(sel)[0][win]] = True
                sp[r[win]] = 0                                                  # the query ends at the first pair within the distance
            r, t = r[win], t[win]
            best[r], prim[r], feature[r] = p.d2[win], t, p.feature[win]
        ia, inode = act[~leaf], node[~leaf]
        if len(ia):
            c1, c2 = g.child1[inode], g.child2[inode]
            b1, b2 = box_dist2(g.bmin[c1], g.bmax[c1], qmin[ia], qmax[ia]), box_dist2(g.bmin[c2], g.bmax[c2], qmin[ia], qmax[ia])
            p1, p2 = b1 < best[ia], b2 < best[ia]
            far1 = b1 > b2                                                      # the farther child first
            for push, c, d in ((np.where(far1, p1, p2), np.where(far1, c1, c2), np.where(far1, b1, b2)),
                               (np.where(far1, p2, p1), np.where(far1, c2, c1), np.where(far1, b2, b1))):
                r = ia[push]
                st_node[r, sp[r]], st_box2[r, sp[r]] = c[push], d[push]
                sp[r] += 1
            if depth is not None:
                depth[ia] = np.maximum(depth[ia], sp[ia])
    return _result(g, q, best, prim, feature)


def brute_force(g, tris, max_dist=None, dtype=np.float32, chunk=32):
    """The pair test of every valid query over ALL triangles in `dtype`: (minimum d2 below max_dist^2, else max_dist^2; its first
    triangle or -1; its feature).  float32: the rule without the tree.  float64: the yardstick (candidates and predicate in float64)."""
    q = unpack(tris)
    n = len(q)
    best = _best_of(max_dist, n).astype(dtype)
    prim = np.full(n, -1, np.int64)
    feature = np.zeros(n, np.int32)
    ok = tv.valid(q)
    qd = q.astype(dtype)
    v0, e1, e2 = (x.astype(dtype) for x in (g.v0, g.e1, g.e2))
    if len(v0) == 0:
        return best, prim, feature
    for s in range(0, n, chunk):
        e = slice(s, s + chunk)
        p = pair(qd[e, None, 0], qd[e, None, 1], qd[e, None, 2], v0[None], e1[None], e2[None])
        d2 = np.where(np.isnan(p.d2), np.inf, p.d2)
        k = d2.argmin(axis=1)                                                  # (the first of equal minima)
        rows = np.arange(len(k))
        m = d2[rows, k]
        win = (m < best[e]) & ok[e]
        best[e] = np.where(win, m, best[e])
        prim[e] = np.where(win, k, -1)
        feature[e] = np.where(win, p.feature[rows, k], 0)
    return best, prim, feature


def query_triangles(g, n, rng, scale=3.0):
    """About n query triangles [N, 3, 3] of size U^3 * 0.3 * extent: a third centred near surfaces, a third in the scene's box, a third
    in a box `scale` times larger."""
    k = max(n // 3, 1)
    lo, hi = nr.bounds(g)
    extent = np.float32((hi - lo).max())
    center = np.concatenate([nr.surface_points(g, k, rng), nr.box_points(g, k, rng), nr.box_points(g, k, rng, scale)]).astype(np.float32)
    m = len(center)
    size = (rng.uniform(0, 1, (m, 1, 1)) ** 3 * np.float32(0.3) * extent).astype(np.float32)
    return (center[:, None, :] + rng.uniform(-1, 1, (m, 3, 3)).astype(np.float32) * size).astype(np.float32)


def scale_of(g, tris):
    """M of the accuracy bound: per query, the largest absolute coordinate of the query and the scene (float64)."""
    lo, hi = nr.bounds(g)
    return np.maximum(np.abs(np.asarray(unpack(tris), np.float64)).max(axis=(1, 2)), max(np.abs(lo).max(), np.abs(hi).max()))
