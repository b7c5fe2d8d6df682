"""Restatement of the triangle cast (include/drt.h drt_renderer_triangle_cast) in float32 numpy over nearest_ref.Geometry, for the
tests.  No tests of its own.

Every operation is one numpy operation in the arrays' dtype, in the order the header writes it (numpy rounds each one on its own; / is
the correctly rounded division; np.fmin / np.fmax drop a NaN operand as fminf / fmaxf do).  float32 is the rule; the same candidates and
the same predicate in float64 are the yardstick of the accuracy bound; on small integers every float32 product and sum is exact, which
is what the exact check uses.  The scenes and Geometry are nearest_ref's, the validity, the bounds, the predicate, cross and pack are
tri_overlap_ref's, the query triangles are tri_distance_ref's, by import.  The traversal is sweep_ref.sphere_cast's with the widened
box and the pair test at the leaves; brute_force is the same pair test over ALL triangles.
"""
import collections

import numpy as np

from tests import nearest_ref as nr
from tests import tri_overlap_ref as tv
from tests.nearest_ref import Geometry, dot  # noqa: F401  (re-exported)
from tests.tri_distance_ref import query_triangles  # noqa: F401  (re-exported)
from tests.tri_overlap_ref import cross, pack, unpack  # noqa: F401  (re-exported)

FIRST, ANY = 0, 1
TriHits = collections.namedtuple("TriHits", "point t normal prim u v feature")
Pair = collections.namedtuple("Pair", "t feature tau")


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _signed(det, *nums):
    """drt.h "how a quotient is formed": sg = det < 0 ? -1 : 1, ad = fabsf(det), every numerator times sg."""
    sg = np.where(det < 0, det.dtype.type(-1), det.dtype.type(1))
    return (np.abs(det),) + tuple(n * sg for n in nums)


def ray(o, d, w0, f1, f2):
    """drt.h "0..5": the ray (o, d) against (w0, f1, f2): (passes, ad, nu, nv, ntau)."""
    with np.errstate(all="ignore"):
        pv = cross(d, f2)
        det = dot(f1, pv)
        tvec = o - w0
        qv = cross(tvec, f1)
        ad, nu, nv, nt = _signed(det, dot(tvec, pv), dot(d, qv), dot(f2, qv))
        ok = (det != 0) & (nu >= 0) & (nv >= 0) & (nu + nv <= ad) & (nt >= 0)
        return ok, ad, nu, nv, nt


def edges(a, ea, b, eb, d):
    """drt.h "6..14": a + ea s + d tau = b + eb w: (passes, ad, ns, nw, ntau)."""
    with np.errstate(all="ignore"):
        nb = -eb
        c = cross(d, nb)
        det = dot(ea, c)
        r = b - a
        ad, ns, nt, nw = _signed(det, dot(r, c), dot(ea, cross(r, nb)), dot(ea, cross(d, r)))
        ok = (det != 0) & (ns >= 0) & (ns <= ad) & (nw >= 0) & (nw <= ad) & (nt >= 0)
        return ok, ad, ns, nw, nt


def quot(n, ad):
    with np.errstate(all="ignore"):
        return np.abs(n) / ad


def candidates(q0, q1, q2, d, v0, e1, e2):
    """drt.h "fifteen candidates" on (cast, triangle) pairs, relative to q0, in order: (passes, tau, c_scene, u, v, normal) each; tau, the
    contact and the normal are meaningful where the candidate passes."""
    q0, q1, q2, d, v0, e1, e2 = np.broadcast_arrays(q0, q1, q2, d, v0, e1, e2)
    with np.errstate(all="ignore"):
        a1, a2 = q1 - q0, q2 - q0
        g = a2 - a1
        nq = cross(a1, a2)
        p0 = v0 - q0
        p1, p2 = p0 + e1, p0 + e2
        h = e2 - e1
        zero3 = np.zeros_like(a1)
        z, o = np.zeros_like(a1[..., 0]), np.ones_like(a1[..., 0])
        nt = cross(e1, e2)
        for P in (zero3, a1, a2):                                               # 0..2
            ok, ad, nu, nv, ntau = ray(P, d, p0, e1, e2)
            u, v = quot(nu, ad), quot(nv, ad)
            yield ok, quot(ntau, ad), (p0 + e1 * u[..., None]) + e2 * v[..., None], u, v, nt
        for P, (u, v) in zip((p0, p1, p2), ((z, z), (o, z), (z, o))):             # 3..5
            ok, ad, _, _, ntau = ray(P, -d, zero3, a1, a2)
            yield ok, quot(ntau, ad), P, u, v, nq
        for A, EA in ((zero3, a1), (a1, g), (a2, -a2)):                           # 6..14
            for j, (B, EB) in enumerate(((p0, e1), (p1, h), (p2, -e2))):
                ok, ad, _, nw, ntau = edges(A, EA, B, EB, d)
                w = quot(nw, ad)
                u, v = ((w, z), (o - w, w), (z, o - w))[j]
                yield ok, quot(ntau, ad), B + EB * w[..., None], u, v, cross(EA, EB)


def pair(q0, q1, q2, d, v0, e1, e2):
    """drt.h "the pair's t": Pair(t, feature, the candidates' own minimum tau)."""
    best = cand = None
    for k, (ok, tau, *_) in enumerate(candidates(q0, q1, q2, d, v0, e1, e2)):
        if best is None:
            best, cand = np.full(tau.shape, np.inf, tau.dtype), np.full(tau.shape, 15, np.int32)
        with np.errstate(invalid="ignore"):
            win = ok & (tau < best)                                              # strict: the first wins a tie
        best, cand = np.where(win, tau, best), np.where(win, np.int32(k), cand)
    touch = tv.triangle_listed(q0, q1, q2, v0, e1, e2)
    return Pair(np.where(touch, best.dtype.type(0), best), np.where(touch, cand | 16, cand).astype(np.int32), best)


def contact_of(q0, q1, q2, d, v0, e1, e2, cand):
    """(c_scene, u, v, normal) of candidate `cand` [n] of each pair, as drt.h "result" takes them (normal not yet flipped)."""
    ct = bu = bv = nrm = None
    for k, (ok, tau, c, u, v, n) in enumerate(candidates(q0, q1, q2, d, v0, e1, e2)):
        if ct is None:
            ct, nrm, bu, bv = np.zeros_like(c), np.zeros_like(c), np.zeros_like(u), np.zeros_like(u)
        sel = cand == k
        ct, nrm, bu, bv = np.where(sel[..., None], c, ct), np.where(sel[..., None], n, nrm), np.where(sel, u, bu), np.where(sel, v, bv)
    return ct, bu, bv, nrm


def widened_slab(bmin, bmax, ext_lo, ext_hi, o, inv_d, best):
    """drt.h "traversal": (visited, enter) of boxes [k, 3] against casts [k]."""
    with np.errstate(all="ignore"):
        t0 = ((bmin - ext_hi) - o) * inv_d
        t1 = ((bmax - ext_lo) - o) * inv_d
        lo, hi = np.fmin(t0, t1), np.fmax(t1, t0)
        enter = np.fmax(np.fmax(lo[:, 0], lo[:, 1]), lo[:, 2])
        exit_ = np.fmin(np.fmin(hi[:, 0], hi[:, 1]), hi[:, 2])
        return (enter <= exit_) & (exit_ >= 0) & (enter <= best), enter


def _motions(n, dirs, tmax):
    d = _f32(np.broadcast_to(np.asarray(dirs, np.float32), (n, 3)))
    return d, _f32(np.broadcast_to(np.asarray(tmax, np.float32), n))


def valid(q, d, tmax):
    return tv.valid(q) & ~np.isnan(d).any(axis=1) & ~np.isnan(tmax)


def _result(g, q, d, best, prim, feature):
    """The records of drt.h "result" from the winning (prim, candidate)."""
    n = len(q)
    hit = prim >= 0
    point, normal = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    u, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    contact = hit & ((feature & 16) == 0)                                       # a start overlap has no contact: zeros
    if contact.any():
        k = np.where(contact, prim, 0)
        with np.errstate(all="ignore"):
            ct, bu, bv, nrm = contact_of(q[:, 0], q[:, 1], q[:, 2], d, g.v0[k], g.e1[k], g.e2[k], np.where(contact, feature, -1))
            p = q[:, 0] + ct
            nrm = np.where((dot(nrm, d) > 0)[:, None], -nrm, nrm)               # flipped against the motion
        point, normal = np.where(contact[:, None], p, nr.F0).astype(np.float32), np.where(contact[:, None], nrm, nr.F0).astype(np.float32)
        u, v = np.where(contact, bu, nr.F0).astype(np.float32), np.where(contact, bv, nr.F0).astype(np.float32)
    return TriHits(point, best, normal, prim.astype(np.int32), u, v, np.where(hit, feature, -1).astype(np.int32))


def records(res):
    """drt_tri_hit records [N, 12] float32 of a TriHits: the bytes the entry point writes."""
    n = len(res.t)
    out = np.zeros((n, 12), np.float32)
    out[:, 0:3], out[:, 3], out[:, 4:7], out[:, 8], out[:, 9] = res.point, res.t, res.normal, res.u, res.v
    out.view(np.int32)[:, 7], out.view(np.int32)[:, 10] = res.prim, res.feature
    return out


def cast(g, tris, dirs, tmax=1.0, mode=FIRST, visits=None, tests=None, depth=None):
    """drt.h "traversal" for casts [N, 3, 3] (or packed [N, 12]) with dirs [3] or [N, 3] and tmax a scalar or [N]: TriHits.  visits /
    tests / depth: int64 [N] arrays that receive the nodes each cast visited (popped and not dropped), the pairs it tested and the most
    entries its stack held."""
    q = unpack(tris)
    n = len(q)
    d, tmax = _motions(n, dirs, tmax)
    best = tmax.copy()
    prim = np.full(n, -1, np.int64)
    feature = np.full(n, -1, np.int32)
    if len(g.bmin) == 0 or n == 0:
        return _result(g, q, d, best, prim, feature)
    qmin, qmax = tv.bounds_of(q)
    with np.errstate(all="ignore"):
        ext_lo, ext_hi = qmin - q[:, 0], qmax - q[:, 0]
        inv_d = (np.float32(1) / d).astype(np.float32)
    o = q[:, 0]
    root = len(g.bmin) - 1                                                     # the root is the last node
    st_node = np.zeros((n, nr.MAX_STACK), np.int64)
    st_enter = np.zeros((n, nr.MAX_STACK), np.float32)
    with np.errstate(invalid="ignore"):
        ok, enter = widened_slab(g.bmin[root][None], g.bmax[root][None], ext_lo, ext_hi, o, inv_d, best)
    ok &= valid(q, d, tmax)                                                    # an invalid cast pushes nothing
    st_node[:, 0], st_enter[:, 0] = root, enter
    sp = ok.astype(np.int64)
    while True:
        act = np.nonzero(sp > 0)[0]
        if len(act) == 0:
            break
        sp[act] -= 1
        node, enter = st_node[act, sp[act]], st_enter[act, sp[act]]
        with np.errstate(invalid="ignore"):
            keep = enter <= best[act]                                           # dropped unless enter <= best
        act, node = act[keep], node[keep]
        if visits is not None:
            visits[act] += 1
        leaf = g.is_leaf[node]
        la, ln = act[leaf], node[leaf]
        start, count = g.start[ln], g.count[ln]
        done = np.zeros(len(la), bool)                                          # mode ANY: the cast has its pair
        for k in range(int(count.max()) if len(ln) else 0):                    # a leaf's triangles in order
            sel = (count > k) & ~done
            r, t = la[sel], start[sel] + k
            if tests is not None:
                tests[r] += 1
            p = pair(q[r, 0], q[r, 1], q[r, 2], d[r], g.v0[t], g.e1[t], g.e2[t])
            with np.errstate(invalid="ignore"):
                first = p.t < best[r]
                win = first | ((p.t == best[r]) & (t < prim[r]))
            if mode == ANY:
                done[np.nonzero(sel)[0][first]] = True
                sp[r[first]] = 0                                                # the cast ends at the first pair with t < best
            r, t = r[win], t[win]
            best[r], prim[r], feature[r] = p.t[win], t, p.feature[win]
        ia, inode = act[~leaf], node[~leaf]
        if len(ia):
            c1, c2 = g.child1[inode], g.child2[inode]
            p1, en1 = widened_slab(g.bmin[c1], g.bmax[c1], ext_lo[ia], ext_hi[ia], o[ia], inv_d[ia], best[ia])
            p2, en2 = widened_slab(g.bmin[c2], g.bmax[c2], ext_lo[ia], ext_hi[ia], o[ia], inv_d[ia], best[ia])
            with np.errstate(invalid="ignore"):
                far1 = en1 > en2                                                # the farther child first
            for push, c, e in ((np.where(far1, p1, p2), np.where(far1, c1, c2), np.where(far1, en1, en2)),
                               (np.where(far1, p2, p1), np.where(far1, c2, c1), np.where(far1, en2, en1))):
                r = ia[push]
                st_node[r, sp[r]], st_enter[r, sp[r]] = c[push], e[push]
                sp[r] += 1
            if depth is not None:
                depth[ia] = np.maximum(depth[ia], sp[ia])
    return _result(g, q, d, best, prim, feature)


def brute_force(g, tris, dirs, tmax=1.0, dtype=np.float32, chunk=32):
    """The pair test of every valid cast over ALL triangles in `dtype`: (the smallest t below tmax, else tmax; its first triangle or -1;
    its feature or -1).  float32: the rule without the tree.  float64: the yardstick (candidates and predicate in float64)."""
    q = unpack(tris)
    n = len(q)
    d, tmax = _motions(n, dirs, tmax)
    best = tmax.astype(dtype)
    prim = np.full(n, -1, np.int64)
    feature = np.full(n, -1, np.int32)
    ok = valid(q, d, tmax)
    qd, dd = q.astype(dtype), d.astype(dtype)
    v0, e1, e2 = (x.astype(dtype) for x in (g.v0, g.e1, g.e2))
    if len(v0) == 0:
        return best, prim, feature
    for s in range(0, n, chunk):
        e = slice(s, s + chunk)
        p = pair(qd[e, None, 0], qd[e, None, 1], qd[e, None, 2], dd[e, None], v0[None], e1[None], e2[None])
        t = np.where(np.isnan(p.t), np.inf, p.t)
        k = t.argmin(axis=1)                                                   # (the first of equal minima: the smallest index)
        rows = np.arange(len(k))
        m = t[rows, k]
        with np.errstate(invalid="ignore"):
            win = (m < best[e]) & ok[e]
        best[e] = np.where(win, m, best[e])
        prim[e] = np.where(win, k, -1)
        feature[e] = np.where(win, p.feature[rows, k], -1)
    return best, prim, feature


def cast_sets(g, n, rng, scale=3.0):
    """About n casts (tris [N, 3, 3], dirs [N, 3]): tri_distance_ref.query_triangles' triangles -- a third near surfaces, a third in the
    scene's box, a third in a box `scale` times larger -- with random directions of lengths up to the scene's extent."""
    tris = query_triangles(g, n, rng, scale)
    lo, hi = nr.bounds(g)
    extent = np.float32((hi - lo).max())
    m = len(tris)
    v = rng.normal(size=(m, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return tris, (v * rng.uniform(0, 1, (m, 1)) * extent).astype(np.float32)


def scale_of(g, tris):
    """M of the accuracy bound: per cast, the largest absolute coordinate of the query and the scene (float64)."""
    lo, hi = nr.bounds(g)
    return np.maximum(np.abs(np.asarray(unpack(tris), np.float64)).max(axis=(1, 2)), max(np.abs(lo).max(), np.abs(hi).max()))
