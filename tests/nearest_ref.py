"""Restatement of the nearest-surface query (include/drt.h drt_renderer_nearest) in float32 numpy, for the tests.  No tests of its
own.

Every operation is one float32 numpy operation, in the order the header writes it (numpy rounds each one on its own; / is the
correctly rounded division; np.fmax drops a NaN operand as fmaxf does).  The traversal is vectorised over points as
ray_query_ref.closest is over rays: every step pops one stack entry of every point that still has one.  It runs over a Geometry:
the tree's topology and boxes plus the (v0, e1, e2, fn) records, taken from the oracle's scene (from_oracle) or from the product's
host scene and its packed TriHot records (from_product: Scene.m_BVHNodes + Scene.debugPack()).
"""
import collections

import numpy as np

Geometry = collections.namedtuple("Geometry", "bmin bmax is_leaf child1 child2 start count v0 e1 e2 fn")
Nearest = collections.namedtuple("Nearest", "point d2 prim u v side")
MAX_STACK = 64
F0, F1 = np.float32(0), np.float32(1)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _geometry(nodes, v0, e1, e2, fn):
    return Geometry(_f32(nodes["bmin"]), _f32(nodes["bmax"]), np.asarray(nodes["is_leaf"]) != 0, np.asarray(nodes["child1"], np.int64),
                    np.asarray(nodes["child2"], np.int64), np.asarray(nodes["prim_start"], np.int64),
                    np.asarray(nodes["prim_count"], np.int64), _f32(v0), _f32(e1), _f32(e2), _f32(fn))


def from_oracle(osc):
    """The oracle scene's nodes (root last) and triangles: e1 = v1 - v0, e2 = v2 - v0 as the pack stores them."""
    p = _f32(osc.tris["p"])
    return _geometry(osc.nodes, p[:, 0], p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], osc.tris["face_n"])


def from_product(sc):
    """The product's host scene: its nodes and the TriHot records of its pack (Scene.debugPack())."""
    _, hot, _ = sc.debugPack()
    h = hot.view(np.float32).reshape(-1, 12)
    return _geometry(sc.m_BVHNodes, h[:, 0:3], h[:, 3:6], h[:, 6:9], h[:, 9:12])


def from_triangles(p, fn=None):
    """Triangles p [T, 3, 3] under a tree of one leaf (no triangles: no nodes); fn defaults to zero."""
    p = _f32(p).reshape(-1, 3, 3)
    nodes = np.zeros(1 if len(p) else 0, [("bmin", "<f4", 3), ("bmax", "<f4", 3), ("is_leaf", "<i4"), ("child1", "<i4"), ("child2", "<i4"),
                                          ("prim_start", "<i4"), ("prim_count", "<i4")])
    if len(p):
        nodes[0] = (p.reshape(-1, 3).min(axis=0), p.reshape(-1, 3).max(axis=0), 1, -1, -1, 0, len(p))
    return _geometry(nodes, p[:, 0], p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], np.zeros((len(p), 3)) if fn is None else fn)


def dot(a, b):
    """(a.x b.x + a.y b.y) + a.z b.z"""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def closest_on_triangle(p, v0, e1, e2):
    """drt.h "per triangle" on (point, triangle) pairs, in the arrays' dtype (float32: the rule; float64: the brute-force yardstick):
    (dist2, u, v, c).  Every case's formula is evaluated, the first matching case is selected."""
    t = p.dtype.type
    zero, one = t(0), t(1)
    with np.errstate(all="ignore"):
        ap = p - v0
        d1, d2 = dot(e1, ap), dot(e2, ap)
        bp = ap - e1
        d3, d4 = dot(e1, bp), dot(e2, bp)
        cp = ap - e2
        d5, d6 = dot(e1, cp), dot(e2, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        cases = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = one / ((va + vb) + vc)
        z, o = np.zeros_like(d1), np.ones_like(d1)
        uv = [(z, z), (o, z), (d1 / (d1 - d3), z), (z, o), (z, d2 / (d2 - d6)), (one - w, w)]
        u, v = vb * den, vc * den                                              # case 7
        for case, (cu, cv) in reversed(list(zip(cases, uv))):                  # last case first: the first matching one wins
            u, v = np.where(case, cu, u), np.where(case, cv, v)
        c = (v0 + e1 * u[..., None]) + e2 * v[..., None]
        diff = p - c
        return dot(diff, diff), u, v, c


def box_dist2(bmin, bmax, p):
    """drt.h "box distance"."""
    with np.errstate(invalid="ignore"):
        d = np.fmax(np.fmax(bmin - p, F0), p - bmax)
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _result(g, p, best, prim, u, v):
    """The record of drt.h "result" from the winning (prim, u, v)."""
    n = len(p)
    hit = prim >= 0
    k = np.where(hit, prim, 0)
    point, side = np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
    if len(g.v0) and hit.any():
        with np.errstate(all="ignore"):
            c = (g.v0[k] + g.e1[k] * u[:, None]) + g.e2[k] * v[:, None]
            s = np.where(dot(p - c, g.fn[k]) < 0, np.float32(-1), F1)
        point, side = np.where(hit[:, None], c, F0).astype(np.float32), np.where(hit, s, F0).astype(np.float32)
    return Nearest(point, best, prim.astype(np.int32), np.where(hit, u, F0).astype(np.float32), np.where(hit, v, F0).astype(np.float32), side)


def nearest(g, points, max_dist=np.inf, visits=None):
    """drt.h "traversal" for points [n, 3] with max_dist a scalar or [n].  visits: an int64 [n] array that receives the number of
    nodes each point visited (popped and not dropped)."""
    p = _f32(points)
    n = len(p)
    md = _f32(np.broadcast_to(np.float32(max_dist) if np.isscalar(max_dist) else max_dist, n))
    with np.errstate(all="ignore"):
        best = (md * md).astype(np.float32)
    prim = np.full(n, -1, np.int64)
    bu, bv = np.zeros(n, np.float32), np.zeros(n, np.float32)
    if len(g.bmin) == 0 or n == 0:
        return _result(g, p, best, prim, bu, bv)
    root = len(g.bmin) - 1                                                     # the root is the last node
    st_node = np.zeros((n, MAX_STACK), np.int64)
    st_box2 = np.zeros((n, MAX_STACK), np.float32)
    st_node[:, 0] = root
    st_box2[:, 0] = box_dist2(g.bmin[root], g.bmax[root], p)
    sp = np.ones(n, np.int64)
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
        for k in range(int(count.max()) if len(ln) else 0):                    # a leaf's triangles in order, strict <
            sel = count > k
            r, t = la[sel], start[sel] + k
            d2, u, v, _ = closest_on_triangle(p[r], g.v0[t], g.e1[t], g.e2[t])
            win = d2 < best[r]
            r, t = r[win], t[win]
            best[r], prim[r], bu[r], bv[r] = d2[win], t, u[win], v[win]
        ia, inode = act[~leaf], node[~leaf]
        if len(ia):
            c1, c2 = g.child1[inode], g.child2[inode]
            b1, b2 = box_dist2(g.bmin[c1], g.bmax[c1], p[ia]), box_dist2(g.bmin[c2], g.bmax[c2], p[ia])
            p1, p2 = b1 < best[ia], b2 < best[ia]
            far1 = b1 > b2                                                      # the farther child first
            for push, c, d in ((np.where(far1, p1, p2), np.where(far1, c1, c2), np.where(far1, b1, b2)),
                               (np.where(far1, p2, p1), np.where(far1, c2, c1), np.where(far1, b2, b1))):
                r = ia[push]
                st_node[r, sp[r]], st_box2[r, sp[r]] = c[push], d[push]
                sp[r] += 1
    return _result(g, p, best, prim, bu, bv)


def brute_force(g, points, max_dist=np.inf, dtype=np.float32, chunk=256):
    """The per-triangle routine over ALL triangles in `dtype`: (minimum dist2 below max_dist^2, else max_dist^2; its first triangle or
    -1).  float32: the rule without the tree (NaN never wins, the first triangle wins a tie).  float64: the yardstick."""
    p = np.ascontiguousarray(points, dtype)
    n = len(p)
    md = np.broadcast_to(np.asarray(max_dist, np.float32), n).astype(dtype)
    with np.errstate(all="ignore"):
        best = md * md
    prim = np.full(n, -1, np.int64)
    v0, e1, e2 = (x.astype(dtype) for x in (g.v0, g.e1, g.e2))
    if len(v0) == 0:
        return best, prim
    for s in range(0, n, chunk):
        d2, *_ = closest_on_triangle(p[s:s + chunk, None, :], v0[None], e1[None], e2[None])
        d2 = np.where(np.isnan(d2), np.inf, d2)
        k = d2.argmin(axis=1)                                                  # (the first of equal minima)
        m = d2[np.arange(len(k)), k]
        win = m < best[s:s + chunk]
        best[s:s + chunk] = np.where(win, m, best[s:s + chunk])
        prim[s:s + chunk] = np.where(win, k, -1)
    return best, prim


# ---------------------------------------------------------------- scenes and point sets shared by the CPU and GPU tests

def oracle_soup(n, seed, leaf, bins):
    """ray_query_ref.soup(n, seed) as an oracle scene with a (leaf, bins) tree -- no product library needed."""
    import oracle
    from tests import ray_query_ref as rq
    from tests import refit_ref as rf
    pos, nrm, uv, mat, materials, textures = rq.soup(n, seed)
    return oracle.Scene(rf.triangles(pos, nrm, uv, mat), materials, textures).build_bvh(leaf, bins)


def scale_of(g, points):
    """M of the accuracy bound: per point, the largest absolute coordinate of the point and the scene (float64)."""
    lo, hi = bounds(g)
    return np.maximum(np.abs(np.asarray(points, np.float64)).max(axis=1), max(np.abs(lo).max(), np.abs(hi).max()))


def bounds(g):
    v = np.concatenate([g.v0, g.v0 + g.e1, g.v0 + g.e2])
    return v.min(axis=0), v.max(axis=0)


def surface_points(g, n, rng, offset=0.01):
    """Points within `offset` x the scene's extent of random points on random triangles."""
    lo, hi = bounds(g)
    prim = rng.integers(0, len(g.v0), n)
    b = rng.uniform(0, 1, (n, 2)).astype(np.float32)
    b = np.where(b.sum(axis=1, keepdims=True) > 1, 1 - b, b).astype(np.float32)
    on = g.v0[prim] + b[:, 0:1] * g.e1[prim] + b[:, 1:2] * g.e2[prim]
    return (on + rng.normal(size=(n, 3)) * offset * float((hi - lo).max()) / 3).astype(np.float32)


def tie_points(g, n, rng):
    """Exact ties: vertices and edge midpoints of random triangles (shared by the neighbours in a mesh)."""
    prim = rng.integers(0, len(g.v0), n)
    v = np.stack([g.v0[prim], g.v0[prim] + g.e1[prim], g.v0[prim] + g.e2[prim]], axis=1).astype(np.float32)
    k = rng.integers(0, 3, n)
    a, b = v[np.arange(n), k], v[np.arange(n), (k + 1) % 3]
    mid = ((a + b) * np.float32(0.5)).astype(np.float32)
    return np.where((rng.uniform(size=n) < 0.5)[:, None], a, mid).astype(np.float32)


def box_points(g, n, rng, scale=1.0):
    """Uniform in the scene's box scaled by `scale` about its centre."""
    lo, hi = bounds(g)
    c, h = (lo + hi) / 2, (hi - lo) / 2 * scale
    return (c + rng.uniform(-1, 1, (n, 3)) * h).astype(np.float32)


def point_sets(g, n, rng):
    """About n points: near surfaces, exact ties, in the scene's box, in a box ten times larger."""
    q = max(n // 4, 1)
    return np.concatenate([surface_points(g, q, rng), tie_points(g, q, rng), box_points(g, q, rng), box_points(g, q, rng, 10.0)]).astype(np.float32)
