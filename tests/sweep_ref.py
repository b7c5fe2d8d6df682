"""Restatement of the sphere cast (include/drt.h drt_renderer_sphere_cast) in float32 numpy, for the tests.  No tests of its own.

Every operation is one numpy operation in the arrays' dtype, in the order the header writes it (numpy rounds each one on its own; /
and np.sqrt are correctly rounded; np.fmin / np.fmax drop a NaN operand as fminf / fmaxf do).  Every branch of a shape is evaluated
and the header's conditions select.  The traversal is vectorised over casts as nearest_ref.nearest is over points, over the same
Geometry (nearest_ref.from_oracle / from_product / from_triangles).  In float64, brute_force over all triangles with no tree is the
yardstick of the accuracy tests.
"""
import collections

import numpy as np

from tests import nearest_ref as nr

SweepHits = collections.namedtuple("SweepHits", "t prim u v point feature")
MAX_STACK = 64
dot = nr.dot


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _edge(m, md, c, e, ee, d, r2, tmin, f, tt, feat):
    """drt.h "edges": the candidate of one edge folded into (tt, feat) on a strict <."""
    T = tt.dtype.type
    me, de = dot(m, e), dot(d, e)
    Cq = ee * c - me * me
    inside = Cq <= 0
    x = cross(d, e)
    det = dot(m, x)
    A, B = dot(x, x), ee * md - de * me
    disc = ee * (A * r2 - det * det)
    enter = ~inside & (A > 0) & (B < 0) & (disc >= 0)
    tau = np.where(enter, Cq / (np.sqrt(disc) - B), T(0))
    ax, t = me + tau * de, tmin + tau
    win = (inside | enter) & (ee > 0) & (ax >= 0) & (ax <= ee) & (t < tt)
    return np.where(win, t, tt), np.where(win, np.where(inside, f + 8, f), feat)


def _vertex(m, b, c, d, dd, r2, tmin, f, tt, feat):
    """drt.h "vertices"."""
    T = tt.dtype.type
    inside = c <= 0
    x = cross(m, d)
    disc = dd * r2 - dot(x, x)
    enter = ~inside & (dd > 0) & (b < 0) & (disc >= 0)
    tau = np.where(enter, c / (np.sqrt(disc) - b), T(0))
    t = tmin + tau
    win = (inside | enter) & (t < tt)
    return np.where(win, t, tt), np.where(win, np.where(inside, f + 8, f), feat)


def sweep_triangle(s, d, dd, r, r2, tmin, v0, e1, e2):
    """drt.h "per triangle" on (cast, triangle) pairs that broadcast, in the arrays' dtype: (t, feature), t = +inf and feature = -1
    where no shape is entered."""
    T = s.dtype.type
    with np.errstate(all="ignore"):
        d11, d22, d12 = dot(e1, e1), dot(e2, e2), dot(e1, e2)
        m0 = s - v0
        n = cross(e1, e2)
        k = r * np.sqrt(dot(n, n))
        h, dn = dot(n, m0), dot(n, d)
        ah = np.abs(h)
        inside = ah <= k
        ok = inside | ((h > 0) & (dn < 0)) | ((h < 0) & (dn > 0))
        tau = np.where(inside, T(0), (ah - k) / np.abs(dn))
        q = m0 + d * tau[..., None]
        q1, q2 = dot(q, e1), dot(q, e2)
        nu, nv, den = d22 * q1 - d12 * q2, d11 * q2 - d12 * q1, d11 * d22 - d12 * d12
        t = tmin + tau
        win = ok & (den > 0) & (nu >= 0) & (nv >= 0) & (nu + nv <= den) & (t < T(np.inf))
        tt = np.where(win, t, T(np.inf))
        feat = np.where(win, np.where(inside, 8, 0), -1)
        m1, m2 = s - (v0 + e1), s - (v0 + e2)
        b0, b1, b2 = dot(m0, d), dot(m1, d), dot(m2, d)
        c0, c1, c2 = dot(m0, m0) - r2, dot(m1, m1) - r2, dot(m2, m2) - r2
        e3 = e2 - e1
        tt, feat = _edge(m0, b0, c0, e1, d11, d, r2, tmin, 1, tt, feat)
        tt, feat = _edge(m0, b0, c0, e2, d22, d, r2, tmin, 2, tt, feat)
        tt, feat = _edge(m1, b1, c1, e3, dot(e3, e3), d, r2, tmin, 3, tt, feat)
        tt, feat = _vertex(m0, b0, c0, d, dd, r2, tmin, 4, tt, feat)
        tt, feat = _vertex(m1, b1, c1, d, dd, r2, tmin, 5, tt, feat)
        tt, feat = _vertex(m2, b2, c2, d, dd, r2, tmin, 6, tt, feat)
    return tt, feat


def contact_uv(cc, v0, e1, e2, f):
    """drt.h "result": (u, v) from the centre cc = o + d t by the feature f = feature & 7."""
    T = cc.dtype.type
    zero, one = T(0), T(1)
    with np.errstate(all="ignore"):
        q = cc - v0
        d11, d22, d12 = dot(e1, e1), dot(e2, e2), dot(e1, e2)
        q1, q2 = dot(q, e1), dot(q, e2)
        nu, nv, den = d22 * q1 - d12 * q2, d11 * q2 - d12 * q1, d11 * d22 - d12 * d12
        e3 = e2 - e1
        w1 = np.fmin(np.fmax(q1 / d11, zero), one)
        w2 = np.fmin(np.fmax(q2 / d22, zero), one)
        w3 = np.fmin(np.fmax(dot(q - e1, e3) / dot(e3, e3), zero), one)
        z, o = np.zeros_like(q1), np.ones_like(q1)
        u = np.select([f == 0, f == 1, f == 2, f == 3, f == 5], [nu / den, w1, z, one - w3, o], z)
        v = np.select([f == 0, f == 2, f == 3, f == 6], [nv / den, w2, w3, o], z)
    return u.astype(cc.dtype), v.astype(cc.dtype)


def inflated_slab(bmin, bmax, r, o, inv_dir, tmin, best):
    """drt.h "traversal": (visited, enter) of boxes [k, 3] against casts [k]."""
    with np.errstate(all="ignore"):
        t0 = ((bmin - r[:, None]) - o) * inv_dir
        t1 = ((bmax + r[:, None]) - o) * inv_dir
        lo, hi = np.fmin(t0, t1), np.fmax(t1, t0)
        enter = np.fmax(np.fmax(lo[:, 0], lo[:, 1]), lo[:, 2])
        exit_ = np.fmin(np.fmin(hi[:, 0], hi[:, 1]), hi[:, 2])
        return (enter <= exit_) & (exit_ >= tmin) & (enter <= best), enter


def _casts(org, dirs, radius, tmin, tmax, dtype=np.float32):
    o, d = np.ascontiguousarray(org, np.float32).astype(dtype), np.ascontiguousarray(dirs, np.float32).astype(dtype)
    n = len(o)
    r, t0, t1 = (np.broadcast_to(np.asarray(x, np.float32), n).astype(dtype) for x in (radius, tmin, tmax))
    return o, d, r, t0, t1


def _result(g, o, d, tmax, best, prim, feat):
    """The record of drt.h "result" from the winning (prim, feature, t)."""
    n = len(o)
    hit = prim >= 0
    k = np.where(hit, prim, 0)
    u, v, point = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
    if len(g.v0) and hit.any():
        with np.errstate(all="ignore"):
            cc = o + d * best[:, None]
            uu, vv = contact_uv(cc, g.v0[k], g.e1[k], g.e2[k], feat & 7)
            p = (g.v0[k] + g.e1[k] * uu[:, None]) + g.e2[k] * vv[:, None]
        u, v = np.where(hit, uu, np.float32(0)).astype(np.float32), np.where(hit, vv, np.float32(0)).astype(np.float32)
        point = np.where(hit[:, None], p, np.float32(0)).astype(np.float32)
    return SweepHits(np.where(hit, best, tmax).astype(np.float32), prim.astype(np.int32), u, v, point, np.where(hit, feat, -1).astype(np.int32))


def sphere_cast(g, org, dirs, radius=0.0, tmin=0.0, tmax=np.inf, visits=None):
    """drt.h "traversal" for casts org / dirs [n, 3] with radius, tmin, tmax scalars or [n].  visits: an int64 [n] array that
    receives the number of nodes each cast visited."""
    o, d, r, tmin, tmax = _casts(org, dirs, radius, tmin, tmax)
    n = len(o)
    best, prim, feat = tmax.copy(), np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    if len(g.bmin) == 0 or n == 0:
        return _result(g, o, d, tmax, best, prim, feat)
    with np.errstate(all="ignore"):
        inv_dir = (np.float32(1) / d).astype(np.float32)
        s = o + d * tmin[:, None]
        dd, r2 = dot(d, d), r * r
    root = len(g.bmin) - 1                                                     # the root is the last node
    st_node = np.zeros((n, MAX_STACK), np.int64)
    st_enter = np.zeros((n, MAX_STACK), np.float32)
    with np.errstate(invalid="ignore"):
        ok, enter = inflated_slab(g.bmin[root][None], g.bmax[root][None], r, o, inv_dir, tmin, best)
        ok &= (r >= 0) & ~np.isnan(o).any(axis=1) & ~np.isnan(d).any(axis=1)   # a negative or NaN radius, a NaN ray: nothing is visited
    st_node[:, 0], st_enter[:, 0] = root, enter
    sp = np.where(ok, 1, 0).astype(np.int64)
    while True:
        act = np.nonzero(sp > 0)[0]
        if len(act) == 0:
            break
        sp[act] -= 1
        node, enter = st_node[act, sp[act]], st_enter[act, sp[act]]
        keep = enter <= best[act]                                               # dropped unless enter <= best
        act, node = act[keep], node[keep]
        if visits is not None:
            visits[act] += 1
        leaf = g.is_leaf[node]
        la, ln = act[leaf], node[leaf]
        start, count = g.start[ln], g.count[ln]
        for k in range(int(count.max()) if len(ln) else 0):                    # a leaf's triangles in order
            sel = count > k
            q, t = la[sel], start[sel] + k
            tt, ff = sweep_triangle(s[q], d[q], dd[q], r[q], r2[q], tmin[q], g.v0[t], g.e1[t], g.e2[t])
            win = (tt < best[q]) | ((tt == best[q]) & (t < prim[q]))
            q, t = q[win], t[win]
            best[q], prim[q], feat[q] = tt[win], t, ff[win]
        ia, inode = act[~leaf], node[~leaf]
        if len(ia):
            c1, c2 = g.child1[inode], g.child2[inode]
            p1, en1 = inflated_slab(g.bmin[c1], g.bmax[c1], r[ia], o[ia], inv_dir[ia], tmin[ia], best[ia])
            p2, en2 = inflated_slab(g.bmin[c2], g.bmax[c2], r[ia], o[ia], inv_dir[ia], tmin[ia], best[ia])
            with np.errstate(invalid="ignore"):
                far1 = en1 > en2                                                # the farther child first
            for push, c, e in ((np.where(far1, p1, p2), np.where(far1, c1, c2), np.where(far1, en1, en2)),
                               (np.where(far1, p2, p1), np.where(far1, c2, c1), np.where(far1, en2, en1))):
                q = ia[push]
                st_node[q, sp[q]], st_enter[q, sp[q]] = c[push], e[push]
                sp[q] += 1
    return _result(g, o, d, tmax, best, prim, feat)


def brute_force(g, org, dirs, radius=0.0, tmin=0.0, tmax=np.inf, dtype=np.float32, chunk=256):
    """The per-triangle routine over ALL triangles in `dtype`, no tree: (t, prim, feature) under the (t, prim) rule, a miss is
    (tmax, -1, -1).  float32: the rule without the boxes.  float64: the yardstick."""
    o, d, r, tmin, tmax = _casts(org, dirs, radius, tmin, tmax, dtype)
    n = len(o)
    best, prim, feat = tmax.copy(), np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    v0, e1, e2 = (x.astype(dtype) for x in (g.v0, g.e1, g.e2))
    if len(v0) == 0 or n == 0:
        return best, prim, feat
    with np.errstate(all="ignore"):
        s = o + d * tmin[:, None]
        dd, r2 = dot(d, d), r * r
        for a in range(0, n, chunk):
            c = slice(a, a + chunk)
            tt, ff = sweep_triangle(s[c, None, :], d[c, None, :], dd[c, None], r[c, None], r2[c, None], tmin[c, None], v0[None], e1[None], e2[None])
            k = tt.argmin(axis=1)                                              # (the first of equal minima: the smallest index)
            rows = np.arange(len(k))
            m = tt[rows, k]
            win = (m < tmax[c]) & (r[c] >= 0)
            best[c], prim[c], feat[c] = np.where(win, m, tmax[c]), np.where(win, k, -1), np.where(win, ff[rows, k], -1)
    return best, prim, feat


# ---------------------------------------------------------------- float64 distances for the accuracy checks

def dist_to_triangle(g, pts, prim):
    """float64 distance from pts [n, 3] to triangle prim [n] each."""
    p = np.asarray(pts, np.float64)
    d2, *_ = nr.closest_on_triangle(p, g.v0[prim].astype(np.float64), g.e1[prim].astype(np.float64), g.e2[prim].astype(np.float64))
    return np.sqrt(d2)


def dist_to_mesh(g, pts, chunk=512):
    """float64 distance from pts [n, 3] to the whole mesh."""
    p = np.asarray(pts, np.float64)
    v0, e1, e2 = (x.astype(np.float64) for x in (g.v0, g.e1, g.e2))
    out = np.full(len(p), np.inf)
    for a in range(0, len(p), chunk):
        d2, *_ = nr.closest_on_triangle(p[a:a + chunk, None, :], v0[None], e1[None], e2[None])
        out[a:a + chunk] = np.sqrt(np.where(np.isnan(d2), np.inf, d2).min(axis=1))
    return out


# ---------------------------------------------------------------- cast sets shared by the CPU and GPU tests

def cast_sets(g, n, rng):
    """About n casts as (org, dirs, radius, tmin, tmax): aimed at surfaces, starting near surfaces, running parallel to faces, coming
    from far outside.  Radii are 0, about 1 %, 3 % and 10 % of the scene's extent; tmin is 0 or positive, tmax infinite or finite."""
    lo, hi = nr.bounds(g)
    ext = float((hi - lo).max())
    q = max(n // 4, 1)
    radius = (ext * rng.choice([0.0, 0.01, 0.03, 0.1], 4 * q) * rng.uniform(0.5, 1.0, 4 * q)).astype(np.float32)

    def on_surface(k):
        prim = rng.integers(0, len(g.v0), k)
        b = rng.uniform(0, 1, (k, 2)).astype(np.float32)
        b = np.where(b.sum(axis=1, keepdims=True) > 1, 1 - b, b).astype(np.float32)
        nrm = np.cross(g.e1[prim].astype(np.float64), g.e2[prim].astype(np.float64))
        nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
        return (g.v0[prim] + b[:, 0:1] * g.e1[prim] + b[:, 1:2] * g.e2[prim]).astype(np.float64), nrm, prim

    # aimed: from a point in 1.5 x the box towards a surface point, the target at t in 0.5 .. 2
    tgt, _, _ = on_surface(q)
    o0 = nr.box_points(g, q, rng, 1.5).astype(np.float64)
    d0 = (tgt - o0) * rng.uniform(0.5, 2.0, (q, 1))
    # near: from 0.5 .. 3 radii (at least 0.1 % of the extent) off a surface point, in a random direction
    tgt, nrm, _ = on_surface(q)
    off = np.maximum(radius[q:2 * q].astype(np.float64), 1e-3 * ext) * rng.uniform(0.5, 3.0, q)
    o1 = tgt + nrm * (off * rng.choice([-1.0, 1.0], q))[:, None]
    d1 = rng.normal(size=(q, 3)) * ext * rng.uniform(0.05, 1.0, (q, 1))
    # parallel: 0.9 .. 1.5 radii above a face, moving in its plane
    tgt, nrm, prim = on_surface(q)
    off = np.maximum(radius[2 * q:3 * q].astype(np.float64), 1e-3 * ext) * rng.uniform(0.9, 1.5, q)
    o2 = tgt + nrm * off[:, None]
    d2 = g.e1[prim] * rng.normal(size=(q, 1)) + g.e2[prim] * rng.normal(size=(q, 1))
    # far: from a box ten times larger towards a point of the scene's box
    o3 = nr.box_points(g, q, rng, 10.0).astype(np.float64)
    d3 = (nr.box_points(g, q, rng).astype(np.float64) - o3) * rng.uniform(0.5, 2.0, (q, 1))
    org = np.concatenate([o0, o1, o2, o3]).astype(np.float32)
    dirs = np.concatenate([d0, d1, d2, d3]).astype(np.float32)
    tmin = np.where(rng.uniform(size=4 * q) < 0.7, 0.0, rng.uniform(0, 0.3, 4 * q)).astype(np.float32)
    tmax = np.where(rng.uniform(size=4 * q) < 0.5, np.inf, rng.uniform(0.5, 3.0, 4 * q)).astype(np.float32)
    return org, dirs, radius, tmin, tmax


# ---------------------------------------------------------------- one triangle and one quad: hand-derived casts and seams

TRI = np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
QUAD = np.float32([[[0, 0, 0], [1, 0, 0], [1, 1, 0]], [[0, 0, 0], [1, 1, 0], [0, 1, 0]]])
DOWN = (0, 0, -1)

# (origin, direction, radius, t, feature, u, v, point) on the unit right triangle, tmin = 0.  All values are exact in float32.
# Entering cases: the face from above; each edge's cylinder where the face's prism and the vertex spheres are out of reach; each
# vertex's sphere from a (3, 4, 12) / 16 offset outside the triangle, where the cylinders entered earlier are cut by their axial range.
# Containment cases (+ 8): the centre starts inside the shape, t = tmin.
HAND = [
    ((0.25, 0.25, 1), DOWN, 0.25, 0.75, 0, 0.25, 0.25, (0.25, 0.25, 0)),
    ((0.5, -1, 0), (0, 1, 0), 0.25, 0.75, 1, 0.5, 0, (0.5, 0, 0)),
    ((-1, 0.5, 0), (1, 0, 0), 0.25, 0.75, 2, 0, 0.5, (0, 0.5, 0)),
    ((0.75, 0.75, 1), DOWN, 0.375, 0.875, 3, 0.5, 0.5, (0.5, 0.5, 0)),
    ((-0.1875, -0.25, 1.75), DOWN, 0.8125, 1.0, 4, 0, 0, (0, 0, 0)),
    ((1.1875, -0.25, 1.75), DOWN, 0.8125, 1.0, 5, 1, 0, (1, 0, 0)),
    ((-0.25, 1.1875, 1.75), DOWN, 0.8125, 1.0, 6, 0, 1, (0, 1, 0)),
    ((0.25, 0.25, 0.125), DOWN, 0.25, 0.0, 8, 0.25, 0.25, (0.25, 0.25, 0)),
    ((0.5, -0.125, 0), (0, 1, 0), 0.25, 0.0, 9, 0.5, 0, (0.5, 0, 0)),
    ((-0.125, 0.5, 0.125), (1, 0, 0), 0.25, 0.0, 10, 0, 0.5, (0, 0.5, 0)),
    ((0.625, 0.625, 0), DOWN, 0.25, 0.0, 11, 0.5, 0.5, (0.5, 0.5, 0)),
    ((-0.125, -0.125, 0), DOWN, 0.25, 0.0, 12, 0, 0, (0, 0, 0)),
    ((1.125, -0.0625, 0), DOWN, 0.25, 0.0, 13, 1, 0, (1, 0, 0)),
    ((-0.0625, 1.125, 0), DOWN, 0.25, 0.0, 14, 0, 1, (0, 1, 0)),
    ((0.25, 0.25, 1), DOWN, 0.0, 1.0, 0, 0.25, 0.25, (0.25, 0.25, 0)),        # radius 0: the ray
    ((0.25, 0.25, 0), DOWN, 0.0, 0.0, 8, 0.25, 0.25, (0.25, 0.25, 0)),        # radius 0, starting on the surface: a closed start
]


def seam_casts(r):
    """Targets on and within rounding of the quad's diagonal (face / face / edge), of its boundary (face / edge) and of its corners
    (edge / vertex), as (x, y) in the plane."""
    tiny = [0.0, 2.0 ** -24, -2.0 ** -24, 3e-7, -3e-7, r / 2, -r / 2, 0.9 * r, -0.9 * r]
    xy = [(x, x + dlt) for x in (0.125, 0.3, 0.5, 0.77, 1 / 3) for dlt in tiny]
    xy += [(x, -abs(dlt)) for x in (0.125, 0.3, 0.77) for dlt in tiny] + [(1 + abs(dlt), y) for y in (0.3, 0.6) for dlt in tiny]
    xy += [(dx, -abs(dy)) for dx in tiny for dy in tiny[:7]] + [(1 + dx, 1 + abs(dy)) for dx in tiny for dy in tiny[:7]]
    return np.float64(xy)
