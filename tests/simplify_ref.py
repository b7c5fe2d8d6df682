"""include/drt.h "mesh simplification" restated in numpy: vertex clustering on a grid with a mean or a quadric-optimal representative,
with the float32 / int64 / float64 arithmetic exactly as the header states it.  The device results are compared with this bit for bit
(tests/test_gpu_simplify.py); the restatement is checked on its own in tests/test_simplify_ref.py.  Nothing here looks at the device
code: the clusters are a unique() over the keys, the sums are np.add.at."""
import collections

import numpy as np

from tests import winding_ref as wr
from tests.weld_ref import exponent

F = np.float32
FLT_MAX = F(3.402823466e+38)
MEAN, QUADRIC = 0, 1
OUTSIDE = -1                      # the key of a vertex that is not in the grid

Simplified = collections.namedtuple("Simplified", "vertices faces first cluster source counts sums")


def _finite(a):
    with np.errstate(invalid="ignore"):
        return np.abs(a) <= FLT_MAX


def grid_of(lo, cell, dims):
    return np.asarray(lo, F).reshape(3), np.asarray(cell, F).reshape(3), np.asarray(dims, np.int64).reshape(3)


def keys_of(vertices, lo, cell, dims):
    """(int64 [V] the key ix + X (iy + Y iz) or OUTSIDE, int64 [V, 3] the cell indices): f = (p - lo) / cell, two fp32 operations; in
    the grid iff every coordinate is finite and 0 <= f < (float)dims on every axis; i = (int)f; nothing is clamped."""
    v = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    lo, cell, dims = grid_of(lo, cell, dims)
    with np.errstate(all="ignore"):
        f = ((v - lo).astype(F) / cell).astype(F)
        inside = _finite(v).all(axis=1) & ((f >= F(0)) & (f < dims.astype(F))).all(axis=1)
    idx = np.zeros((len(v), 3), np.int64)
    idx[inside] = f[inside].astype(np.int64)                                         # truncation
    key = np.where(inside, idx[:, 0] + dims[0] * (idx[:, 1] + dims[1] * idx[:, 2]), OUTSIDE)
    return key, idx


def clusters_of(key):
    """(int32 [V] the cluster id of every vertex, int32 [C] first): in-grid vertices of one key are one cluster, every other vertex is
    its own; first = the smallest member, clusters numbered in ascending first."""
    n = len(key)
    rep = np.arange(n, dtype=np.int64)
    inside = np.nonzero(key != OUTSIDE)[0]
    if len(inside):
        _, first, inverse = np.unique(key[inside], return_index=True, return_inverse=True)
        rep[inside] = inside[first][inverse.reshape(-1)]
    first = np.nonzero(rep == np.arange(n))[0]                                        # ascending
    rank = np.zeros(n, np.int64)
    rank[first] = np.arange(len(first))
    return rank[rep].astype(np.int32), first.astype(np.int32)


def _fixed30(x):
    """int64 trunc((double)x * 2^30) of float32 values"""
    with np.errstate(invalid="ignore"):
        return np.trunc(np.asarray(x, F).astype(np.float64) * np.ldexp(1.0, 30)).astype(np.int64)


def simplify(vertices, faces, lo, cell, dims, placement=QUADRIC, vertex_capacity=None, tri_capacity=None):
    """Simplified(vertices [min(C, cap)], faces [min(M, cap)], first, cluster [V], source, counts (C, M), sums) by the rule; sums is
    the int64 [C, 13] table of cnt, acc[3], A00 A01 A02 A11 A12 A22, b[3]."""
    v = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    lo, cell, dims = grid_of(lo, cell, dims)
    nv = len(v)
    key, idx = keys_of(v, lo, cell, dims)
    cluster, first = clusters_of(key)
    nc = len(first)
    inside = key != OUTSIDE
    cl = cluster.astype(np.int64)
    # the cell centre and r = (p - g) / cell of every in-grid vertex, fp32 with one rounding per operation
    with np.errstate(all="ignore"):
        g = (lo + ((idx.astype(F) + F(0.5)).astype(F) * cell).astype(F)).astype(F)
        r = np.where(inside[:, None], ((v - g).astype(F) / cell).astype(F), F(0))
    sums = np.zeros((nc, 13), np.int64)
    np.add.at(sums[:, 0], cl[inside], 1)
    np.add.at(sums[:, 1:4], cl[inside], _fixed30(r[inside]))
    cnt = sums[:, 0]
    if placement == QUADRIC and len(f):
        ok = ((f >= 0) & (f < nv)).all(axis=1)
        p = np.zeros((len(f), 3, 3), F)
        p[ok] = v[f[ok]]
        ok &= _finite(p).all(axis=(1, 2))
        with np.errstate(all="ignore"):
            n = wr.cross((p[:, 1] - p[:, 0]).astype(F), (p[:, 2] - p[:, 0]).astype(F)).astype(F)
            l = np.sqrt(wr.dot(n, n).astype(F)).astype(F)
            ok &= (l > 0) & _finite(l)
            if ok.any():
                e = exponent(l[ok].max())
                u = (n / l[:, None]).astype(F)
                w = (l.astype(np.float64) * np.ldexp(1.0, -(e + 1))).astype(F)        # the power of two in float64: exact; then fp32
                wu = (w[:, None] * u).astype(F)
                for k in range(3):
                    vk = np.where(ok, f[:, k], 0)
                    take = ok & inside[vk] & (cnt[cl[vk]] > 1)
                    rk = r[vk]
                    s = wr.dot(u, rk).astype(F)
                    terms = [(wu[:, i] * u[:, j]).astype(F) for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
                    terms += [(wu[:, i] * s).astype(F) for i in range(3)]
                    q = _fixed30(np.stack(terms, axis=1))
                    np.add.at(sums[:, 4:13], cl[vk[take]], q[take])
    # the finish, float64 with one rounding per operation
    out = v[first].copy()
    many = np.nonzero(cnt > 1)[0]
    if len(many):
        S = sums[many].astype(np.float64)
        with np.errstate(all="ignore"):
            m = S[:, 1:4] / (S[:, 0] * np.ldexp(1.0, 30))[:, None]
            x = m.copy()
            if placement == QUADRIC:
                A00, A01, A02, A11, A12, A22 = (S[:, 4 + i] for i in range(6))
                b0, b1, b2 = S[:, 10], S[:, 11], S[:, 12]
                tr = (A00 + A11) + A22
                lam = tr * np.ldexp(1.0, -10)
                a00, a11, a22, a01, a02, a12 = A00 + lam, A11 + lam, A22 + lam, A01, A02, A12
                d0, d1, d2 = b0 + lam * m[:, 0], b1 + lam * m[:, 1], b2 + lam * m[:, 2]
                c0 = a11 * a22 - a12 * a12
                c1 = a01 * a22 - a12 * a02
                c2 = a01 * a12 - a11 * a02
                det = (a00 * c0 - a01 * c1) + a02 * c2
                e0 = d1 * a22 - a12 * d2
                e1 = d1 * a12 - a11 * d2
                e2 = a01 * d2 - d1 * a02
                x0 = ((d0 * c0 - a01 * e0) + a02 * e1) / det
                x1 = ((a00 * e0 - d0 * c1) + a02 * e2) / det
                x2 = ((d0 * c2 - a00 * e1) - a01 * e2) / det
                q = np.stack([x0, x1, x2], axis=1)
                good = (tr != 0) & (np.abs(q) <= 0.5).all(axis=1)                       # (a NaN or an infinity fails the comparison)
                x = np.where(good[:, None], q, m)
            gm = g[first[many]].astype(np.float64)
            out[many] = (gm + x * cell.astype(np.float64)).astype(F)
    # the triangles
    ok = ((f >= 0) & (f < nv)).all(axis=1) if len(f) else np.zeros(0, bool)
    ids = np.zeros((len(f), 3), np.int32)
    ids[ok] = cluster[f[ok]]
    keep = ok & (ids[:, 0] != ids[:, 1]) & (ids[:, 1] != ids[:, 2]) & (ids[:, 2] != ids[:, 0])
    source = np.nonzero(keep)[0].astype(np.int32)
    out_faces = ids[keep]
    nm = len(source)
    vc = nc if vertex_capacity is None else min(nc, int(vertex_capacity))
    tc = nm if tri_capacity is None else min(nm, int(tri_capacity))
    return Simplified(out[:vc].copy(), out_faces[:tc].copy(), first[:vc].copy(), cluster, source[:tc].copy(), (nc, nm), sums)


def default_grid(vertices, resolution=None, cell=None):
    """The wrapper's default box, restated: lo = the smallest finite coordinate per axis; e = hi - lo in float64; with a resolution,
    cell = (float)(e (1 + 2^-16) / res) (1 where e = 0); with a cell, dims = max(1, ceil(e (1 + 2^-16) / cell))."""
    v = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    fin = v[_finite(v).all(axis=1)]
    if len(fin) == 0:
        lo, e = np.zeros(3, np.float64), np.zeros(3, np.float64)
    else:
        lo = fin.min(axis=0).astype(np.float64)
        e = fin.max(axis=0).astype(np.float64) - lo
    pad = e * (1.0 + 2.0 ** -16)
    if cell is None:
        dims = np.asarray(resolution, np.int64) * np.ones(3, np.int64)
        c = np.where(e > 0, pad / dims, 1.0).astype(F)
    else:
        c = np.full(3, cell, F)
        dims = np.maximum(1, np.ceil(pad / c.astype(np.float64))).astype(np.int64)
    return lo.astype(F), c, dims


# ---- what the tests measure on a result ----

def directed_edge_balance(faces):
    """True iff every directed edge (a, b) appears exactly as often as (b, a)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b = f.reshape(-1), np.roll(f, -1, axis=1).reshape(-1)
    n = int(max(a.max(initial=0), b.max(initial=0))) + 1
    fwd, fcount = np.unique(a * n + b, return_counts=True)
    bwd, bcount = np.unique(b * n + a, return_counts=True)
    return len(fwd) == len(bwd) and (fwd == bwd).all() and (fcount == bcount).all()


def volume(vertices, faces):
    """the signed volume of a closed mesh, float64"""
    p = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def sphere(rings=33, sectors=62, radius=0.8):
    """a closed latitude-longitude sphere: 2 sectors (rings - 1) triangles, outward"""
    v = [[0.0, 0.0, radius]]
    for i in range(1, rings):
        th = np.pi * i / rings
        for j in range(sectors):
            ph = 2 * np.pi * j / sectors
            v.append([radius * np.sin(th) * np.cos(ph), radius * np.sin(th) * np.sin(ph), radius * np.cos(th)])
    v.append([0.0, 0.0, -radius])
    south = len(v) - 1
    ring = lambda i, j: 1 + (i - 1) * sectors + j % sectors
    f = []
    for j in range(sectors):
        f.append([0, ring(1, j), ring(1, j + 1)])
        f.append([south, ring(rings - 1, j + 1), ring(rings - 1, j)])
    for i in range(1, rings - 1):
        for j in range(sectors):
            f.append([ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)])
            f.append([ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)])
    return np.asarray(v, F), np.asarray(f, np.int32)


def cube(n=16):
    """the unit cube [0, 1]^3 with n x n quads per side, 12 n^2 triangles, outward, shared vertices"""
    ids, v, f = {}, [], []

    def vid(p):
        if p not in ids:
            ids[p] = len(v)
            v.append([c / n for c in p])
        return ids[p]

    for axis in range(3):
        a, b = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    q = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0, 0, 0]
                        p[axis], p[a], p[b] = side, i + di, j + dj
                        q.append(vid(tuple(p)))
                    if side == 0:
                        q = q[::-1]
                    f.append([q[0], q[1], q[2]])
                    f.append([q[0], q[2], q[3]])
    return np.asarray(v, F), np.asarray(f, np.int32)
