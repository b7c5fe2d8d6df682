"""include/drt.h "vertex welding, vertex normals and smoothing" restated in numpy: the three rules with the float32 / float64 / int64
arithmetic exactly as the header states it.  The device results are compared with these bit for bit (tests/test_gpu_weld.py); the
restatements are checked on their own in tests/test_weld_ref.py."""
import numpy as np

from tests import winding_ref as wr

F = np.float32
FLT_MAX = F(3.402823466e+38)
ANGLE, AREA = 0, 1


def corners(tris):
    """uint32 [3 N, 3]: the three words of every corner c = 3 t + k of [N, 3, 3] float32 or packed [N, 12] (drt_tri) triangles."""
    t = np.ascontiguousarray(tris, np.float32)
    if t.ndim == 2 and t.shape[1] == 12:
        t = np.ascontiguousarray(t[:, 0:9])
    return t.reshape(-1, 3).view(np.uint32)


def weld(tris, capacity=None):
    """(vertices float32 [min(V, capacity), 3], faces int32 [N, 3], first int32 [min(V, capacity)], V): corners with equal words are
    one vertex, rep = the smallest corner index of a position, vertices numbered in ascending rep."""
    w = corners(tris)
    n = len(w) // 3
    if n == 0:
        return np.zeros((0, 3), F), np.zeros((0, 3), np.int32), np.zeros(0, np.int32), 0
    keys = np.ascontiguousarray(w).view(np.dtype((np.void, 12))).reshape(-1)
    _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)      # first: the smallest index of each position
    order = np.argsort(first, kind="stable")                                          # ascending rep = first appearance
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    faces = rank[inverse.reshape(-1)].astype(np.int32).reshape(n, 3)
    first = first[order].astype(np.int32)
    v = len(first)
    cap = v if capacity is None else min(v, int(capacity))
    return w[first[:cap]].view(np.float32).copy(), faces, first[:cap].copy(), v


def exponent(m):
    """floor(log2 m) of a positive finite float32, denormals included."""
    return int(np.frexp(np.float64(m))[1]) - 1


def fixed(x, k):
    """int64 trunc((double)x * 2^k) of float32 values (the product is exact)."""
    with np.errstate(invalid="ignore"):           # (a value that is not finite belongs to a triangle that adds nothing)
        return np.trunc(np.asarray(x, F).astype(np.float64) * np.ldexp(1.0, int(k))).astype(np.int64)


def _finite(a):
    with np.errstate(invalid="ignore"):
        return np.abs(a) <= FLT_MAX


def _valid(vertices, faces):
    """(bool [N]: every index inside [0, V) and every coordinate finite, positions float32 [N, 3, 3] (zeros where invalid))"""
    v = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(axis=1)
    p = np.zeros((len(f), 3, 3), F)
    p[ok] = v[f[ok]]
    ok &= _finite(p).all(axis=(1, 2))
    return ok, f, p


def vertex_normals(vertices, faces, weight=ANGLE, sums=None):
    """float32 [V, 3] by the rule; sums: an int64 [V, 3] array that receives the fixed-point sums."""
    v = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    ok, f, p = _valid(v, faces)
    acc = np.zeros((len(v), 3), np.int64)
    with np.errstate(all="ignore"):
        n = wr.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).astype(F)
        l = np.sqrt(wr.dot(n, n)).astype(F)
        ok &= (l != 0) & _finite(l)
        if weight == AREA:
            m = np.abs(n[ok]).max() if ok.any() else F(0)
            if m > 0:
                q = fixed(n, 28 - exponent(m))
                for k in range(3):
                    np.add.at(acc, f[ok, k], q[ok])
        else:
            u = (n / l[:, None]).astype(F)
            for k in range(3):
                a, b = p[:, (k + 1) % 3] - p[:, k], p[:, (k + 2) % 3] - p[:, k]
                angle = wr.atan2(np.where(ok, l, F(1)), np.where(ok, wr.dot(a, b), F(1))).astype(F)
                take = ok & _finite(angle)
                q = fixed((angle[:, None] * u).astype(F), 28)
                np.add.at(acc, f[take, k], q[take])
    if sums is not None:
        sums[...] = acc
    x = acc.astype(np.float64)
    length = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])
    with np.errstate(all="ignore"):
        return np.where(length[:, None] > 0, x / np.where(length > 0, length, 1.0)[:, None], 0.0).astype(F)


def smooth_step(vertices, faces, factor, fixed_mask=None):
    """One step of the rule: float32 [V, 3]."""
    p = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    ok, f, tri = _valid(p, faces)
    fin = _finite(p)
    m = np.abs(p[fin]).max() if fin.any() else F(0)
    k = 27 - exponent(m) if m > 0 else 0
    acc, cnt = np.zeros((len(p), 3), np.int64), np.zeros(len(p), np.int64)
    q = fixed(tri, k)
    for a in range(3):
        np.add.at(acc, f[ok, a], q[ok, (a + 1) % 3] + q[ok, (a + 2) % 3])
        np.add.at(cnt, f[ok, a], 2)
    keep = (cnt == 0) | ~fin.all(axis=1)
    if fixed_mask is not None:
        keep |= np.asarray(fixed_mask).reshape(-1) != 0
    with np.errstate(all="ignore"):
        mean = acc.astype(np.float64) / (cnt.astype(np.float64) * np.ldexp(1.0, k))[:, None]
        pd = p.astype(np.float64)
        new = (pd + np.float64(F(factor)) * (mean - pd)).astype(F)
    out = p.copy()
    out[~keep] = new[~keep]
    return out


def smooth(vertices, faces, factors, fixed_mask=None):
    p = np.ascontiguousarray(vertices, F).reshape(-1, 3).copy()
    for f in factors:
        p = smooth_step(p, faces, f, fixed_mask)
    return p


def edges_of(faces):
    """(int64 [E, 2] the distinct undirected edges with different ends, int64 [E] how many half-edges run along each)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.stack([f, np.roll(f, -1, axis=1)], axis=-1).reshape(-1, 2)
    e = np.sort(e[e[:, 0] != e[:, 1]], axis=1)
    return np.unique(e, axis=0, return_counts=True)


def twins_of(faces):
    """int32 [N, 3]: drt_tri_edge_adjacency's table made from the index buffer by integers: the twin half-edge, -1 on a boundary edge,
    -2 where the edge is non-manifold, flipped or between one vertex and itself."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b = f.reshape(-1), np.roll(f, -1, axis=1).reshape(-1)
    adj = np.full(len(a), -2, np.int64)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    live = np.nonzero(a != b)[0]
    order = live[np.lexsort((hi[live], lo[live]))]
    key = np.stack([lo[order], hi[order]], axis=1)
    start = np.r_[0, np.nonzero((key[1:] != key[:-1]).any(axis=1))[0] + 1, len(order)]
    for s, e in zip(start[:-1], start[1:]):
        if e - s == 1:
            adj[order[s]] = -1
        elif e - s == 2 and a[order[s]] != a[order[s + 1]]:
            adj[order[s]], adj[order[s + 1]] = order[s + 1], order[s]
    return adj.astype(np.int32).reshape(-1, 3)
