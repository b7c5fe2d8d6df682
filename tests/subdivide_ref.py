"""include/drt.h "mesh subdivision" restated in numpy, independent of the device code: one level of midpoint or Loop subdivision of an
indexed mesh on the tables of tests/adjacency_ref.py.  The device results are compared with these byte for byte
(tests/test_gpu_subdivide.py); the restatement is checked against a plain dictionary-of-edges Loop and against the scheme's invariants
in tests/test_subdivide_ref.py."""
import numpy as np

from tests import adjacency_ref as ar

MIDPOINT, LOOP = 0, 1
NAN_WORD = 0x7FC00000


def shift(vertices):
    """k of the rule: 27 - floor(log2 M) with M the largest finite |coordinate| of float32 [V, 3]; 0 if M is 0"""
    with np.errstate(invalid="ignore"):                                        # (a signalling NaN is no error here)
        v = np.abs(np.asarray(vertices, np.float32).reshape(-1).astype(np.float64))
    v = v[np.isfinite(v)]
    m = float(v.max()) if len(v) else 0.0
    return 27 - (int(np.frexp(m)[1]) - 1) if m > 0 else 0


def fixed(x, k):
    """q(x) = (int64) trunc((double)x * 2^k) of finite float32 values"""
    return np.trunc(np.asarray(x, np.float32).astype(np.float64) * np.ldexp(1.0, k)).astype(np.int64)


def children(faces, edge, n_vertices):
    """int32 [4 N, 3]: (a, m0, m2), (b, m1, m0), (c, m2, m1), (m0, m1, m2) with m(h) = V + edge[h], or faces[h] where edge[h] < 0"""
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    e = np.asarray(edge, np.int32).reshape(-1, 3)
    m = np.where(e >= 0, (np.int64(n_vertices) + e).astype(np.int32), f)
    out = np.empty((len(f), 4, 3), np.int32)
    out[:, 0] = np.stack([f[:, 0], m[:, 0], m[:, 2]], axis=1)
    out[:, 1] = np.stack([f[:, 1], m[:, 1], m[:, 0]], axis=1)
    out[:, 2] = np.stack([f[:, 2], m[:, 2], m[:, 1]], axis=1)
    out[:, 3] = m
    return out.reshape(-1, 3)


def _gather(vertices, index):
    """(float64 [n, 3] positions with zeros where there is none, bool [n]: the index is inside [0, V) and the position is finite)"""
    index = np.asarray(index, np.int64)
    inside = (index >= 0) & (index < len(vertices))
    p = np.zeros((len(index), 3), np.float64)
    with np.errstate(invalid="ignore"):
        p[inside] = vertices[index[inside]].astype(np.float64)
    ok = inside.copy()
    ok[inside] = np.isfinite(vertices[index[inside]]).all(axis=1)
    p[~ok] = 0
    return p, ok


def subdivide(vertices, faces, scheme=LOOP, detail=None):
    """(vertices float32 [V + E, 3], faces int32 [4 N, 3], parents int32 [V + E, 2]) of one level.  detail: a dict that receives n_int,
    n_cr, k and the tables."""
    vertices = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    nv, nt = len(vertices), len(faces)
    adj, edge, half_edge = ar.by_index(faces)
    ne = len(half_edge)
    flat = faces.reshape(-1)
    h = half_edge.astype(np.int64)
    nxt = 3 * (h // 3) + (h % 3 + 1) % 3
    ia, ib = flat[h], flat[nxt]
    out_faces = children(faces, edge, nv)
    parents = np.empty((nv + ne, 2), np.int32)
    parents[:nv, 0] = parents[:nv, 1] = np.arange(nv, dtype=np.int32)
    parents[nv:, 0], parents[nv:, 1] = ia, ib
    out = np.empty((nv + ne, 3), np.float32)
    out[:nv] = vertices                                                        # (a copy of the bytes)
    pa, oka = _gather(vertices, ia)
    pb, okb = _gather(vertices, ib)
    usable = oka & okb
    odd = ((pa + pb) * 0.5).astype(np.float32)
    interior = np.zeros(ne, bool)
    n_int = n_cr = np.zeros(nv, np.int64)
    k = 0
    if scheme == LOOP and ne:
        twin = adj.reshape(-1)[h].astype(np.int64)
        interior = twin >= 0
        prv = 3 * (h // 3) + (h % 3 + 2) % 3                                  # the corner opposite h
        tw = np.where(interior, twin, 0)
        prv2 = 3 * (tw // 3) + (tw % 3 + 2) % 3                               # ... and opposite adj[h]
        pc, okc = _gather(vertices, flat[prv])
        pd, okd = _gather(vertices, flat[prv2])
        full = interior & okc & okd
        loop = ((pa + pb) * 0.375 + (pc + pd) * 0.125).astype(np.float32)
        odd = np.where(full[:, None], loop, odd)
        # the sums: one pass over the edges, int64
        k = shift(vertices)
        acc = np.zeros((2, nv, 3), np.int64)                                   # 0: interior, 1: crease
        cnt = np.zeros((2, nv), np.int64)
        u = np.flatnonzero(usable)
        kind = (~interior[u]).astype(np.int64)
        a, b = ia[u].astype(np.int64), ib[u].astype(np.int64)
        qa, qb = fixed(vertices[a], k), fixed(vertices[b], k)
        np.add.at(acc, (kind, a), qb)
        np.add.at(acc, (kind, b), qa)
        np.add.at(cnt, (kind, a), 1)
        np.add.at(cnt, (kind, b), 1)
        n_int, n_cr = cnt[0], cnt[1]
        inverse = np.ldexp(1.0, -k)
        with np.errstate(invalid="ignore"):
            p = vertices.astype(np.float64)
        s_int, s_cr = acc[0].astype(np.float64) * inverse, acc[1].astype(np.float64) * inverse
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            beta = np.where(n_int == 3, 0.1875, 0.375 / n_int.astype(np.float64))[:, None]
            smooth = (p + beta * (s_int - n_int.astype(np.float64)[:, None] * p)).astype(np.float32)
            crease = (p + 0.125 * (s_cr - 2.0 * p)).astype(np.float32)
        finite = np.isfinite(vertices).all(axis=1)
        take_smooth = finite & (n_cr == 0) & (n_int > 0)
        take_crease = finite & (n_cr == 2)
        out[:nv][take_smooth] = smooth[take_smooth]
        out[:nv][take_crease] = crease[take_crease]
    out[nv:] = odd
    out[nv:].view(np.uint32)[~usable] = NAN_WORD
    if detail is not None:
        detail.update(n_int=n_int, n_cr=n_cr, k=k, adj=adj, edge=edge, half_edge=half_edge, interior=interior, usable=usable)
    return out, out_faces, parents


def levels(vertices, faces, n, scheme=LOOP):
    """n levels: the restatement applied n times; parents is the last level's (None for n = 0)"""
    parents = None
    for _ in range(n):
        vertices, faces, parents = subdivide(vertices, faces, scheme)
    return vertices, faces, parents
