"""Restatement of the triangle overlap query (include/drt.h drt_renderer_overlap_triangles) in float32 numpy over nearest_ref.Geometry,
for the tests.  No tests of its own.

Every operation is one float32 numpy operation, in the order the header writes it (numpy rounds each one on its own; np.fmin / np.fmax
drop a NaN operand as fminf / fmaxf do).  The node cull, the capacities, the segments and the pair sets are overlap_ref's, by import:
the header says they are the box query's.  The traversal is overlap_ref.overlap's with the triangle test in place of the box test and
the validity in front of the root.  brute_force is the same triangle test over ALL triangles, with no cull.
"""
import numpy as np

from tests import nearest_ref as nr
from tests.overlap_ref import ANY, LIST, _max3, _min3, _segments, caps_of, cull_passes, pair_sets  # noqa: F401  (re-exported)

FLT_MAX = np.finfo(np.float32).max


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def pack(tris):
    """drt_tri records [N, 12] float32 from [N, 3, 3] vertices: v[3][3], pad 0."""
    t = _f32(tris).reshape(-1, 9)
    out = np.zeros((len(t), 12), np.float32)
    out[:, :9] = t
    return out


def unpack(tris):
    """[N, 3, 3] vertices of [N, 12] records or of [N, 3, 3] itself."""
    t = _f32(tris)
    if t.ndim == 2 and t.shape[1] == 12:
        return _f32(t[:, :9]).reshape(-1, 3, 3)
    return t.reshape(-1, 3, 3)


def valid(q):
    """drt.h "validity": all nine coordinates satisfy fabsf(x) <= FLT_MAX."""
    with np.errstate(invalid="ignore"):
        return (np.abs(q) <= FLT_MAX).all(axis=(-1, -2))


def bounds_of(q):
    """drt.h "bounds": qmin[j] = min3(q0[j], q1[j], q2[j]), qmax likewise."""
    return _min3(q[..., 0, :], q[..., 1, :], q[..., 2, :]), _max3(q[..., 0, :], q[..., 1, :], q[..., 2, :])


def cross(a, b):
    """(a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x)"""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def triangle_axes(q0, q1, q2, v0, e1, e2):
    """drt.h "triangle test" on (query, triangle) pairs (broadcast over the leading dimensions): bool [..., 17], ok of the seventeen
    axes in the header's order."""
    with np.errstate(all="ignore"):
        a1, a2 = q1 - q0, q2 - q0
        g = a2 - a1
        h = e2 - e1
        p0 = v0 - q0
        p1, p2 = p0 + e1, p0 + e2
        nq, nt = cross(a1, a2), cross(e1, e2)
        A, E = (a1, g, a2), (e1, h, e2)
        axes = [nq, nt] + [cross(a, e) for a in A for e in E] + [cross(nq, a) for a in A] + [cross(nt, e) for e in E]
        ok = []
        for L in axes:
            s1, s2 = nr.dot(L, a1), nr.dot(L, a2)
            t0, t1, t2 = nr.dot(L, p0), nr.dot(L, p1), nr.dot(L, p2)
            zero = np.zeros_like(s1)
            ok.append((_min3(t0, t1, t2) <= _max3(zero, s1, s2)) & (_min3(zero, s1, s2) <= _max3(t0, t1, t2)))
        return np.stack(np.broadcast_arrays(*ok), axis=-1)


def triangle_listed(q0, q1, q2, v0, e1, e2):
    return triangle_axes(q0, q1, q2, v0, e1, e2).all(axis=-1)


def overlap(g, tris, caps, mode=LIST, visits=None, events=None):
    """drt.h "traversal" for queries [N, 3, 3] (or packed [N, 12]) with caps a scalar or [N] (already clamped: caps_of): (prims int32
    of sum(caps) slots, query i's at [cumsum(caps)[i-1], cumsum(caps)[i]); counts uint32 [N]).  Mode ANY: no slots (caps is ignored),
    counts 0 or 1.  visits and events as overlap_ref.overlap's."""
    q = unpack(tris)
    n = len(q)
    qmin, qmax = bounds_of(q)
    found_q, found_prim = [], []
    if len(g.bmin) and n:
        root = len(g.bmin) - 1                                                 # the root is the last node
        st = np.zeros((n, nr.MAX_STACK), np.int64)
        st[:, 0] = root
        # an invalid query pushes nothing; the root is tested against the root box
        sp = (valid(q) & cull_passes(qmin, qmax, g.bmin[root], g.bmax[root])).astype(np.int64)
        while True:
            act = np.nonzero(sp > 0)[0]
            if len(act) == 0:
                break
            sp[act] -= 1
            node = st[act, sp[act]]
            if visits is not None:
                visits[act] += 1
            leaf = g.is_leaf[node]
            la, ln = act[leaf], node[leaf]
            start, count = g.start[ln], g.count[ln]
            done = np.zeros(len(la), bool)                                     # mode ANY: the query has its triangle
            for k in range(int(count.max()) if len(ln) else 0):                # a leaf's triangles in order
                sel = (count > k) & ~done
                r, t = la[sel], start[sel] + k
                listed = triangle_listed(q[r, 0], q[r, 1], q[r, 2], g.v0[t], g.e1[t], g.e2[t])
                found_q.append(r[listed])
                found_prim.append(t[listed])
                if mode == ANY:
                    done[np.nonzero(sel)[0][listed]] = True
                    sp[r[listed]] = 0                                          # the traversal ends at the first listed triangle
            ia, inode = act[~leaf], node[~leaf]
            if len(ia):
                c1, c2 = g.child1[inode], g.child2[inode]
                for child in (c2, c1):                                         # child 2 first
                    push = cull_passes(qmin[ia], qmax[ia], g.bmin[child], g.bmax[child])
                    r = ia[push]
                    st[r, sp[r]] = child[push]
                    sp[r] += 1
    pb = np.concatenate(found_q) if found_q else np.zeros(0, np.int64)
    pp = np.concatenate(found_prim) if found_prim else np.zeros(0, np.int64)
    if mode == ANY:
        return np.zeros(0, np.int32), np.bincount(pb, minlength=n).astype(np.uint32)
    return _segments(pb, pp, n, caps, events)


def brute_force(g, tris, caps, mode=LIST, chunk=64):
    """The triangle test of every valid query over ALL triangles, with no cull: (prims, counts) as overlap's."""
    q = unpack(tris)
    n, T = len(q), len(g.v0)
    ok = valid(q)
    found_q, found_prim = [], []
    for s in range(0, n if T else 0, chunk):
        e = slice(s, s + chunk)
        listed = triangle_listed(q[e, None, 0], q[e, None, 1], q[e, None, 2], g.v0[None], g.e1[None], g.e2[None]) & ok[e, None]
        i, t = np.nonzero(listed)
        found_q.append(i + s)
        found_prim.append(t)
    pb = np.concatenate(found_q) if found_q else np.zeros(0, np.int64)
    pp = np.concatenate(found_prim) if found_prim else np.zeros(0, np.int64)
    if mode == ANY:
        return np.zeros(0, np.int32), np.minimum(np.bincount(pb, minlength=n), 1).astype(np.uint32)
    return _segments(pb, pp, n, caps)


def scene_triangles(g):
    """The scene's own triangles as queries [T, 3, 3], in tree order: (v0, v0 + e1, v0 + e2) of the stored records."""
    return np.stack([g.v0, g.v0 + g.e1, g.v0 + g.e2], axis=1).astype(np.float32)


def self_pairs(g, tris):
    """Renderer.selfIntersections in numpy: pairs i < j of triangle indices whose query i lists triangle j and that share no vertex
    position (bit-equal coordinates), int32 [P, 2] in (i, j) order.  tris: the scene's real vertices [T, 3, 3] in tree order (not
    scene_triangles(g): v0 + e1 can differ from the real v1 by an ulp, and a neighbour's vertex would no longer be bit-equal)."""
    q = unpack(tris)
    _, totals = overlap(g, q, 0)
    prims, _ = overlap(g, q, totals)
    i = np.repeat(np.arange(len(q), dtype=np.int64), totals.astype(np.int64))
    j = prims.astype(np.int64)
    keep = j > i
    i, j = i[keep], j[keep]
    shared = (q[i][:, :, None, :].view(np.uint32) == q[j][:, None, :, :].view(np.uint32)).all(axis=-1).any(axis=(1, 2))
    return np.stack([i[~shared], j[~shared]], axis=1).astype(np.int32)
