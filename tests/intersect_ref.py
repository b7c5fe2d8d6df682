"""Restatement of the triangle intersection segments (include/drt.h drt_renderer_intersect_triangles) in float32 numpy over
nearest_ref.Geometry, for the tests.  No tests of its own.

Every operation is one float32 numpy operation, in the order the header writes it (numpy rounds each one on its own).  The validity,
the bounds, the node cull, the capacities and the order of the lists are tri_overlap_ref's and overlap_ref's, by import: the header
says they are the triangle overlap query's.  The traversal is tri_overlap_ref.overlap's with the segment rule in place of the
predicate.  brute_force is the same rule over ALL triangles, with no cull.
"""
import numpy as np

from tests import nearest_ref as nr
from tests.overlap_ref import _segments, caps_of, cull_passes  # noqa: F401  (re-exported)
from tests.tri_overlap_ref import bounds_of, cross, pack, scene_triangles, unpack, valid  # noqa: F401  (re-exported)

MISS = np.zeros(8, np.float32)
MISS.view(np.int32)[3] = -1                                                   # the miss record: all zeros with prim = -1


def is_miss(rec):
    """bool per record of [..., 8]: the miss record, word for word (prim = -1 is a NaN as a float: == on the floats would fail)."""
    return (np.ascontiguousarray(rec).view(np.int32) == MISS.view(np.int32)).all(axis=-1)


def _pick(c, a, b):
    """c ? a : b on points [..., 3] with c [...]"""
    return np.where(c[..., None], a, b)


def _cut(lo, s_lo, hi, s_hi):
    """drt.h "cut points": t = s_lo / (s_lo - s_hi), lo + (hi - lo) * t per component."""
    t = s_lo / (s_lo - s_hi)
    return lo + (hi - lo) * t[..., None]


def _apex_cuts(w, s):
    """The two cut points of a triangle with world vertices w = (w0, w1, w2) and signed values s = (s0, s1, s2) whose classes are not
    all the same: apex k alone in its class, (X1 = cut(k, k+1), edge k, X2 = cut(k, k+2), edge (k+2) % 3).  Where the classes are all
    the same the values mean nothing."""
    a0, a1, a2 = s[0] >= 0, s[1] >= 0, s[2] >= 0
    k = np.where(a1 == a2, 0, np.where(a0 == a2, 1, 2))
    k0, k1 = k == 0, k == 1
    vk, va, vb = _pick(k0, w[0], _pick(k1, w[1], w[2])), _pick(k0, w[1], _pick(k1, w[2], w[0])), _pick(k0, w[2], _pick(k1, w[0], w[1]))
    sk, sa, sb = np.where(k0, s[0], np.where(k1, s[1], s[2])), np.where(k0, s[1], np.where(k1, s[2], s[0])), np.where(k0, s[2], np.where(k1, s[0], s[1]))
    above = sk >= 0
    # lo is the below one of the two and hi the above one: the apex is hi when it is above
    x1 = _cut(_pick(above, va, vk), np.where(above, sa, sk), _pick(above, vk, va), np.where(above, sk, sa))
    x2 = _cut(_pick(above, vb, vk), np.where(above, sb, sk), _pick(above, vk, vb), np.where(above, sk, sb))
    return x1, k, x2, (k + 2) % 3


def segment(q0, q1, q2, v0, e1, e2):
    """drt.h "signed values" to "record" on (query, triangle) pairs (broadcast over the leading dimensions): (has bool [...],
    p [..., 3], q [..., 3] float32, code int32 [...]).  Where has is false the other three mean nothing."""
    with np.errstate(all="ignore"):
        q0, q1, q2, v0, e1, e2 = np.broadcast_arrays(q0, q1, q2, v0, e1, e2)
        w0, w1, w2 = v0, v0 + e1, v0 + e2
        # the scene triangle against the query's plane
        a1, a2 = q1 - q0, q2 - q0
        nq = cross(a1, a2)
        s = [nr.dot(nq, w - q0) for w in (w0, w1, w2)]
        has = ~((s[0] >= 0) == (s[1] >= 0)) | ~((s[1] >= 0) == (s[2] >= 0))
        # the query against the scene triangle's plane
        nt = cross(e1, e2)
        u = [nr.dot(nt, q - v0) for q in (q0, q1, q2)]
        has &= ~((u[0] >= 0) == (u[1] >= 0)) | ~((u[1] >= 0) == (u[2] >= 0))
        # line direction and its axis
        D = cross(nq, nt)
        aD = np.abs(D)
        j = np.where(aD[..., 1] > aD[..., 0], 1, 0)
        j = np.where(aD[..., 2] > np.take_along_axis(aD, j[..., None], -1)[..., 0], 2, j)
        Dj = np.take_along_axis(D, j[..., None], -1)[..., 0]
        has &= np.abs(Dj) > 0
        # cut points: the scene's on its edges 0..2, the query's on 4 + its edges
        T1, c1, T2, c2 = _apex_cuts((w0, w1, w2), s)
        Q1, d1, Q2, d2 = _apex_cuts((q0, q1, q2), u)
        d1, d2 = d1 + 4, d2 + 4
        on = lambda P: np.take_along_axis(P, j[..., None], -1)[..., 0]
        # intervals on axis j
        first = on(T1) <= on(T2)
        tl, ctl, th, cth = _pick(first, T1, T2), np.where(first, c1, c2), _pick(first, T2, T1), np.where(first, c2, c1)
        first = on(Q1) <= on(Q2)
        ql, cql, qh, cqh = _pick(first, Q1, Q2), np.where(first, d1, d2), _pick(first, Q2, Q1), np.where(first, d2, d1)
        use = on(ql) > on(tl)                                                 # on a tie the scene's point is kept
        lo, clo = _pick(use, ql, tl), np.where(use, cql, ctl)
        use = on(qh) < on(th)
        hi, chi = _pick(use, qh, th), np.where(use, cqh, cth)
        has &= on(lo) <= on(hi)                                               # touching counts; a NaN fails
        # orientation: along cross(nq, nt)
        fwd = Dj > 0
        p, cp, q, cq = _pick(fwd, lo, hi), np.where(fwd, clo, chi), _pick(fwd, hi, lo), np.where(fwd, chi, clo)
        return has, p.astype(np.float32), q.astype(np.float32), (cp + 16 * cq).astype(np.int32)


def _records(fq, fp, P, Q, code, n, caps):
    """The flat records float32 [sum(caps), 8] (p, prim, q, code; the miss record in unused slots) and counts uint32 [n] from the found
    (query, prim) pairs in any order: overlap_ref._segments gives the slots, the records follow their prims."""
    prims, counts = _segments(fq, fp, n, caps)
    caps = np.broadcast_to(np.asarray(caps, np.int64), n)
    rec = np.tile(MISS, (len(prims), 1))
    if len(fq):
        key = fq * (1 << 32) + fp
        order = np.argsort(key)
        owner = np.repeat(np.arange(n, dtype=np.int64), caps)
        used = np.nonzero(prims >= 0)[0]
        at = order[np.searchsorted(key[order], owner[used] * (1 << 32) + prims[used])]
        rec[used, 0:3], rec[used, 4:7] = P[at], Q[at]
        rec.view(np.int32)[used, 3], rec.view(np.int32)[used, 7] = fp[at], code[at]
    return rec, counts


def _gather(found):
    if not found:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.int32)
    return tuple(np.concatenate(x) for x in zip(*found))


def intersect(g, tris, caps):
    """drt.h "traversal" for queries [N, 3, 3] (or packed [N, 12]) with caps a scalar or [N] (already clamped: caps_of): (records
    float32 [sum(caps), 8], query i's at [cumsum(caps)[i-1], cumsum(caps)[i]); counts uint32 [N])."""
    q = unpack(tris)
    n = len(q)
    qmin, qmax = bounds_of(q)
    found = []
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
            leaf = g.is_leaf[node]
            la, ln = act[leaf], node[leaf]
            start, count = g.start[ln], g.count[ln]
            for k in range(int(count.max()) if len(ln) else 0):                # a leaf's triangles in order
                sel = count > k
                r, t = la[sel], start[sel] + k
                has, P, Q, code = segment(q[r, 0], q[r, 1], q[r, 2], g.v0[t], g.e1[t], g.e2[t])
                found.append((r[has], t[has], P[has], Q[has], code[has]))
            ia, inode = act[~leaf], node[~leaf]
            if len(ia):
                c1, c2 = g.child1[inode], g.child2[inode]
                for child in (c2, c1):                                         # child 2 first
                    push = cull_passes(qmin[ia], qmax[ia], g.bmin[child], g.bmax[child])
                    r = ia[push]
                    st[r, sp[r]] = child[push]
                    sp[r] += 1
    return _records(*_gather(found), n, caps)


def brute_force(g, tris, caps, chunk=64):
    """The rule of every valid query over ALL triangles, with no cull: (records, counts) as intersect's."""
    q = unpack(tris)
    n, T = len(q), len(g.v0)
    ok = valid(q)
    found = []
    for s in range(0, n if T else 0, chunk):
        e = slice(s, s + chunk)
        has, P, Q, code = segment(q[e, None, 0], q[e, None, 1], q[e, None, 2], g.v0[None], g.e1[None], g.e2[None])
        has &= ok[e, None]
        i, t = np.nonzero(has)
        found.append((i + s, t, P[has], Q[has], code[has]))
    return _records(*_gather(found), n, caps)


def whole(g, tris):
    """Every record of every query: (splits int64 [N + 1], records [M, 8]) -- a count, the scan, a fill."""
    _, totals = intersect(g, tris, 0)
    rec, _ = intersect(g, tris, totals)
    return np.concatenate([[0], np.cumsum(totals.astype(np.int64))]), rec


def self_cuts(g, tris):
    """Renderer.selfIntersectionSegments in numpy: the records of the pairs i < j that share no vertex position (bit-equal
    coordinates), in (i, j) order: (pairs int32 [P, 2], p, q float32 [P, 3], code int32 [P]).  tris: the scene's real vertices
    [T, 3, 3] in tree order, as tri_overlap_ref.self_pairs takes them."""
    q = unpack(tris)
    splits, rec = whole(g, q)
    i = np.repeat(np.arange(len(q), dtype=np.int64), np.diff(splits))
    j = rec.view(np.int32)[:, 3].astype(np.int64)
    keep = j > i
    shared = (q[i][:, :, None, :].view(np.uint32) == q[j][:, None, :, :].view(np.uint32)).all(axis=-1).any(axis=(1, 2))
    keep &= ~shared
    return np.stack([i[keep], j[keep]], axis=1).astype(np.int32), rec[keep, 0:3], rec[keep, 4:7], rec.view(np.int32)[keep, 7]
