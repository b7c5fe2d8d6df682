"""Restatement of the nearest-triangle lists (include/drt.h drt_renderer_nearest_list) in float32 numpy over nearest_ref.Geometry, for
the tests.  No tests of its own.

The per-triangle and per-box arithmetic is nearest_ref's (closest_on_triangle, box_dist2), so d2, u and v have the nearest query's
bits.  The traversal is nearest_ref.nearest's, vectorised over points in the same way -- every step pops one stack entry of every
point that still has one -- with the header's search bound in place of `best`, and with each point's list held as a row of [n, cap]
arrays kept in the rule's order (ascending d2, equal d2 by ascending prim).  brute_force is the same rule without the tree: all
triangles, sorted.
"""
import collections

import numpy as np

from tests import nearest_ref as nr

GATHER, K = 0, 1                                                          # drt.h DRT_NEAR_GATHER, DRT_NEAR_K
Slots = collections.namedtuple("Slots", "d2 prim u v point side")       # one entry per slot of every point's segment, point after point
F0, F1 = np.float32(0), np.float32(1)
_FREE_PRIM = np.int64(2) ** 62                                            # key of a free slot: behind every record


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def radius2(n, max_dist):
    """r2 = max_dist * max_dist, the point's own product."""
    md = _f32(np.broadcast_to(np.float32(max_dist) if np.isscalar(max_dist) else max_dist, n))
    with np.errstate(all="ignore"):
        return (md * md).astype(np.float32)


def caps_of(offsets, capacity):
    """drt.h "segments": cap_i = offsets[i+1] > offsets[i] ? the difference : 0, clamped so that offsets[i] + cap_i <= capacity."""
    o = np.asarray(offsets, np.int64)
    cap = np.where(o[1:] > o[:-1], o[1:] - o[:-1], 0)
    return np.minimum(cap, np.clip(capacity - o[:-1], 0, None))


def comes_before(d2a, prima, d2b, primb):
    return (d2a < d2b) | ((d2a == d2b) & (prima < primb))


class _Lists:
    """Every point's list as a row: the first stored[i] entries of row i, in order; free slots carry the key (+inf, 2^62)."""

    def __init__(self, n, caps):
        self.caps = caps
        width = int(caps.max()) if n else 0
        self.d2 = np.full((n, width), np.inf, np.float32)
        self.prim = np.full((n, width), _FREE_PRIM, np.int64)
        self.u, self.v = np.zeros((n, width), np.float32), np.zeros((n, width), np.float32)
        self.stored, self.total = np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.out_of_order, self.evicted = np.zeros(n, bool), np.zeros(n, bool)   # what the inputs made the insert do

    def full(self, r):
        return self.stored[r] == self.caps[r]

    def tail_d2(self, r):
        """d2 of the last slot of the segment (meaningful where full and cap > 0)."""
        if self.d2.shape[1] == 0:
            return np.zeros(len(r), np.float32)
        return self.d2[r, np.maximum(self.caps[r] - 1, 0)]

    def insert(self, r, d2, prim, u, v):
        """One listed candidate for each of the (distinct) points r."""
        self.total[r] += 1
        cap = self.caps[r]
        if self.d2.shape[1] == 0:
            return
        last = np.maximum(cap - 1, 0)
        full = self.stored[r] == cap
        ok = (cap > 0) & ~(full & ~comes_before(d2, prim, self.d2[r, last], self.prim[r, last]))
        r, d2, prim, u, v, full, last = r[ok], d2[ok], prim[ok], u[ok], v[ok], full[ok], last[ok]
        j = np.where(full, last, self.stored[r])                               # the slot that opens
        self.evicted[r] |= full
        prev = np.maximum(j - 1, 0)
        self.out_of_order[r] |= (j > 0) & comes_before(d2, prim, self.d2[r, prev], self.prim[r, prev])
        self.d2[r, j], self.prim[r, j], self.u[r, j], self.v[r, j] = d2, prim, u, v
        self.stored[r] = np.where(full, self.stored[r], self.stored[r] + 1)
        order = np.lexsort((self.prim[r], self.d2[r]), axis=1)                 # by d2, then prim; free slots stay behind
        rows = r[:, None]
        for f in (self.d2, self.prim, self.u, self.v):
            f[rows, np.arange(f.shape[1])[None, :]] = f[rows, order]


def _slots(g, p, r2, caps, lists):
    """drt.h "segments" and "surf": the flat records, miss records behind each list."""
    n = len(p)
    base = np.concatenate([[0], np.cumsum(caps)])
    m = int(base[-1])
    d2, prim = np.repeat(r2, caps), np.full(m, -1, np.int32)                   # the miss record {r2, -1, 0, 0}
    u, v = np.zeros(m, np.float32), np.zeros(m, np.float32)
    point, side = np.zeros((m, 3), np.float32), np.zeros(m, np.float32)
    i, j = np.nonzero(np.arange(lists.d2.shape[1])[None, :] < lists.stored[:, None])
    dest = base[i] + j
    k = lists.prim[i, j]
    d2[dest], prim[dest], u[dest], v[dest] = lists.d2[i, j], k, lists.u[i, j], lists.v[i, j]
    if len(dest):
        with np.errstate(all="ignore"):
            c = (g.v0[k] + g.e1[k] * u[dest][:, None]) + g.e2[k] * v[dest][:, None]
            point[dest] = c
            side[dest] = np.where(nr.dot(p[i] - c, g.fn[k]) < 0, np.float32(-1), F1)
    return Slots(_f32(d2), prim, u, v, point, side)


def near_list(g, points, max_dist, caps, mode, visits=None, events=None):
    """drt.h "traversal" for points [n, 3] with max_dist a scalar or [n] and caps a scalar or [n] (already clamped: caps_of):
    (Slots of sum(caps) entries, point i's at [cumsum(caps)[i-1], cumsum(caps)[i]); counts uint32 [n]).  visits: an int64 [n] array
    that receives the number of nodes each point visited (popped and kept).  events: a dict that receives "out_of_order" and
    "evicted", bool [n]: the point had a candidate inserted before a stored record / into a full list."""
    p = _f32(points).reshape(-1, 3)
    n = len(p)
    caps = np.broadcast_to(np.asarray(caps, np.int64), n).copy()
    r2 = radius2(n, max_dist)
    L = _Lists(n, caps)
    k_mode = mode == K

    def keep(r, box2):
        """drt.h "search bound"."""
        with np.errstate(invalid="ignore"):
            return np.where(L.full(r), box2 <= L.tail_d2(r), box2 < r2[r]) if k_mode else box2 < r2[r]

    if len(g.bmin) and n:
        root = len(g.bmin) - 1                                                 # the root is the last node
        st_node = np.zeros((n, nr.MAX_STACK), np.int64)
        st_box2 = np.zeros((n, nr.MAX_STACK), np.float32)
        st_node[:, 0] = root
        st_box2[:, 0] = nr.box_dist2(g.bmin[root], g.bmax[root], p)
        sp = np.where(caps == 0, 0, 1) if k_mode else np.ones(n, np.int64)     # mode K with cap 0 visits nothing
        while True:
            act = np.nonzero(sp > 0)[0]
            if len(act) == 0:
                break
            sp[act] -= 1
            node, box2 = st_node[act, sp[act]], st_box2[act, sp[act]]
            kept = keep(act, box2)                                             # dropped unless keep
            act, node = act[kept], node[kept]
            if visits is not None:
                visits[act] += 1
            leaf = g.is_leaf[node]
            la, ln = act[leaf], node[leaf]
            start, count = g.start[ln], g.count[ln]
            for k in range(int(count.max()) if len(ln) else 0):                # a leaf's triangles in order
                sel = count > k
                r, t = la[sel], start[sel] + k
                d2, u, v, _ = nr.closest_on_triangle(p[r], g.v0[t], g.e1[t], g.e2[t])
                with np.errstate(invalid="ignore"):
                    listed = d2 < r2[r]                                        # NaN is never listed
                L.insert(r[listed], d2[listed], t[listed], u[listed], v[listed])
            ia, inode = act[~leaf], node[~leaf]
            if len(ia):
                c1, c2 = g.child1[inode], g.child2[inode]
                b1, b2 = nr.box_dist2(g.bmin[c1], g.bmax[c1], p[ia]), nr.box_dist2(g.bmin[c2], g.bmax[c2], p[ia])
                p1, p2 = keep(ia, b1), keep(ia, b2)
                far1 = b1 > b2                                                  # the farther child first
                for push, c, d in ((np.where(far1, p1, p2), np.where(far1, c1, c2), np.where(far1, b1, b2)),
                                   (np.where(far1, p2, p1), np.where(far1, c2, c1), np.where(far1, b2, b1))):
                    r = ia[push]
                    st_node[r, sp[r]], st_box2[r, sp[r]] = c[push], d[push]
                    sp[r] += 1
    if events is not None:
        events["out_of_order"], events["evicted"] = L.out_of_order, L.evicted
    return _slots(g, p, r2, caps, L), (L.stored if k_mode else L.total).astype(np.uint32)


def brute_force(g, points, max_dist, caps, mode, chunk=128):
    """The rule without the tree, in float32: every triangle with dist2 < r2, sorted by (d2, prim), the first cap stored.  counts: the
    total (GATHER) or min(cap, total) (K).  Also returns tied, bool [n]: two of the point's listed triangles have the same d2."""
    p = _f32(points).reshape(-1, 3)
    n, T = len(p), len(g.v0)
    caps = np.broadcast_to(np.asarray(caps, np.int64), n).copy()
    r2 = radius2(n, max_dist)
    L = _Lists(n, caps)
    tied = np.zeros(n, bool)
    width = L.d2.shape[1]
    for s in range(0, n if T else 0, chunk):
        q = p[s:s + chunk]
        d2, u, v, _ = nr.closest_on_triangle(q[:, None, :], g.v0[None], g.e1[None], g.e2[None])
        with np.errstate(invalid="ignore"):
            listed = d2 < r2[s:s + chunk, None]
        key = np.where(listed, d2, np.float32(np.inf))
        prim = np.broadcast_to(np.arange(T)[None, :], key.shape)
        order = np.lexsort((prim, key), axis=1)                                # by d2, then prim; unlisted ones behind
        rows = np.arange(len(q))[:, None]
        total = listed.sum(axis=1)
        L.total[s:s + chunk] = total
        L.stored[s:s + chunk] = np.minimum(total, caps[s:s + chunk])
        skey = key[rows, order]
        tied[s:s + chunk] = ((skey[:, 1:] == skey[:, :-1]) & (np.arange(1, T)[None, :] < total[:, None])).any(axis=1)
        w = min(width, T)
        first = order[:, :w]
        use = np.arange(w)[None, :] < L.stored[s:s + chunk, None]
        for f, src in ((L.d2, d2), (L.u, u), (L.v, v)):
            f[s:s + chunk, :w] = np.where(use, src[rows, first], f[s:s + chunk, :w])
        L.prim[s:s + chunk, :w] = np.where(use, first, L.prim[s:s + chunk, :w])
    return _slots(g, p, r2, caps, L), (L.stored if mode == K else L.total).astype(np.uint32), tied


def differing_points(a, b, caps):
    """bool [n]: some slot of the point differs between two Slots (bit for bit), segments of `caps` slots."""
    n = len(caps)
    owner = np.repeat(np.arange(n), caps)
    bad = np.zeros(len(owner), bool)
    for f in Slots._fields:
        x, y = np.ascontiguousarray(getattr(a, f)).view(np.uint32), np.ascontiguousarray(getattr(b, f)).view(np.uint32)
        bad |= (x != y).reshape(len(owner), x[0].size if len(owner) else 1).any(axis=1)
    out = np.zeros(n, bool)
    out[owner[bad]] = True
    return out
