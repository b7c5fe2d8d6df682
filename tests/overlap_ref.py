"""Restatement of the box overlap query (include/drt.h drt_renderer_overlap_boxes) in float32 numpy over nearest_ref.Geometry, for the
tests.  No tests of its own.

Every operation is one float32 numpy operation, in the order the header writes it (numpy rounds each one on its own; np.fmin / np.fmax
drop a NaN operand as fminf / fmaxf do).  The traversal is vectorised over boxes as nearest_ref.nearest is over points: every step
pops one stack entry of every box that still has one, over the same tree.  Only the predicate leaves the triangle test, so a list is
the ascending triangle indices of the visited leaves' listed triangles; the insert of the kernel is restated only as far as it can be
observed -- the first cap of the sorted list -- and `events` reports what the arrival order made it do.  brute_force is the same
triangle test over ALL triangles, with no cull.
"""
import bisect

import numpy as np

from tests import nearest_ref as nr

LIST, ANY = 0, 1                                                          # drt.h DRT_OVERLAP_LIST, DRT_OVERLAP_ANY
IDENTITY = np.eye(3, dtype=np.float32)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def pack(center, half, axes=None):
    """drt_box records [N, 16] float32: center, half, axis[3][3] (default the identity), pad 0.  half: [N, 3], [3] or a scalar."""
    c = _f32(center).reshape(-1, 3)
    n = len(c)
    out = np.zeros((n, 16), np.float32)
    out[:, 0:3] = c
    out[:, 3:6] = np.broadcast_to(_f32(half), (n, 3))
    out[:, 6:15] = np.broadcast_to(IDENTITY if axes is None else _f32(axes), (n, 3, 3)).reshape(n, 9)
    return out


def from_corners(lo, hi):
    """center = (lo + hi) / 2, half = (hi - lo) / 2 in float32, as Renderer.overlapBoxes(lo=, hi=) makes them."""
    lo, hi = _f32(lo).reshape(-1, 3), _f32(hi).reshape(-1, 3)
    return pack((lo + hi) / np.float32(2), (hi - lo) / np.float32(2))


def unpack(boxes):
    b = _f32(boxes).reshape(-1, 16)
    return b[:, 0:3], b[:, 3:6], b[:, 6:15].reshape(-1, 3, 3)


def caps_of(offsets, capacity):
    """drt.h "segments": cap_i = offsets[i+1] > offsets[i] ? the difference : 0, clamped so that offsets[i] + cap_i <= capacity."""
    o = np.asarray(offsets, np.int64)
    cap = np.where(o[1:] > o[:-1], o[1:] - o[:-1], 0)
    return np.minimum(cap, np.clip(capacity - o[:-1], 0, None))


def world_bounds(boxes):
    """drt.h "world bounds of the query": (qmin, qmax) [N, 3]."""
    c, h, ax = unpack(boxes)
    with np.errstate(all="ignore"):
        ext = (np.abs(ax[:, 0, :]) * h[:, 0:1] + np.abs(ax[:, 1, :]) * h[:, 1:2]) + np.abs(ax[:, 2, :]) * h[:, 2:3]
        return c - ext, c + ext


def cull_passes(qmin, qmax, bmin, bmax):
    """drt.h "node cull": closed, no arithmetic on the node, a NaN fails."""
    with np.errstate(invalid="ignore"):
        return ((qmin <= bmax) & (bmin <= qmax)).all(axis=-1)


def _min3(a, b, c):
    return np.fmin(np.fmin(a, b), c)


def _max3(a, b, c):
    return np.fmax(np.fmax(a, b), c)


def _edge_axis(la, lb, hm, hn, pm, pn):
    """One edge axis on the two box axes (m, n) it does not vanish on: s_i = la p_i[m] + lb p_i[n], r = half[m] |la| + half[n] |lb|."""
    s = [la * pm[i] + lb * pn[i] for i in range(3)]
    r = hm * np.abs(la) + hn * np.abs(lb)
    return (_min3(*s) <= r) & (_max3(*s) >= -r)


def triangle_axes(center, half, axes, v0, e1, e2):
    """drt.h "triangle test" on (box, triangle) pairs (broadcast over the leading dimensions): bool [..., 13], ok of the three box
    axes, the plane and the nine edge axes (f1: k = 0, 1, 2; g; f2) in the header's order."""
    with np.errstate(all="ignore"):
        a = v0 - center
        p0 = np.stack([nr.dot(axes[..., k, :], a) for k in range(3)], axis=-1)
        f1 = np.stack([nr.dot(axes[..., k, :], e1) for k in range(3)], axis=-1)
        f2 = np.stack([nr.dot(axes[..., k, :], e2) for k in range(3)], axis=-1)
        p1, p2, g = p0 + f1, p0 + f2, f2 - f1
        h = np.broadcast_to(half, p0.shape)
        ok = []
        for k in range(3):
            ok.append((_min3(p0[..., k], p1[..., k], p2[..., k]) <= h[..., k]) & (_max3(p0[..., k], p1[..., k], p2[..., k]) >= -h[..., k]))
        n = np.stack([f1[..., 1] * f2[..., 2] - f1[..., 2] * f2[..., 1], f1[..., 2] * f2[..., 0] - f1[..., 0] * f2[..., 2],
                      f1[..., 0] * f2[..., 1] - f1[..., 1] * f2[..., 0]], axis=-1)
        d = nr.dot(n, p0)
        r = (np.abs(n[..., 0]) * h[..., 0] + np.abs(n[..., 1]) * h[..., 1]) + np.abs(n[..., 2]) * h[..., 2]
        ok.append(np.abs(d) <= r)
        x, y, z = ([p[..., j] for p in (p0, p1, p2)] for j in range(3))
        for E in (f1, g, f2):
            ok.append(_edge_axis(-E[..., 2], E[..., 1], h[..., 1], h[..., 2], y, z))       # k = 0: L = (0, -E.z, E.y)
            ok.append(_edge_axis(E[..., 2], -E[..., 0], h[..., 0], h[..., 2], x, z))       # k = 1: L = (E.z, 0, -E.x)
            ok.append(_edge_axis(-E[..., 1], E[..., 0], h[..., 0], h[..., 1], x, y))       # k = 2: L = (-E.y, E.x, 0)
        return np.stack(ok, axis=-1)


def triangle_listed(center, half, axes, v0, e1, e2):
    return triangle_axes(center, half, axes, v0, e1, e2).all(axis=-1)


def _segments(pairs_box, pairs_prim, n, caps, events=None):
    """The flat records from the (box, prim) pairs in arrival order: each box's first cap indices in ascending order, -1 behind
    them; counts = all of them."""
    caps = np.broadcast_to(np.asarray(caps, np.int64), n).copy()
    base = np.concatenate([[0], np.cumsum(caps)])
    prims = np.full(int(base[-1]), -1, np.int32)
    counts = np.bincount(pairs_box, minlength=n).astype(np.uint32) if len(pairs_box) else np.zeros(n, np.uint32)
    if events is not None:
        events["out_of_order"], events["evicted"] = np.zeros(n, bool), np.zeros(n, bool)
    if len(pairs_box):
        arrival = np.argsort(pairs_box, kind="stable")                         # per box, in arrival order
        b, t = pairs_box[arrival], pairs_prim[arrival]
        start = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
        if events is not None:
            for i in np.nonzero((counts > 1) & (caps > 0))[0]:                   # the kernel's insert, step by step
                kept = []
                for cand in t[start[i]:start[i + 1]].tolist():
                    if len(kept) == caps[i]:
                        if not cand < kept[-1]:
                            continue
                        events["evicted"][i] = True
                        kept.pop()
                    if kept and cand < kept[-1]:
                        events["out_of_order"][i] = True
                    bisect.insort(kept, cand)
        order = np.lexsort((t, b))
        b, t = b[order], t[order]
        rank = np.arange(len(b)) - start[b]
        keep = rank < caps[b]
        prims[base[b[keep]] + rank[keep]] = t[keep]
    return prims, counts


def overlap(g, boxes, caps, mode=LIST, visits=None, events=None):
    """drt.h "traversal" for boxes [N, 16] with caps a scalar or [N] (already clamped: caps_of): (prims int32 of sum(caps) slots, box
    i's at [cumsum(caps)[i-1], cumsum(caps)[i]); counts uint32 [N]).  Mode ANY: no slots (caps is ignored), counts 0 or 1.  visits:
    an int64 [N] array that receives the number of nodes each box visited.  events: a dict that receives "out_of_order" and
    "evicted", bool [N]: the box had a triangle inserted before a stored one / into a full list."""
    boxes = _f32(boxes).reshape(-1, 16)
    n = len(boxes)
    c, h, ax = unpack(boxes)
    qmin, qmax = world_bounds(boxes)
    found_box, found_prim = [], []
    if len(g.bmin) and n:
        root = len(g.bmin) - 1                                                 # the root is the last node
        st = np.zeros((n, nr.MAX_STACK), np.int64)
        st[:, 0] = root
        sp = cull_passes(qmin, qmax, g.bmin[root], g.bmax[root]).astype(np.int64)       # the root is tested against the root box
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
            done = np.zeros(len(la), bool)                                     # mode ANY: the box has its triangle
            for k in range(int(count.max()) if len(ln) else 0):                # a leaf's triangles in order
                sel = (count > k) & ~done
                r, t = la[sel], start[sel] + k
                listed = triangle_listed(c[r], h[r], ax[r], g.v0[t], g.e1[t], g.e2[t])
                found_box.append(r[listed])
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
    pb = np.concatenate(found_box) if found_box else np.zeros(0, np.int64)
    pp = np.concatenate(found_prim) if found_prim else np.zeros(0, np.int64)
    if mode == ANY:
        return np.zeros(0, np.int32), np.bincount(pb, minlength=n).astype(np.uint32)
    return _segments(pb, pp, n, caps, events)


def brute_force(g, boxes, caps, mode=LIST, chunk=64):
    """The triangle test over ALL triangles, with no cull: (prims, counts) as overlap's."""
    boxes = _f32(boxes).reshape(-1, 16)
    n, T = len(boxes), len(g.v0)
    c, h, ax = unpack(boxes)
    found_box, found_prim = [], []
    for s in range(0, n if T else 0, chunk):
        e = slice(s, s + chunk)
        listed = triangle_listed(c[e, None], h[e, None], ax[e, None], g.v0[None], g.e1[None], g.e2[None])
        i, t = np.nonzero(listed)
        found_box.append(i + s)
        found_prim.append(t)
    pb = np.concatenate(found_box) if found_box else np.zeros(0, np.int64)
    pp = np.concatenate(found_prim) if found_prim else np.zeros(0, np.int64)
    if mode == ANY:
        return np.zeros(0, np.int32), np.minimum(np.bincount(pb, minlength=n), 1).astype(np.uint32)
    return _segments(pb, pp, n, caps)


def pair_sets(prims, counts):
    """The (box, prim) pairs of a result whose capacities were its counts, as a set of box * 2^32 + prim."""
    owner = np.repeat(np.arange(len(counts), dtype=np.int64), np.asarray(counts, np.int64))
    assert len(owner) == len(prims) and (np.asarray(prims) >= 0).all()
    return set((owner * (1 << 32) + np.asarray(prims, np.int64)).tolist())
