"""Restatement of the plane-section query (include/drt.h drt_renderer_plane_sections) in float32 numpy over nearest_ref.Geometry, for
the tests.  No tests of its own.  Written from the header, not from the kernel.

Every operation is one float32 numpy operation, in the order the header writes it (numpy rounds each one on its own; / is the
correctly rounded division).  The traversal is a stack traversal vectorised over planes, as overlap_ref.overlap is over boxes: the
header says that the set of records does not depend on the traversal order, so this one pops child 2 last or first as the tree has
them and SORTS the (plane, triangle) pairs it finds; the kernel's level-by-level lists are not restated.  brute_force is the same
triangle test over ALL triangles, with no cull.
"""
import numpy as np

from tests import nearest_ref as nr
from tests.overlap_ref import caps_of  # noqa: F401  (re-exported: the segments are the box query's)

LIST, ANY = 0, 1                                                          # drt.h DRT_SECTION_LIST, DRT_SECTION_ANY
FLT_MAX = np.finfo(np.float32).max
SECTION = np.dtype([("p", "<f4", 3), ("prim", "<i4"), ("q", "<f4", 3), ("code", "<i4")])      # drt_section, 32 bytes
assert SECTION.itemsize == 32
MISS = np.zeros(1, SECTION)
MISS["prim"] = -1                                                         # the miss record: all zeros with prim = -1


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def pack(normals, d):
    """drt_plane records [N, 4] float32: n, d.  d: [N] or a scalar."""
    n = _f32(normals).reshape(-1, 3)
    out = np.zeros((len(n), 4), np.float32)
    out[:, 0:3] = n
    out[:, 3] = np.broadcast_to(_f32(d), len(n))
    return out


def valid(planes):
    """drt.h "validity": all four words satisfy fabsf(x) <= FLT_MAX."""
    with np.errstate(invalid="ignore"):
        return (np.abs(planes) <= FLT_MAX).all(axis=-1)


def signed(n, d, x):
    """drt.h "signed value": s(x) = dot(n, x) - d."""
    with np.errstate(all="ignore"):
        return nr.dot(n, x) - d


def cull_corners(n, bmin, bmax):
    """drt.h "node cull": cmin[j] = n[j] >= 0 ? bmin[j] : bmax[j], cmax[j] the other one."""
    with np.errstate(invalid="ignore"):
        pos = n >= 0
    return np.where(pos, bmin, bmax), np.where(pos, bmax, bmin)


def cull_passes(n, d, bmin, bmax):
    """... a box passes iff s(cmin) < 0 && s(cmax) >= 0."""
    cmin, cmax = cull_corners(n, bmin, bmax)
    with np.errstate(invalid="ignore"):
        return (signed(n, d, cmin) < 0) & (signed(n, d, cmax) >= 0)


def classify(n, d, v0, e1, e2):
    """drt.h "triangle test" on (plane, triangle) pairs (broadcast over the leading dimensions): (cut bool [...], v [..., 3, 3] the
    vertices v0, v0 + e1, v0 + e2, s [..., 3] their signed values)."""
    with np.errstate(all="ignore"):
        v = np.stack(np.broadcast_arrays(v0, v0 + e1, v0 + e2), axis=-2)
        s = np.stack([signed(n, d, v[..., i, :]) for i in range(3)], axis=-1)
        above = s >= 0
    cut = ~((above[..., 0] == above[..., 1]) & (above[..., 1] == above[..., 2]))
    return cut, v, s


def _cut_point(va, sa, vb, sb):
    """drt.h cut(a, b): lo the below one of the two, hi the above one; t = s_lo / (s_lo - s_hi), lo + (hi - lo) * t per component."""
    with np.errstate(all="ignore"):
        a_above = sa >= 0
        lo, hi = np.where(a_above[:, None], vb, va), np.where(a_above[:, None], va, vb)
        s_lo, s_hi = np.where(a_above, sb, sa), np.where(a_above, sa, sb)
        t = s_lo / (s_lo - s_hi)
        return (lo + (hi - lo) * t[:, None]).astype(np.float32)


def segments_of(v, s):
    """drt.h "segment" for CUT triangles, vertices v [M, 3, 3] and signed values s [M, 3]: (p [M, 3], q [M, 3], code [M])."""
    with np.errstate(invalid="ignore"):
        above = s >= 0
    # the apex is the vertex alone in its class
    k = np.where(above[:, 1] == above[:, 2], 0, np.where(above[:, 0] == above[:, 2], 1, 2))
    m = np.arange(len(k))
    k1, k2 = (k + 1) % 3, (k + 2) % 3
    P = _cut_point(v[m, k], s[m, k], v[m, k1], s[m, k1])
    Q = _cut_point(v[m, k], s[m, k], v[m, k2], s[m, k2])
    apex_above = above[m, k]
    p = np.where(apex_above[:, None], P, Q)                                # apex above: P -> Q; apex below: Q -> P
    q = np.where(apex_above[:, None], Q, P)
    return p.astype(np.float32), q.astype(np.float32), (k + 4 * apex_above).astype(np.int32)


def _records(g, planes, pairs_plane, pairs_prim, n, caps):
    """The flat records from (plane, prim) pairs in any order: each plane's first cap records in ascending triangle index, the miss
    record behind them; counts = all of them."""
    caps = np.broadcast_to(np.asarray(caps, np.int64), n).copy()
    base = np.concatenate([[0], np.cumsum(caps)])
    out = np.repeat(MISS, int(base[-1]))
    counts = np.bincount(pairs_plane, minlength=n).astype(np.uint32) if len(pairs_plane) else np.zeros(n, np.uint32)
    if len(pairs_plane):
        order = np.lexsort((pairs_prim, pairs_plane))                     # it sorts: the list is ascending on any tree
        b, t = pairs_plane[order], pairs_prim[order]
        start = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
        rank = np.arange(len(b)) - start[b]
        keep = rank < caps[b]
        b, t, rank = b[keep], t[keep], rank[keep]
        cut, v, s = classify(planes[b, 0:3], planes[b, 3], g.v0[t], g.e1[t], g.e2[t])
        assert cut.all()
        p, q, code = segments_of(v, s)
        slot = base[b] + rank
        out["p"][slot], out["q"][slot], out["prim"][slot], out["code"][slot] = p, q, t, code
    return out, counts


def sections(g, planes, caps, mode=LIST, visits=None):
    """drt.h "node cull", "triangle test", "segment", "record" and "list" for planes [N, 4] with caps a scalar or [N] (already
    clamped: caps_of): (records SECTION of sum(caps) slots, plane i's at [cumsum(caps)[i-1], cumsum(caps)[i]); counts uint32 [N]).
    Mode ANY: no slots (caps is ignored), counts 0 or 1.  visits: an int64 [N] array that receives the nodes each plane visited."""
    planes = _f32(planes).reshape(-1, 4)
    n = len(planes)
    nn, dd = planes[:, 0:3], planes[:, 3]
    found_plane, found_prim = [], []
    if len(g.bmin) and n:
        root = len(g.bmin) - 1                                                 # the root is the last node
        st = np.zeros((n, min(len(g.bmin), 2 * nr.MAX_STACK)), np.int64)   # (a depth-first stack holds at most depth + 1)
        st[:, 0] = root
        # an invalid plane pushes nothing; the root is tested against the root box
        sp = (valid(planes) & cull_passes(nn, dd, g.bmin[root], g.bmax[root])).astype(np.int64)
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
            for k in range(int(count.max()) if len(ln) else 0):                # a leaf's triangles in order
                sel = count > k
                r, t = la[sel], start[sel] + k
                cut, _, _ = classify(nn[r], dd[r], g.v0[t], g.e1[t], g.e2[t])
                found_plane.append(r[cut])
                found_prim.append(t[cut])
            ia, inode = act[~leaf], node[~leaf]
            if len(ia):
                for child in (g.child2[inode], g.child1[inode]):
                    push = cull_passes(nn[ia], dd[ia], g.bmin[child], g.bmax[child])
                    r = ia[push]
                    st[r, sp[r]] = child[push]
                    sp[r] += 1
    pb = np.concatenate(found_plane) if found_plane else np.zeros(0, np.int64)
    pp = np.concatenate(found_prim) if found_prim else np.zeros(0, np.int64)
    if mode == ANY:
        return np.zeros(0, SECTION), np.minimum(np.bincount(pb, minlength=n), 1).astype(np.uint32)
    return _records(g, planes, pb, pp, n, caps)


def brute_force(g, planes, caps, mode=LIST, chunk=64):
    """The triangle test of every valid plane over ALL triangles, with no cull: (records, counts) as sections'."""
    planes = _f32(planes).reshape(-1, 4)
    n, T = len(planes), len(g.v0)
    ok = valid(planes)
    found_plane, found_prim = [], []
    for s in range(0, n if T else 0, chunk):
        e = slice(s, s + chunk)
        cut, _, _ = classify(planes[e, None, 0:3], planes[e, None, 3], g.v0[None], g.e1[None], g.e2[None])
        i, t = np.nonzero(cut & ok[e, None])
        found_plane.append(i + s)
        found_prim.append(t)
    pb = np.concatenate(found_plane) if found_plane else np.zeros(0, np.int64)
    pp = np.concatenate(found_prim) if found_prim else np.zeros(0, np.int64)
    if mode == ANY:
        return np.zeros(0, SECTION), np.minimum(np.bincount(pb, minlength=n), 1).astype(np.uint32)
    return _records(g, planes, pb, pp, n, caps)


def whole(g, planes):
    """Every record of every plane: (records, counts) at capacities = the counts."""
    _, counts = sections(g, planes, 0)
    return sections(g, planes, counts.astype(np.int64))


def areas(planes, records, counts):
    """drt.h: 0.5 * sum dot(n / |n|, cross(p, q)) per plane, in float64, plane by plane (n = 0: 0).  records: the whole lists."""
    planes = _f32(planes).reshape(-1, 4)
    out = np.zeros(len(planes), np.float64)
    start = np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))])
    for i in range(len(planes)):
        nn = planes[i, 0:3].astype(np.float64)
        length = np.sqrt((nn * nn).sum())
        if length > 0 and start[i + 1] > start[i]:
            r = records[start[i]:start[i + 1]]
            out[i] = 0.5 * (np.cross(r["p"].astype(np.float64), r["q"].astype(np.float64)) @ (nn / length)).sum()
    return out
