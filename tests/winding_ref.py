"""Restatement of the generalised winding numbers (include/drt.h drt_renderer_winding_numbers / _winding_inside /
_winding_signed_distance) over the oracle's scene, for the tests.  No tests of its own.

Everything is float32 numpy in the header's operation order (numpy rounds every operation on its own; division and sqrt are correctly
rounded).  A scene is anything with `.nodes` (root last) and `.tris["p"]`, as in tests/inside_ref.py: the oracle's, or
inside_ref.product_scene() of a host scene.  The box "as the tree stores it" of a node is the node's own bmin / bmax: the packer copies
it into the parent's record, and the root's into the root box.
"""
import numpy as np

from tests import nearest_ref as nr

F = np.float32
MAX_STACK = 64
# drt.h "atan2", digit for digit: the strings are what the header and winding.hpp must hold
ATAN_COEFFS = ("8.05374449538e-2", "1.38776856032e-1", "1.99777106478e-1", "3.33329491539e-1")
TAN_PI_8, PI_4, PI_2, PI = "0.414213562", "0.785398163", "1.57079633", "3.14159265"
INV_4PI = "0.0795774715"
_C = [F(c) for c in ATAN_COEFFS]
_T8, _P4, _P2, _PI, _I4PI = F(TAN_PI_8), F(PI_4), F(PI_2), F(PI), F(INV_4PI)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def atan2(y, x):
    """drt.h "atan2" for float32 arrays, y != 0."""
    y, x = _f32(y), _f32(x)
    with np.errstate(all="ignore"):
        ax, ay = np.abs(x), np.abs(y)
        swap = ay > ax
        mx, mn = np.where(swap, ay, ax), np.where(swap, ax, ay)
        big = mn > _T8 * mx
        t = np.where(big, mn - mx, mn) / np.where(big, mn + mx, mx)
        s = t * t
        r = (((_C[0] * s - _C[1]) * s + _C[2]) * s - _C[3]) * s * t + t
        r = np.where(big, _P4 + r, r)
        r = np.where(swap, _P2 - r, r)
        r = np.where(x < 0, _PI - r, r)
        r = np.where(y < 0, -r, r)
    assert r.dtype == np.float32
    return r


def stored(osc):
    """(v0, e1, e2) [n, 3] each, as the packer stores them."""
    p = _f32(osc.tris["p"])
    return p[:, 0], p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]


def solid_angle(q, v0, e1, e2):
    """drt.h "triangle term" for matching rows: omega in steradians, exactly 0 where det == 0."""
    with np.errstate(all="ignore"):
        a = v0 - q
        b, c = a + e1, a + e2
        det = dot(a, cross(e1, e2))
        la, lb, lc = np.sqrt(dot(a, a)), np.sqrt(dot(b, b)), np.sqrt(dot(c, c))
        den = ((la * lb * lc + dot(a, b) * lc) + dot(b, c) * la) + dot(c, a) * lb
        zero = det == 0
        om = F(2) * atan2(np.where(zero, F(1), det), den)
    return np.where(zero, F(0), om).astype(np.float32)


def _finish(N, S, A, lo, hi):
    """{N[3], r2, p[3], pad} of a node from its sums and its stored box."""
    with np.errstate(all="ignore"):
        p = S / A
        ok = (A > 0) & (A < np.inf) & (np.abs(p) < np.inf).all()
        if not ok:
            p = F(0.5) * (lo + hi)
        d = np.fmax(np.abs(p - lo), np.abs(hi - p))
        r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    return np.concatenate([N, [r2], p, [F(0)]]).astype(np.float32)


def _leaf_sums(tri, start, count):
    v0, e1, e2 = tri
    N, S, A = np.zeros(3, F), np.zeros(3, F), F(0)
    with np.errstate(all="ignore"):
        for k in range(start, start + count):
            n = F(0.5) * cross(e1[k], e2[k])
            area = np.sqrt(dot(n, n))
            c = v0[k] + (e1[k] + e2[k]) / F(3)
            N, A, S = N + n, A + area, S + area * c
    return N, S, A


def _post_order(nodes):
    order, todo = [], [len(nodes) - 1] if len(nodes) else []
    while todo:
        i = todo.pop()
        order.append(i)
        if not nodes["is_leaf"][i]:
            todo += [int(nodes["child1"][i]), int(nodes["child2"][i])]
    return order[::-1]                           # children before their parent


def moments(osc):
    """drt.h "node moment" bottom-up: float32 [n_nodes, 8] in the scene's node order (nodes the root does not reach stay zero)."""
    nodes, tri = osc.nodes, stored(osc)
    out = np.zeros((len(nodes), 8), F)
    sums = {}
    with np.errstate(all="ignore"):
        for i in _post_order(nodes):
            nd = nodes[i]
            if nd["is_leaf"]:
                sums[i] = _leaf_sums(tri, int(nd["prim_start"]), int(nd["prim_count"]))
            else:
                a, b = sums[int(nd["child1"])], sums[int(nd["child2"])]
                sums[i] = (a[0] + b[0], a[1] + b[1], a[2] + b[2])
            out[i] = _finish(*sums[i], _f32(nd["bmin"]), _f32(nd["bmax"]))
    return out


def moment_direct(osc, i, tri=None):
    """One node's moment by a direct sum in the stated order: a leaf's triangles in ascending index, a parent child 1 + child 2."""
    nodes = osc.nodes
    tri = stored(osc) if tri is None else tri

    def sums(j):
        nd = nodes[j]
        if nd["is_leaf"]:
            return _leaf_sums(tri, int(nd["prim_start"]), int(nd["prim_count"]))
        with np.errstate(all="ignore"):
            a, b = sums(int(nd["child1"])), sums(int(nd["child2"]))
            return a[0] + b[0], a[1] + b[1], a[2] + b[2]

    return _finish(*sums(i), _f32(nodes[i]["bmin"]), _f32(nodes[i]["bmax"]))


def device_order(nodes):
    """Index array that puts per-node rows into the device's order: interior nodes in node order, then the leaves in node order."""
    leaf = np.asarray(nodes["is_leaf"]) != 0
    return np.concatenate([np.nonzero(~leaf)[0], np.nonzero(leaf)[0]])


def winding(osc, points, beta=2.0, mom=None, visits=None, depth=None):
    """drt.h "evaluation of a point": float32 [n].  visits: an int64 [n, 2] array that receives (nodes visited, triangles added);
    depth: an int64 [n] array that receives the largest number of stack entries."""
    q = _f32(points)[:, :3]
    n = len(q)
    acc = np.zeros(n, F)
    nodes = osc.nodes
    bad = ~np.isfinite(q).all(axis=1)
    if len(nodes) and n:
        mom = moments(osc) if mom is None else mom
        v0, e1, e2 = stored(osc)
        with np.errstate(all="ignore"):
            beta2 = F(beta) * F(beta)
        root = len(nodes) - 1
        st = np.zeros((n, MAX_STACK), np.int64)
        st[:, 0] = root
        sp = np.where(bad, 0, 1)
        while True:
            if depth is not None:
                np.maximum(depth, sp, out=depth)
            act = np.nonzero(sp > 0)[0]
            if len(act) == 0:
                break
            sp[act] -= 1
            node = st[act, sp[act]]
            if visits is not None:
                visits[act, 0] += 1
            m = mom[node]
            with np.errstate(all="ignore"):
                d = m[:, 4:7] - q[act]
                dd = dot(d, d)
                far = dd > beta2 * m[:, 3]
                term = dot(d, m[:, 0:3]) / (dd * np.sqrt(dd))
                acc[act[far]] = acc[act[far]] + term[far]
            leaf = (nodes["is_leaf"][node] != 0) & ~far
            la, ln = act[leaf], node[leaf]
            start, cnt = nodes["prim_start"][ln], nodes["prim_count"][ln]
            for k in range(int(cnt.max()) if len(ln) else 0):                  # ascending index
                sel = cnt > k
                r, prim = la[sel], (start[sel] + k).astype(np.int64)
                with np.errstate(all="ignore"):
                    acc[r] = acc[r] + solid_angle(q[r], v0[prim], e1[prim], e2[prim])
                if visits is not None:
                    visits[r, 1] += 1
            inner = (nodes["is_leaf"][node] == 0) & ~far
            ia, inode = act[inner], node[inner]
            for c in (nodes["child2"][inode], nodes["child1"][inode]):       # child 2 first: child 1 is the next one popped
                st[ia, sp[ia]] = c
                sp[ia] += 1
    with np.errstate(all="ignore"):
        w = (acc * _I4PI).astype(np.float32)
    w[bad] = np.nan
    return w


def inside(osc, points, beta=2.0, threshold=0.5, mom=None):
    with np.errstate(invalid="ignore"):
        return winding(osc, points, beta, mom) >= F(threshold)


def signed_distance(osc, points, max_dist=np.inf, beta=2.0, threshold=0.5, g=None, mom=None):
    """nearest_ref.nearest's record with side = -1 where w >= threshold, else +1, miss records included."""
    near = nr.nearest(nr.from_oracle(osc) if g is None else g, points, max_dist)
    return near._replace(side=np.where(inside(osc, points, beta, threshold, mom), F(-1), F(1)).astype(np.float32))


def brute_force64(pos, points, chunk=256):
    """w in float64 over ALL triangles pos [T, 3, 3] with numpy's arctan2: the yardstick of the fp32 rule's error."""
    pos, q = np.asarray(pos, np.float64), np.asarray(points, np.float64)[:, :3]
    out = np.zeros(len(q))
    for s in range(0, len(q), chunk):
        a = pos[None, :, 0] - q[s:s + chunk, None]
        b = pos[None, :, 1] - q[s:s + chunk, None]
        c = pos[None, :, 2] - q[s:s + chunk, None]
        la, lb, lc = [np.linalg.norm(v, axis=2) for v in (a, b, c)]
        det = np.einsum("ijk,ijk->ij", a, np.cross(b, c))
        den = la * lb * lc + np.einsum("ijk,ijk->ij", a, b) * lc + np.einsum("ijk,ijk->ij", b, c) * la + np.einsum("ijk,ijk->ij", c, a) * lb
        out[s:s + chunk] = (2 * np.arctan2(det, den)).sum(axis=1) / (4 * np.pi)
    return out
