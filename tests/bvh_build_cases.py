"""Inputs for the BVH builders, for tests/test_bvh_build_cases.py (CPU: the host builder against the oracle's) and
tests/test_gpu_bvh_build.py (the device builder against both).  No tests of its own.

A case is a list of triangles in load order and the (leaf, bins) settings it is built with; every setting carries what all three
builders do with it, RETURNS or REFUSES (DRT_ERR_BVH: some node's chosen plane leaves a side empty, where the reference never
terminates).  The expectations are written down here, not discovered at run time: they were established with the host builder and
the oracle's builder, which agreed node for node wherever both returned.  Normals, UVs and materials are those of
tests/test_gpu_bvh_build.py's _soup: one normal, zero UVs, one material.

What each case meets is said beside it; tests/test_bvh_build_cases.py asserts that it still does (a later change of a seed must
not quietly empty a case of its point).
"""
import collections
import functools

import numpy as np

import oracle
from tests import hostile_meshes as hm
from tests import ray_query_ref as rq

RETURNS, REFUSES = True, False
Case = collections.namedtuple("Case", "name pos settings")          # settings: [(leaf, bins, RETURNS | REFUSES)]
ONE_MATERIAL = [((0.8, 0.8, 0.8), -1)]

# hostile_x4 times 2^k.  The SAH still works at the first four: at 2^56 the root's area is just below FLT_MAX, at 2^-72 the areas
# are subnormal (57, -73 and -74 return as well).  At the others areas overflow or underflow to 0, the cost is NaN and the first
# plane wins until a side is empty.  Where that happens was tried with (n - 1, 8), where only the root splits: at 123, 124 and
# -75 .. -80 the root still splits and the refusal comes levels below it (at -78 (700, 8) returns a tree of 9 nodes); at 58 .. 122,
# 125, 126 and -90 .. -126 the root's own first plane leaves its left side empty.
SCALES_IN_RANGE = (40, 56, -60, -72)
SCALES_REFUSED_BELOW_THE_ROOT = (124, -75, -78)
SCALES_REFUSED_AT_THE_ROOT = (58, 100, -126)
# rq.soup(n, n, 0.25, 4.0) at (1, 3).  n = 511, 1023, 1024 and 4097 with these seeds are refused by both CPU builders and left out.
SIZES = (2, 3, 5, 63, 64, 65, 512, 513, 1025)
CHAIN = 110                                                         # 109 levels below the root; 240 is refused by every builder


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _soup1500():
    return rq.soup(1500, 7, 0.25, 2.0)[0]


def _poke(pos, seed, count, value):
    """`count` distinct coordinates of pos, chosen at random, set to value."""
    out = pos.copy()
    where = np.random.default_rng(seed).choice(out.size, count, replace=False)
    out.reshape(-1)[where] = value
    return out


def _one(pos, where, value):
    out = pos.copy()
    out[where] = value
    return out


def _signed_zeros(rng, shape):
    return np.where(rng.uniform(size=shape) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)


def _hostile_x4():
    base = hm.degenerate().pos
    return _f32(np.concatenate([base + np.float32([8 * i, 0, 0]) for i in range(4)]))


def _zeros():
    """rq.soup(1500, 5, 0.25, 2.0) with about 15 % of the x coordinates set to a zero of either sign (seed 11, the first tried)."""
    pos = rq.soup(1500, 5, 0.25, 2.0)[0].copy()
    rng = np.random.default_rng(11)
    hit = rng.uniform(size=(1500, 3)) < 0.15
    pos[:, :, 0] = np.where(hit, _signed_zeros(rng, (1500, 3)), pos[:, :, 0])
    return pos


def _flat():
    """1 500 triangles of half-size 0.25 about centres uniform in [-4, 4]^3, every z a zero of either sign (seed 1, the first tried)."""
    rng = np.random.default_rng(1)
    pos = _f32(rng.uniform(-4, 4, (1500, 1, 3)) + rng.uniform(-0.25, 0.25, (1500, 3, 3)))
    pos[:, :, 2] = _signed_zeros(rng, (1500, 3))
    return pos


def _axis():
    """700 point-triangles (k, 0, 0), k a permutation of 0..699 (seed 13): every box has zero area, so every cost is NaN."""
    k = np.random.default_rng(13).permutation(700).astype(np.float32)
    pos = np.zeros((700, 3, 3), np.float32)
    pos[:, :, 0] = k[:, None]
    return pos


def _line():
    t = np.linspace(0, 1, 700).astype(np.float32)
    return _f32(t[:, None, None] * np.float32([1, 2, 3])[None, None, :] * np.ones((1, 3, 1), np.float32))


def _row(descending):
    """2 048 copies of one triangle in the plane x = const at x = 0..2047: integer centroids that lie exactly on planes, nodes of
    exactly 1 024 and 512 triangles.  Ascending: no partition swaps anything.  Descending: the root's swaps 1 024 pairs."""
    x = np.arange(2048, dtype=np.float32)
    pos = np.tile(np.float32([[0, -.25, -.25], [0, .25, -.25], [0, 0, .5]]), (2048, 1, 1))
    pos[:, :, 0] = (x[::-1] if descending else x)[:, None]
    return pos


def _chain(right):
    """rq.degenerate_chain(110) times 2^-60 (areas stay finite): one triangle peels off per level, 109 levels.  Negated in x the
    chain grows to the right, where the left sibling of every level waits on the reference's stack.  As it is, it would not grow
    to the left one triangle at a time: the plane of two bins rounds to the centroid 2^(k-1) exactly, `c < plane` is false and two
    triangles leave per level (66 levels).  So the left chain has its third vertex at 1.5 x: the plane 0.75 * 2^k then lies
    strictly between the centroids 7/12 * 2^k and 7/6 * 2^k."""
    pos = _f32(rq.degenerate_chain(CHAIN)[0] * np.float32(2.0 ** -60))
    if right:
        pos[:, :, 0] = -pos[:, :, 0]
    else:
        pos[:, 2, 0] *= np.float32(1.5)
    return pos


def _scaled(pos, k):
    with np.errstate(over="ignore", under="ignore"):
        return _f32(pos * np.float32(2.0 ** k))


HOSTILE_SETTINGS = [(4, 8, RETURNS), (2, 16, RETURNS), (3, 3, RETURNS), (20, 8, RETURNS), (8, 64, RETURNS),
                    (1, 2, REFUSES), (1, 8, REFUSES)]                 # leaf 1: the duplicates cannot be separated


@functools.lru_cache(maxsize=None)
def cases():
    """{name: Case} of the whole catalogue."""
    x4 = _hostile_x4()
    n4 = len(x4)
    soup = _soup1500()
    out = [
        # zero-area triangles, needles and duplicates spread over three chunks; the same far from the origin
        Case("hostile_x4", x4, HOSTILE_SETTINGS),
        Case("hostile_x4_offset", _f32(x4 + hm.OFFSET), HOSTILE_SETTINGS),
    ]
    for k in SCALES_IN_RANGE:
        out.append(Case("hostile_x4_scaled(%d)" % k, _scaled(x4, k), [(4, 8, RETURNS)] + ([(2, 16, RETURNS)] if k == -60 else [])))
    for k in SCALES_REFUSED_BELOW_THE_ROOT:
        out.append(Case("hostile_x4_scaled(%d)" % k, _scaled(x4, k), [(4, 8, REFUSES), (n4 - 1, 8, RETURNS)] + ([(700, 8, RETURNS)] if k == -78 else [])))
    for k in SCALES_REFUSED_AT_THE_ROOT:                           # (n, 8): a single leaf, the tree that has to survive the refusal
        out.append(Case("hostile_x4_scaled(%d)" % k, _scaled(x4, k), [(4, 8, REFUSES), (n4 - 1, 8, REFUSES), (n4, 8, RETURNS)]))
    out += [
        # the zero-sign freedom; delta == 0 on one axis, every candidate of that axis empty
        Case("zeros", _zeros(), [(4, 8, RETURNS), (1, 2, REFUSES)]),
        Case("flat", _flat(), [(4, 8, RETURNS), (2, 4, REFUSES), (1, 16, REFUSES)]),
        # parent area 0 in every node; zero-volume triangles in non-zero boxes
        Case("axis", _axis(), [(4, 8, RETURNS), (1, 2, RETURNS), (1, 3, RETURNS)]),
        Case("line", _line(), [(4, 8, RETURNS), (1, 2, RETURNS)]),
        # fminf skips a NaN and a NaN centroid goes right; inf bounds through the key map and a NaN cost at the root; refusal below it
        Case("nan", _poke(soup, 21, 20, np.nan), [(4, 8, RETURNS), (20, 8, RETURNS)]),
        Case("one_inf", _one(soup, (5, 0, 0), np.inf),[(4, 8, RETURNS), (20, 8, RETURNS)]),
        Case("many_inf", _poke(soup, 23, 20, np.inf), [(4, 8, REFUSES), (20, 8, REFUSES), (1499, 8, RETURNS)]),
        # (-inf makes the root's planes NaN, so everything goes right at the root itself; (1500, 8) is a single leaf)
        Case("many_minus_inf", _poke(soup, 23, 20, -np.inf), [(4, 8, REFUSES), (20, 8, REFUSES), (1499, 8, REFUSES), (1500, 8, RETURNS)]),
        Case("asc", _row(False), [(1, 2, RETURNS), (4, 8, RETURNS), (1, 32, RETURNS)]),
        Case("desc", _row(True), [(1, 2, RETURNS), (4, 8, RETURNS), (1, 32, RETURNS)]),
        Case("chain_left", _chain(False), [(1, 2, RETURNS)]),
        Case("chain_right", _chain(True), [(1, 2, RETURNS)]),
    ]
    # the smallest trees and the root's chunk edges
    out += [Case("soup%d" % n, rq.soup(n, n, 0.25, 4.0)[0], [(1, 3, RETURNS)]) for n in SIZES]
    # 765 candidates per node; a root with two leaf children; max(leaf, 0) + 1 in the device builder's buffer bounds
    out.append(Case("soup1500", soup, [(4, 64, RETURNS), (4, 256, RETURNS), (1499, 2, RETURNS), (0, 8, REFUSES), (-1, 8, REFUSES)]))
    assert len({c.name for c in out}) == len(out) and all(c.pos.dtype == np.float32 and c.pos.shape[1:] == (3, 3) for c in out)
    return {c.name: c for c in out}


def entries(returns=None):
    """[(case name, leaf, bins, returns)] of the whole catalogue, or of its returning / refusing settings only."""
    return [(c.name, leaf, bins, r) for c in cases().values() for leaf, bins, r in c.settings if returns is None or r == returns]


def entry_id(e):
    return "%s-%d-%d" % e[:3]


def a_returning_setting(name):
    """(leaf, bins) of the case's first setting that returns (every case has one)."""
    return next((leaf, bins) for leaf, bins, r in cases()[name].settings if r)


def streams(pos):
    n = len(pos)
    return pos, np.tile(np.float32([0, 1, 0]), (n, 3, 1)), np.zeros((n, 3, 2), np.float32), np.zeros(n, np.int32)


def product_scene(drt, pos):
    """The case as the product's scene, not built yet."""
    sc = drt.Scene()
    sc.addMaterial(*ONE_MATERIAL[0])
    sc.setGeometry(*streams(pos))
    return sc


def build(drt, sc, leaf, bins, device=-1):
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount, b.m_BuildDevice = leaf, bins, device
    b.buildIterative(sc)
    return sc


def oracle_scene(pos):
    """The case as the oracle's scene, not built yet (build_bvh raises RuntimeError where the oracle's builder fails)."""
    p, nrm, uv, mat = streams(pos)
    tris = np.zeros(len(p), oracle.TRI_DTYPE)
    a = [_f32(p.reshape(-1, 3)), _f32(nrm.reshape(-1, 3)), _f32(uv.reshape(-1, 2))]
    oracle.lib().o_build_triangles(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, mat.ctypes.data, len(p), tris.ctypes.data)
    return oracle.Scene(tris, ONE_MATERIAL, [])


# ---------------------------------------------------------------- what a tree shows (numpy, on the product's node records)

def levels(nodes):
    """The depth of every node below the root (root 0), the root being the last node."""
    depth = np.full(len(nodes), -1)
    depth[-1] = 0
    todo = [len(nodes) - 1]
    while todo:
        i = todo.pop()
        if not nodes["is_leaf"][i]:
            for c in (int(nodes["child1"][i]), int(nodes["child2"][i])):
                depth[c] = depth[i] + 1
                todo.append(c)
    assert (depth >= 0).all()
    return depth


def negative_zero_bounds(nodes):
    b = np.concatenate([nodes["bmin"], nodes["bmax"]], axis=1)
    return int((b.view(np.uint32) == 0x80000000).sum())
