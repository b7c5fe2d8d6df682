"""The nearest-list rule of include/drt.h as tests/near_list_ref.py restates it (CPU only): hand-derived lists on one triangle and on
the two-triangle quad, miss records, NaN inputs and zero-area triangles, capacities, and on a deep triangle soup and cornell_box the
float32 brute force, the agreement of the two modes and of slot 0 with the nearest query, and the pruning of mode K."""
import numpy as np
import pytest

import oracle
from tests import near_list_ref as nl
from tests import nearest_ref as nr
from tests.scenes import scene_path

TRI = np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
QUAD = np.float32([[[0, 0, 0], [1, 0, 0], [1, 1, 0]], [[0, 0, 0], [1, 1, 0], [0, 1, 0]]])      # test_gpu_nearest.py's: ties on the diagonal
UP = np.float32([[0, 0, 1]])
INF = np.float32(np.inf)
# (point, u, v, closest point, d2, side) of test_nearest_ref.py's HAND, three of them: a vertex, the face, on the plane
HAND = [((2, -0.5, -1), 1, 0, (1, 0, 0), 2.25, -1), ((0.25, 0.25, 3), 0.25, 0.25, (0.25, 0.25, 0), 9, 1), ((0.25, 0.5, 0), 0.25, 0.5, (0.25, 0.5, 0), 0, 1)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_miss_slots(s, r2):
    assert (s.prim == -1).all() and (bits(s.d2) == bits(np.broadcast_to(np.float32(r2), s.d2.shape))).all()
    for f in (s.u, s.v, s.point, s.side):
        assert (bits(f) == 0).all()


def take(s, idx):
    return nl.Slots(*[f[idx] for f in s])


def split_quad():
    """The quad under a three-node tree whose first-visited leaf holds triangle 1: both boxes are the quad's, so b1 > b2 is false,
    child 2 is pushed first and child 1 -- triangle 1 -- is popped first."""
    nodes = np.zeros(3, [("bmin", "<f4", 3), ("bmax", "<f4", 3), ("is_leaf", "<i4"), ("child1", "<i4"), ("child2", "<i4"), ("prim_start", "<i4"),
                         ("prim_count", "<i4")])
    lo, hi = QUAD.reshape(-1, 3).min(axis=0), QUAD.reshape(-1, 3).max(axis=0)
    nodes[0] = (lo, hi, 1, -1, -1, 1, 1)
    nodes[1] = (lo, hi, 1, -1, -1, 0, 1)
    nodes[2] = (lo, hi, 0, 0, 1, 0, 0)
    return nr._geometry(nodes, QUAD[:, 0], QUAD[:, 1] - QUAD[:, 0], QUAD[:, 2] - QUAD[:, 0], np.repeat(UP, 2, axis=0))


def test_one_triangle_by_hand():
    g = nr.from_triangles(TRI, UP)
    pts = np.float32([h[0] for h in HAND])
    for mode in (nl.GATHER, nl.K):
        s, counts = nl.near_list(g, pts, np.inf, 2, mode)
        assert counts.tolist() == [1, 1, 1] and counts.dtype == np.uint32 and s.prim.dtype == np.int32
        first, second = take(s, slice(0, None, 2)), take(s, slice(1, None, 2))
        assert first.prim.tolist() == [0, 0, 0] and first.d2.tolist() == [h[4] for h in HAND]
        assert first.u.tolist() == [h[1] for h in HAND] and first.v.tolist() == [h[2] for h in HAND]
        assert first.point.tolist() == [list(map(float, h[3])) for h in HAND] and first.side.tolist() == [h[5] for h in HAND]
        assert_miss_slots(second, INF)                                              # the miss record {r2, -1, 0, 0} and surf's {0, 0, 0, 0}
        ref = nr.nearest(g, pts)
        for f in ("d2", "u", "v", "point", "side"):
            assert (bits(getattr(first, f)) == bits(getattr(ref, f))).all(), f      # nearest's bits
    # a finite radius, strictly: d2 < r2
    s, counts = nl.near_list(g, pts, np.float32([1.5, 3, 0]), 1, nl.GATHER)
    assert counts.tolist() == [0, 0, 0] and s.d2.tolist() == [2.25, 9, 0] and (s.prim == -1).all()
    s, counts = nl.near_list(g, pts, np.float32([1.75, 3.5, 1e-3]), 1, nl.K)
    assert counts.tolist() == [1, 1, 1] and s.d2.tolist() == [2.25, 9, 0] and (s.prim == 0).all()


def test_quad_diagonal_ties_are_ordered_by_prim():
    p = np.float32([[0.5, 0.5, 0.5], [0.25, 0.25, -1]])
    for g in (nr.from_triangles(QUAD, np.repeat(UP, 2, axis=0)), split_quad()):
        for mode in (nl.GATHER, nl.K):
            s, counts = nl.near_list(g, p, np.inf, 3, mode)
            assert counts.tolist() == [2, 2]
            assert s.prim.tolist() == [0, 1, -1, 0, 1, -1] and s.d2.tolist() == [0.25, 0.25, np.inf, 1, 1, np.inf]
            assert s.point[[0, 1, 3, 4]].tolist() == [[0.5, 0.5, 0]] * 2 + [[0.25, 0.25, 0]] * 2 and s.side.tolist() == [1, 1, 0, -1, -1, 0]
        # k = 1: the smaller prim is stored, whichever triangle is found first
        ev = {}
        s, counts = nl.near_list(g, p, np.inf, 1, nl.K, events=ev)
        assert s.prim.tolist() == [0, 0] and counts.tolist() == [1, 1] and s.d2.tolist() == [0.25, 1]
        s, counts = nl.near_list(g, p, np.inf, 1, nl.GATHER)
        assert s.prim.tolist() == [0, 0] and counts.tolist() == [2, 2]
    # under the split tree triangle 1 is found first (nearest keeps it), and the search bound's <= lets the equal box in: an eviction
    assert nr.nearest(split_quad(), p).prim.tolist() == [1, 1] and ev["evicted"].all()
    assert nr.nearest(nr.from_triangles(QUAD), p).prim.tolist() == [0, 0]


def test_nan_inputs_zero_area_triangles_and_an_empty_scene():
    g = nr.from_triangles(TRI, UP)
    pts = np.float32([h[0] for h in HAND])
    for mode in (nl.GATHER, nl.K):
        for k in range(3):                                                          # a NaN coordinate: never listed
            p = np.float32([[0.25, 0.25, 1]])
            p[0, k] = np.nan
            s, counts = nl.near_list(g, p, 2.0, 2, mode)
            assert counts.tolist() == [0]
            assert_miss_slots(s, 4.0)
        s, counts = nl.near_list(g, pts, np.nan, 2, mode)                           # a NaN radius: r2 is some NaN, nothing is listed
        assert not counts.any() and np.isnan(s.d2).all() and (s.prim == -1).all() and (bits(s.point) == 0).all() and (bits(s.side) == 0).all()
        s, counts = nl.near_list(nr.from_triangles(np.zeros((0, 3, 3))), pts, 3.0, 2, mode)
        assert not counts.any()
        assert_miss_slots(s, 9.0)
        # test_nearest_ref.py's sliver (v0 = v1: its matching case divides 0 by 0) is never listed, wherever it stands in the leaf
        sliver = np.float32([[0, 0, 1], [0, 0, 1], [2, 0, 1]])
        for tris, good in ((np.stack([sliver, TRI[0]]), 1), (np.stack([TRI[0], sliver]), 0)):
            s, counts = nl.near_list(nr.from_triangles(tris, np.repeat(UP, 2, axis=0)), np.float32([[0.25, 0.25, 0.875]]), np.inf, 2, mode)
            assert counts.tolist() == [1] and s.prim.tolist() == [good, -1] and s.d2.tolist() == [0.765625, np.inf]
        # v1 = v2 counts as the segment it is
        seg = np.float32([[[0, 0, 0], [2, 0, 0], [2, 0, 0]]])
        s, counts = nl.near_list(nr.from_triangles(seg, UP), np.float32([[1, 1, 0]]), np.inf, 1, mode)
        assert counts.tolist() == [1] and s.d2.tolist() == [1] and s.point.tolist() == [[1, 0, 0]]


def test_offsets_give_capacities_as_list_hits_rule_does():
    assert nl.caps_of([0, 2, 2, 7, 5, 9], 100).tolist() == [2, 0, 5, 0, 4]          # equal and decreasing pairs give 0
    assert nl.caps_of([0, 2, 2, 7, 5, 9], 6).tolist() == [2, 0, 4, 0, 1]            # clamped: offsets[i] + cap_i <= capacity
    assert nl.caps_of([8, 9, 3], 6).tolist() == [0, 0] and nl.caps_of([0, 4], 0).tolist() == [0]


@pytest.fixture(scope="module", params=["soup", "cornell_box"])
def case(request):
    if request.param == "soup":
        osc = nr.oracle_soup(3000, 5, 2, 8)
        assert oracle.tree_depth(osc.nodes) >= 12
    else:
        osc = oracle.Scene.load_glb(scene_path("cornell_box")).build_bvh(20, 8)
    g = nr.from_oracle(osc)
    pts = nr.point_sets(g, 400, np.random.default_rng(3))
    lo, hi = nr.bounds(g)
    return request.param, g, pts, float((hi - lo).max())


def test_capacity_zero_uneven_capacities_and_what_the_insert_meets(case):
    name, g, pts, extent = case
    n = len(pts)
    radius = np.float32(0.3 * extent)
    whole, totals, _ = nl.brute_force(g, pts, radius, 0, nl.GATHER)
    assert totals.max() >= 8 and (totals == 0).any()
    # capacity 0: GATHER counts and stores nothing; K visits nothing and counts 0
    visits = np.zeros(n, np.int64)
    s, counts = nl.near_list(g, pts, radius, 0, nl.K, visits=visits)
    assert len(s.d2) == 0 and not counts.any() and not visits.any()
    s, counts = nl.near_list(g, pts, radius, 0, nl.GATHER, visits=visits)
    assert len(s.d2) == 0 and visits.any()
    assert (counts != totals).sum() <= 0.005 * n
    # uneven capacities 0 .. 9, zeros included: each segment is the list at its own capacity
    rng = np.random.default_rng(9)
    caps = rng.integers(0, 10, n)
    caps[rng.integers(0, n, n // 8)] = 0
    assert (caps == 0).sum() >= n // 16 and (caps < totals).any() and (caps > totals).any()
    for mode in (nl.GATHER, nl.K):
        ev = {}
        got, counts = nl.near_list(g, pts, radius, caps, mode, events=ev)
        ref, ref_counts, _ = nl.brute_force(g, pts, radius, caps, mode)
        bad = nl.differing_points(got, ref, caps) | (counts != ref_counts)
        assert bad.sum() <= 0.005 * n, (name, mode, bad.sum())
        # the inputs really produce inserts before a stored record and into a full list
        assert ev["out_of_order"].sum() >= n // 20 and ev["evicted"].sum() >= n // 20, (name, mode, ev["out_of_order"].sum(), ev["evicted"].sum())
        owner = np.repeat(np.arange(n), caps)
        slot = np.arange(len(owner)) - np.repeat(np.concatenate([[0], np.cumsum(caps)])[:-1], caps)
        stored = slot < np.minimum(caps, counts if mode == nl.K else np.minimum(counts, caps))[owner]
        assert_miss_slots(take(got, ~stored), np.repeat(np.float32(radius) * np.float32(radius), (~stored).sum()))
        # in order: ascending d2, equal d2 by ascending prim
        nxt = stored[1:] & stored[:-1] & (owner[1:] == owner[:-1])
        assert nl.comes_before(got.d2[:-1][nxt], got.prim[:-1][nxt], got.d2[1:][nxt], got.prim[1:][nxt]).all()


@pytest.mark.parametrize("frac", [0.02, 0.1, 0.3])
def test_gather_equals_the_float32_brute_force(case, frac):
    name, g, pts, extent = case
    n = len(pts)
    radius = np.float32(frac * extent)
    _, totals, _ = nl.brute_force(g, pts, radius, 0, nl.GATHER)
    ref, ref_counts, _ = nl.brute_force(g, pts, radius, totals, nl.GATHER)
    _, counts = nl.near_list(g, pts, radius, 0, nl.GATHER)
    got, counts2 = nl.near_list(g, pts, radius, totals, nl.GATHER)                   # the fill at the brute force's totals
    bad = nl.differing_points(got, ref, totals.astype(np.int64)) | (counts != ref_counts) | (counts2 != ref_counts)
    print("%s radius %.2f: differs on %d of %d points, mean count %.2f, max %d" % (name, frac, bad.sum(), n, totals.mean(), totals.max()))
    assert bad.sum() <= 0.005 * n                      # pruning with fp32 boxes need not be exactly conservative
    assert totals.max() >= 2


@pytest.mark.parametrize("k", [1, 4, 8])
def test_k_nearest_equals_the_float32_brute_force_and_slot_0_is_nearest(case, k):
    name, g, pts, extent = case
    n = len(pts)
    ref, ref_counts, tied = nl.brute_force(g, pts, np.inf, k, nl.K)
    visits = np.zeros(n, np.int64)
    got, counts = nl.near_list(g, pts, np.inf, k, nl.K, visits=visits)
    bad = nl.differing_points(got, ref, np.full(n, k)) | (counts != ref_counts)
    print("%s k = %d: differs on %d of %d points, %.1f nodes visited per point of %d" % (name, k, bad.sum(), n, visits.mean(), len(g.bmin)))
    assert bad.sum() <= 0.005 * n                      # pruning with fp32 boxes need not be exactly conservative
    assert (counts == min(k, len(g.v0))).all()
    # slot 0 has the nearest query's d2, bit for bit; its prim may differ only where the brute force shows an exact tie
    near_visits = np.zeros(n, np.int64)
    one = nr.nearest(g, pts, visits=near_visits)
    first = take(got, slice(0, None, k))
    assert (bits(first.d2) == bits(one.d2)).all()
    other = first.prim != one.prim
    print("%s k = %d: slot 0's prim is not nearest's on %d points, all ties: %s" % (name, k, other.sum(), bool(tied[other].all())))
    assert tied[other].all() and (first.prim[other] < one.prim[other]).all()
    if name == "soup":
        assert not other.any()
    if k == 1:
        # mode K prunes: at k = 1 the bound is nearest's `best` but for the <= (an equal box is still visited).  Measured on these
        # inputs, nodes visited per point: soup 17.40 against nearest's 17.17, of 3617 nodes; cornell_box 4.03 against 3.37, of 5 --
        # its walls share edges, and the tie points sit on them.
        print("%s k = 1: %.2f nodes visited per point, nearest %.2f, of %d" % (name, visits.mean(), near_visits.mean(), len(g.bmin)))
        assert (visits >= near_visits).all()
        if name == "soup":
            assert visits.mean() < 0.05 * len(g.bmin) and visits.mean() <= 1.05 * near_visits.mean()


@pytest.mark.parametrize("frac", [0.1, 0.3])
def test_mode_k_stores_what_gather_stores_at_the_same_capacity(case, frac):
    name, g, pts, extent = case
    n, k = len(pts), 4
    radius = np.float32(frac * extent)
    a, ca = nl.near_list(g, pts, radius, k, nl.K)
    b, cb = nl.near_list(g, pts, radius, k, nl.GATHER)
    bad = nl.differing_points(a, b, np.full(n, k)) | (ca != np.minimum(cb, k))
    print("%s radius %.2f: the modes differ on %d of %d points" % (name, frac, bad.sum(), n))
    assert bad.sum() <= 0.005 * n
    assert (cb > k).any() and (cb < k).any()
