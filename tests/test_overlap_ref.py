"""The box overlap rule of include/drt.h as tests/overlap_ref.py restates it (CPU only): hand-derived cases that separate one group of
axes each, rotated against axis-aligned boxes, NaN and infinite inputs, zero-area triangles, points, capacities and segments, and the
traversal against the brute force -- a subset always, equal where that can be derived."""
import numpy as np
import pytest

import oracle
from tests import nearest_ref as nr
from tests import overlap_ref as ov
from tests import ray_query_ref as rq
from tests import refit_ref as rf
from tests.scenes import scene_path

TRI = np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])               # the unit triangle
SLANT = np.float32([[[1, 0, 0], [0, 1, 0], [0, 0, 1]]])             # the plane x + y + z = 1
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def listed(g, boxes):
    """bool [N]: box i lists triangle 0 of a one-triangle scene -- by the traversal, in both modes, and by the brute force."""
    prims, counts = ov.overlap(g, boxes, 1)
    _, anyc = ov.overlap(g, boxes, 0, ov.ANY)
    bprims, bcounts = ov.brute_force(g, boxes, 1)
    assert (counts == anyc).all() and (prims == np.where(counts > 0, 0, -1)).all()
    assert (bcounts >= counts).all()
    return counts > 0, bcounts > 0


def axes_ok(g, boxes):
    return ov.triangle_axes(*ov.unpack(boxes), g.v0, g.e1, g.e2)


def test_unit_triangle_by_hand():
    g = nr.from_triangles(TRI)
    boxes = ov.pack([[0.25, 0.25, 0], [0.75, 0.75, 0], [0.75, 0.75, 0]], [[0.125] * 3, [0.125] * 3, [0.25] * 3])
    got, brute = listed(g, boxes)
    assert got.tolist() == [True, False, True] and brute.tolist() == [True, False, True]
    ok = axes_ok(g, boxes)
    assert ok[0].all() and ok[2].all()
    # box 1: the boxes' AABBs overlap ([0.625, 0.875]^2 against [0, 1]^2) and the plane z = 0 cuts the box; only the hypotenuse's
    # edge axis separates.  g = f2 - f1 = (-1, 1, 0), k = 2: L = (-g.y, g.x, 0) = (-1, -1, 0); s_i = -(x_i + y_i) of the vertices
    # relative to the centre, (-0.75, -0.75), (0.25, -0.75), (-0.75, 0.25): 1.5, 0.5, 0.5; r = 0.125 + 0.125 = 0.25 and
    # min s = 0.5 > 0.25.  It is axis 3 + 1 + 3 + 2 = 9 of the 13.
    assert ok[1].tolist() == [True] * 9 + [False] + [True] * 3
    # box 2 touches: r = 0.25 + 0.25 = 0.5 and min s = 0.5 <= 0.5


def test_only_the_plane_separates():
    g = nr.from_triangles(SLANT)
    boxes = ov.pack([[0, 0, 0]] * 2, [[0.25] * 3, [0.375] * 3])
    got, brute = listed(g, boxes)
    assert got.tolist() == [False, True] and brute.tolist() == [False, True]
    # n = cross((-1, 1, 0), (-1, 0, 1)) = (1, 1, 1), d = dot(n, (1, 0, 0)) = 1; r = 3 half: 0.75 < 1 <= 1.125
    ok = axes_ok(g, boxes)
    assert ok[0].tolist() == [True] * 3 + [False] + [True] * 9 and ok[1].all()


def test_a_rotated_box_is_not_its_axis_aligned_box():
    g = nr.from_triangles(TRI)
    c = [0.75, 0.75, 0]
    # The box is turned 45 degrees about z: axis 0 = (1, 1, 0) / sqrt 2 is the diagonal, perpendicular to the hypotenuse x + y = 1,
    # whose distance from the centre is (0.75 + 0.75 - 1) / sqrt 2 = 0.35355.  Along axis 0 every point of the triangle projects to
    # (x + y - 1.5) / sqrt 2 <= -0.35355, so the long half-length 0.3125 leaves the triangle outside (box axis 0 separates) and
    # 0.40625 reaches it: the box then holds (0.5, 0.5, 0), the hypotenuse's midpoint.  The margins, 0.04 and 0.05, are far beyond
    # the rounding of sqrt 0.5 in float32.
    s = np.float32(np.sqrt(0.5))
    turned = np.float32([[s, s, 0], [-s, s, 0], [0, 0, 1]])
    short, long_ = [0.3125, 0.0625, 0.125], [0.40625, 0.0625, 0.125]
    boxes = ov.pack([c, c], [short, long_], turned)
    got, brute = listed(g, boxes)
    assert got.tolist() == [False, True] and brute.tolist() == [False, True]
    # (the hypotenuse's edge axis cross(unit_2, g), axis 9, is parallel to box axis 0 and separates with it; no other does)
    assert np.nonzero(~axes_ok(g, boxes)[0])[0].tolist() == [0, 9]
    # the axis-aligned box of the same extents: x in [0.75 - h0, 0.75 + h0], y in [0.6875, 0.8125], so min (x + y) = 1.4375 - h0:
    # 1.125 and 1.03125, both beyond the hypotenuse -- the long one answers differently
    got, brute = listed(g, ov.pack([c, c], [short, long_]))
    assert got.tolist() == [False, False] and brute.tolist() == [False, False]
    # axes are used as given, not normalised: with axis 0 = (1, 1, 0) and axis 1 = (-1, 1, 0) every product is exact, the box is
    # |x + y - 1.5| <= half[0], |y - x| <= half[1], and the hypotenuse is at exactly 0.5: touching counts
    raw = np.float32([[1, 1, 0], [-1, 1, 0], [0, 0, 1]])
    boxes = ov.pack([c] * 3, [[0.375, 0.125, 0.125], [0.5, 0.125, 0.125], [0.625, 0.125, 0.125]], raw)
    qmin, qmax = ov.world_bounds(boxes)
    assert qmin[1].tolist() == [0.125, 0.125, -0.125] and qmax[1].tolist() == [1.375, 1.375, 0.125]          # ext = half[0] + half[1]
    got, brute = listed(g, boxes)
    assert got.tolist() == [False, True, True] and brute.tolist() == [False, True, True]


def test_nan_and_infinite_queries_and_an_empty_scene_list_nothing():
    g = nr.from_triangles(TRI)
    good = ov.pack([[0.25, 0.25, 0]], [[0.125] * 3])
    assert listed(g, good)[0].tolist() == [True]
    for word in list(range(0, 6)) + [6, 7, 10, 11, 14]:                        # the centre, the half, some of the axes
        bad = good.copy()
        bad[0, word] = NAN
        qmin, qmax = ov.world_bounds(bad)
        assert np.isnan(qmin).any() and np.isnan(qmax).any()
        visits = np.zeros(1, np.int64)
        prims, counts = ov.overlap(g, bad, 2, visits=visits)
        assert counts.tolist() == [0] and prims.tolist() == [-1, -1] and not visits.any(), word      # the root fails
        assert ov.overlap(g, bad, 0, ov.ANY)[1].tolist() == [0]
    pad = good.copy()
    pad[0, 15] = NAN                                                           # the pad word is ignored
    assert listed(g, pad)[0].tolist() == [True]
    # an infinite half beside a zero axis component: 0 * inf = NaN in ext
    inf = good.copy()
    inf[0, 3] = INF
    assert np.isnan(ov.world_bounds(inf)[0]).any()
    assert ov.overlap(g, inf, 1)[1].tolist() == [0] and ov.overlap(g, inf, 0, ov.ANY)[1].tolist() == [0]
    # an empty scene
    empty = nr.from_triangles(np.zeros((0, 3, 3)))
    prims, counts = ov.overlap(empty, good, 3)
    assert prims.tolist() == [-1] * 3 and counts.tolist() == [0]
    assert ov.overlap(empty, good, 0, ov.ANY)[1].tolist() == [0] and ov.brute_force(empty, good, 3)[1].tolist() == [0]
    # no boxes
    prims, counts = ov.overlap(g, np.zeros((0, 16), np.float32), 2)
    assert len(prims) == 0 and len(counts) == 0 and counts.dtype == np.uint32 and prims.dtype == np.int32


def test_zero_area_triangles_points_and_flat_boxes():
    # a segment (v1 = v2) from (0, 0, 0) to (2, 0, 0): cross(f1, f2) = 0 and the edge axes of g = 0 vanish, passed with 0 <= 0;
    # the box axes and the edge axes of f1 decide
    seg = nr.from_triangles(np.float32([[[0, 0, 0], [2, 0, 0], [2, 0, 0]]]))
    boxes = ov.pack([[1, 0, 0], [1, 0.5, 0], [1, 0.25, 0], [3, 0, 0]], [[0.25] * 3] * 4)
    got, brute = listed(seg, boxes)
    assert got.tolist() == [True, False, True, False] and brute.tolist() == [True, False, True, False]      # through, beside, touching, beyond
    ok = axes_ok(seg, boxes)
    assert ok[:, 3].all() and ok[:, 7:10].all()                               # the plane and g's axes: 0 <= 0
    # a point (v0 = v1 = v2)
    dot = nr.from_triangles(np.float32([[[1, 1, 1]] * 3]))
    got, _ = listed(dot, ov.pack([[1, 1, 1], [1, 1, 1.5], [1, 1, 1.5]], [[0, 0, 0], [0.25] * 3, [0.5] * 3]))
    assert got.tolist() == [True, False, True]
    # half = 0 on a vertex, on an edge, in the face, off the plane and outside the triangle in its plane
    g = nr.from_triangles(TRI)
    pts = [[1, 0, 0], [0.5, 0.5, 0], [0.25, 0.25, 0], [0.25, 0.25, 0.125], [0.75, 0.75, 0]]
    got, brute = listed(g, ov.pack(pts, 0.0))
    assert got.tolist() == [True, True, True, False, False] and brute.tolist() == got.tolist()
    # a flat box (half.z = 0) in the triangle's plane and one above it
    got, _ = listed(g, ov.pack([[0.25, 0.25, 0], [0.25, 0.25, 0.125]], [[0.125, 0.125, 0]] * 2))
    assert got.tolist() == [True, False]


def test_corners_give_centre_and_half_in_float32():
    b = ov.from_corners([[0.5, -1, 0.25]], [[1.5, 3, 0.25]])
    assert b[0, :6].tolist() == [1, 1, 0.25, 0.5, 2, 0] and b[0, 6:15].reshape(3, 3).tolist() == np.eye(3).tolist() and b[0, 15] == 0


def fan(n=6):
    """n triangles that all contain the z axis' point (0, 0, k / 8), one per leaf-sized step, so that one box meets all of them."""
    k = np.arange(n, dtype=np.float32) / np.float32(8)
    p = np.zeros((n, 3, 3), np.float32)
    p[:, 0] = np.stack([-np.ones(n), -np.ones(n), k], axis=1)
    p[:, 1] = np.stack([np.ones(n), -np.ones(n), k], axis=1)
    p[:, 2] = np.stack([np.zeros(n), np.ones(n), k], axis=1)
    return nr.from_triangles(p)


def test_capacities_the_prefix_property_and_segments():
    g = fan(6)
    boxes = ov.pack([[0, 0, 0.25], [0, 0, 0.5], [5, 5, 5], [0, 0, 0.0625]], [[0.125] * 3, [1.0] * 3, [0.125] * 3, [0.03125] * 3])
    whole, totals = ov.overlap(g, boxes, 6)
    assert totals.tolist() == [3, 6, 0, 0]                                      # z in [0.125, 0.375]: triangles 1, 2, 3; all; none; between two
    assert whole.reshape(4, 6).tolist() == [[1, 2, 3, -1, -1, -1], [0, 1, 2, 3, 4, 5], [-1] * 6, [-1] * 6]
    for cap in (0, 1, 3, 4, 9):                                                 # 0, 1, the exact count of box 0, more
        prims, counts = ov.overlap(g, boxes, cap)
        assert (counts == totals).all()                                         # the total, so truncation shows
        rows = prims.reshape(4, cap)
        full = np.full((4, max(cap, 6)), -1, np.int32)
        full[:, :6] = whole.reshape(4, 6)
        assert (rows == full[:, :cap]).all(), cap                               # the first K of a longer list are the list at capacity K
        bp, bc = ov.brute_force(g, boxes, cap)
        assert (bp == prims).all() and (bc == counts).all()
    # uneven capacities
    prims, counts = ov.overlap(g, boxes, [2, 0, 1, 3])
    assert prims.tolist() == [1, 2, -1, -1, -1, -1] and (counts == totals).all()
    # mode ANY: 0 or 1, and no slots
    prims, counts = ov.overlap(g, boxes, 4, ov.ANY)
    assert len(prims) == 0 and counts.tolist() == [1, 1, 0, 0] and counts.dtype == np.uint32
    # segments from offsets, as drt_renderer_list_hits has them: equal and decreasing pairs give 0, the capacity clamps
    assert ov.caps_of([0, 2, 2, 7, 5, 9], 100).tolist() == [2, 0, 5, 0, 4]
    assert ov.caps_of([0, 2, 2, 7, 5, 9], 6).tolist() == [2, 0, 4, 0, 1]
    assert ov.caps_of([8, 9, 3], 6).tolist() == [0, 0] and ov.caps_of([0, 4], 0).tolist() == [0]
    # out-of-order offsets: box 0 owns [4, 7), box 1 nothing (7 -> 0 decreases), box 2 owns [0, 4) clamped by nothing
    off = [4, 7, 0, 4]
    caps = ov.caps_of(off, 7)
    assert caps.tolist() == [3, 0, 4]
    prims, counts = ov.overlap(g, boxes[[1, 0, 0]], caps)
    assert prims.tolist() == [0, 1, 2, 1, 2, 3, -1] and counts.tolist() == [6, 3, 3]


def dyadic_soup(n, seed, leaf=2):
    """n small triangles whose coordinates are all multiples of 2^-6 in [-4, 4), under the oracle's tree."""
    rng = np.random.default_rng(seed)
    base = rng.integers(-200, 200, (n, 1, 3))
    pos = ((base + rng.integers(-24, 25, (n, 3, 3))) / 64.0).astype(np.float32)
    assert (pos >= -4).all() and (pos < 4).all() and (pos * 64 == np.round(pos * 64)).all()
    _, nrm, uv, mat, materials, textures = rq.soup(n, seed)
    return nr.from_oracle(oracle.Scene(rf.triangles(pos, nrm, uv, mat), materials, textures).build_bvh(leaf, 8))


def dyadic_boxes(n, seed):
    """Axis-aligned boxes with dyadic centres and halves, from points (half = 0) to the whole scene, inside [-4, 4)."""
    rng = np.random.default_rng(seed)
    half = rng.choice([0, 1, 2, 8, 24, 64], (n, 3)) / 64.0
    half[: n // 8] = half[: n // 8, :1]                                         # some cubes
    half[-2:] = 2.0
    center = rng.integers(-120, 121, (n, 3)) / 64.0
    center[-2:] = [[0, 0, 0], [1.5, -1.5, 0.5]]                                 # [-2, 2]^3, and a box that reaches 3.5
    boxes = ov.pack(center, half)
    lo, hi = ov.world_bounds(boxes)
    assert (lo >= -4).all() and (hi < 4).all()
    return boxes


def missed_by_the_traversal(g, boxes):
    """(pairs the brute force lists, pairs the traversal lists), after asserting the subset exactly and the counts' consistency."""
    _, totals = ov.overlap(g, boxes, 0)
    prims, counts = ov.overlap(g, boxes, totals)
    assert (counts == totals).all()
    _, btotals = ov.brute_force(g, boxes, 0)
    bprims, _ = ov.brute_force(g, boxes, btotals)
    mine, brute = ov.pair_sets(prims, totals), ov.pair_sets(bprims, btotals)
    assert mine <= brute                                                        # the cull only ever removes
    assert (ov.overlap(g, boxes, 0, ov.ANY)[1] == (totals > 0)).all()           # ANY is LIST's count > 0
    return brute, mine


def test_on_dyadic_inputs_the_traversal_equals_the_brute_force():
    """Coordinates that are multiples of 2^-6 in [-4, 4) and axis-aligned boxes: every subtraction and v0 + e1 is exact, a node's box
    holds its triangles' real vertices, and a triangle that passes the three box axes has an AABB that meets (qmin, qmax), so every
    ancestor's box passes the cull: nothing the brute force lists can be missed."""
    g = dyadic_soup(600, 3)
    boxes = dyadic_boxes(160, 4)
    _, totals = ov.overlap(g, boxes, 0)
    brute, mine = missed_by_the_traversal(g, boxes)
    assert brute == mine
    assert totals.max() >= 100 and (totals == 0).any() and (totals == 1).any()


def test_the_list_does_not_depend_on_the_order_in_which_the_leaves_arrive():
    """The builder lays a node's triangles out with child 1's first, and child 1 is popped first, so on its trees the triangles of a
    box arrive in ascending order: every insert is an append and a full list takes nothing more.  The rule does not depend on that:
    with the children of every node exchanged the triangles arrive in descending runs, capacity 4 meets inserts before stored
    records and evictions, and every slot and count is the same."""
    g = dyadic_soup(600, 3)
    boxes = dyadic_boxes(160, 4)
    swapped = g._replace(child1=g.child2, child2=g.child1)
    for caps in (4, 1, np.random.default_rng(1).integers(0, 9, len(boxes))):
        ev, ev_swapped = {}, {}
        prims, counts = ov.overlap(g, boxes, caps, events=ev)
        prims2, counts2 = ov.overlap(swapped, boxes, caps, events=ev_swapped)
        assert (prims == prims2).all() and (counts == counts2).all()
        assert not ev["out_of_order"].any() and not ev["evicted"].any()
        assert ev_swapped["evicted"].sum() >= 5                                 # (that they occur, not how often)
        if not np.isscalar(caps) or caps > 1:                                   # (a list of one slot has no middle)
            assert ev_swapped["out_of_order"].sum() >= 5
        assert (ov.overlap(swapped, boxes, 0, ov.ANY)[1] == (counts > 0)).all()


@pytest.mark.parametrize("name", ["cornell_box", "soup"])
def test_elsewhere_the_traversal_lists_a_subset_of_the_brute_force(name):
    """Random floats and rotated boxes: v0 + e1 can round outside a node box built from the real v1, so the subset is asserted and the
    number of pairs the traversal misses is measured and printed, not asserted against a figure (DESIGN 5.20 records it)."""
    if name == "soup":
        g = nr.from_oracle(nr.oracle_soup(3000, 5, 2, 8))
    else:
        g = nr.from_oracle(oracle.Scene.load_glb(scene_path("cornell_box")).build_bvh(20, 8))
    rng = np.random.default_rng(7)
    n = 300
    lo, hi = nr.bounds(g)
    extent = np.float32((hi - lo).max())
    center = np.concatenate([nr.surface_points(g, n // 2, rng), nr.tie_points(g, n // 4, rng), nr.box_points(g, n // 4, rng)])
    half = (rng.uniform(0, 1, (n, 3)) ** 3 * 0.2 * extent).astype(np.float32)
    half[::10] = 0                                                              # points on vertices, edges and near surfaces
    q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    axes = q.astype(np.float32)
    axes[::2] = np.eye(3, dtype=np.float32)                                     # every other box axis-aligned
    boxes = ov.pack(center, half, axes)
    brute, mine = missed_by_the_traversal(g, boxes)
    print("%s: the brute force lists %d (box, triangle) pairs over %d boxes, the traversal misses %d of them" % (name, len(brute), n, len(brute - mine)))
    assert len(mine) > n
