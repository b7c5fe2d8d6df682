"""The nearest-surface rule of include/drt.h as tests/nearest_ref.py restates it (CPU only): hand-derived cases on one triangle,
the miss record, and on a deep triangle soup and cornell_box the float32 brute-force minimum and the float64 distance."""
import numpy as np
import pytest

import oracle
from tests import nearest_ref as nr
from tests.scenes import scene_path

TRI = np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
UP = np.float32([[0, 0, 1]])

# (point, u, v, closest point, d2, side): one point in each of the seven regions of the rule's case chain, one on the plane inside
# the triangle, one exactly on a vertex.  All values are exact in float32.
HAND = [
    ((-1, -1, 1), 0, 0, (0, 0, 0), 3, 1),                    # 1: vertex v0
    ((2, -0.5, -1), 1, 0, (1, 0, 0), 2.25, -1),              # 2: vertex v1
    ((0.25, -1, 0), 0.25, 0, (0.25, 0, 0), 1, 1),            # 3: edge v0 v1 (in the plane: dot = 0 is not < 0)
    ((-0.5, 2, 1), 0, 1, (0, 1, 0), 2.25, 1),                # 4: vertex v2
    ((-1, 0.5, 0), 0, 0.5, (0, 0.5, 0), 1, 1),               # 5: edge v0 v2
    ((1, 1, -2), 0.5, 0.5, (0.5, 0.5, 0), 4.5, -1),          # 6: edge v1 v2
    ((0.25, 0.25, 3), 0.25, 0.25, (0.25, 0.25, 0), 9, 1),    # 7: the face
    ((0.25, 0.5, 0), 0.25, 0.5, (0.25, 0.5, 0), 0, 1),       # on the plane, inside
    ((1, 0, 0), 1, 0, (1, 0, 0), 0, 1),                      # exactly on v1
]


def assert_miss(res, max_dist):
    md = np.float32(max_dist)
    with np.errstate(all="ignore"):
        want = md * md
    assert (res.prim == -1).all()
    assert (res.d2.view(np.uint32) == np.full(res.d2.shape, want, np.float32).view(np.uint32)).all() or (np.isnan(want) and np.isnan(res.d2).all())
    for f in (res.point, res.u, res.v, res.side):
        assert (f.view(np.uint32) == 0).all()


def test_hand_derived_regions_of_one_triangle():
    g = nr.from_triangles(TRI, UP)
    pts = np.float32([h[0] for h in HAND])
    res = nr.nearest(g, pts)
    assert (res.prim == 0).all()
    assert res.u.tolist() == [h[1] for h in HAND] and res.v.tolist() == [h[2] for h in HAND]
    assert res.point.tolist() == [list(map(float, h[3])) for h in HAND]
    assert res.d2.tolist() == [h[4] for h in HAND] and res.side.tolist() == [h[5] for h in HAND]
    for dtype in (np.float32, np.float64):
        best, prim = nr.brute_force(g, pts, dtype=dtype)
        assert best.dtype == dtype and best.tolist() == [h[4] for h in HAND] and (prim == 0).all()


def test_a_zero_area_triangle_never_wins():
    """v0 = v1: the point projects between v0 and v2, case 3 matches (vc = 0 <= 0, d1 = 0 >= 0, d3 = 0 <= 0) and divides 0 by 0: u,
    and with it dist2, is NaN, and NaN < best is false.  The good triangle wins although the sliver's segment is nearer, whichever of
    the two comes first in the leaf."""
    sliver = np.float32([[0, 0, 1], [0, 0, 1], [2, 0, 1]])
    for tris, good in ((np.stack([sliver, TRI[0]]), 1), (np.stack([TRI[0], sliver]), 0)):
        g = nr.from_triangles(tris, np.repeat(UP, 2, axis=0))
        p = np.float32([[0.25, 0.25, 0.875]])
        d2, *_ = nr.closest_on_triangle(p, g.v0[1 - good][None], g.e1[1 - good][None], g.e2[1 - good][None])
        assert np.isnan(d2).all()
        res = nr.nearest(g, p)
        assert res.prim.tolist() == [good] and res.d2.tolist() == [0.765625] and res.point.tolist() == [[0.25, 0.25, 0.0]]
        assert (res.u.tolist(), res.v.tolist(), res.side.tolist()) == ([0.25], [0.25], [1.0])
        assert nr.brute_force(g, p)[1].tolist() == [good]
    # alone, it is a miss
    assert_miss(nr.nearest(nr.from_triangles(sliver[None], UP), p), np.inf)


def test_miss_records():
    g = nr.from_triangles(TRI, UP)
    pts = np.float32([h[0] for h in HAND])
    assert_miss(nr.nearest(g, pts, 0.0), 0.0)                                     # max_dist = 0: not even the points on the triangle
    res = nr.nearest(g, pts, 1.25)                                                # a finite radius: d2 < 1.5625 only
    inside = np.float32([h[4] for h in HAND]) < np.float32(1.5625)
    assert inside.sum() == 4 and (res.prim == np.where(inside, 0, -1)).all()
    assert_miss(nr.Nearest(*[f[~inside] for f in res]), 1.25)
    radius = np.float32([0.5, 3, 1, 1, 1.5, 2, 2.5, 0, 1e-3])                     # per point: d2 < radius^2, strictly
    res = nr.nearest(g, pts, radius)
    assert res.prim.tolist() == [-1, 0, -1, -1, 0, -1, -1, -1, 0]
    assert res.d2.tolist() == [0.25, 2.25, 1, 1, 1, 4, 6.25, 0, 0]
    for k in range(3):                                                            # a NaN coordinate
        p = np.float32([[0.25, 0.25, 1]])
        p[0, k] = np.nan
        assert_miss(nr.nearest(g, p), np.inf)
        assert_miss(nr.nearest(g, p, 2.0), 2.0)
    assert_miss(nr.nearest(g, pts[:2], np.nan), np.nan)
    assert_miss(nr.nearest(nr.from_triangles(np.zeros((0, 3, 3))), pts, 3.0), 3.0)  # an empty scene


# The measured largest |sqrt(d2) - d64| / (2^-23 M) of the restatement on exactly these inputs (seed 3, 600 points each):
#   soup 0.7413, cornell_box 0.5729.  B = four times the larger one; the margin covers other seeds.
B_MEASURED = 0.7413
B = 4 * B_MEASURED


@pytest.fixture(scope="module", params=["soup", "cornell_box"])
def case(request):
    if request.param == "soup":
        osc = nr.oracle_soup(3000, 5, 2, 8)
        assert oracle.tree_depth(osc.nodes) >= 12
    else:
        osc = oracle.Scene.load_glb(scene_path("cornell_box")).build_bvh(20, 8)
    g = nr.from_oracle(osc)
    rng = np.random.default_rng(3)
    pts = np.concatenate([nr.surface_points(g, 200, rng), nr.box_points(g, 200, rng), nr.box_points(g, 200, rng, 10.0)])
    visits = np.zeros(len(pts), np.int64)
    return request.param, g, pts, nr.nearest(g, pts, visits=visits), visits


def test_tree_answer_is_the_float32_brute_force_minimum(case):
    name, g, pts, res, visits = case
    best, prim = nr.brute_force(g, pts, dtype=np.float32)
    differs = res.d2.view(np.uint32) != best.view(np.uint32)
    print("%s: d2 differs from the float32 brute force on %d of %d points, %.1f nodes visited per point" % (name, differs.sum(), len(pts), visits.mean()))
    assert differs.sum() <= 0.005 * len(pts)           # pruning with fp32 boxes need not be exactly conservative
    assert (res.prim >= 0).all()
    # the winner's own distance is the one reported (prim may differ from the brute force's only on an exact tie)
    same = ~differs
    d2, u, v, c = nr.closest_on_triangle(pts, g.v0[res.prim], g.e1[res.prim], g.e2[res.prim])
    assert (d2.view(np.uint32) == res.d2.view(np.uint32)).all() and (c.view(np.uint32) == res.point.view(np.uint32)).all()
    if name == "soup":                                  # (cornell_box's walls share edges: exact ties, and 34 triangles are no tree to speak of)
        assert (res.prim[same] == prim[same]).all()
        assert visits.mean() < 0.05 * len(g.bmin)


def test_distance_is_within_B_ulps_of_the_float64_distance(case):
    name, g, pts, res, _ = case
    best64, _ = nr.brute_force(g, pts, dtype=np.float64)
    err = np.abs(np.sqrt(res.d2.astype(np.float64)) - np.sqrt(best64)) / (2.0 ** -23 * nr.scale_of(g, pts))
    print("%s: largest |sqrt(d2) - d64| / (2^-23 M) = %.4f (B = %.4f)" % (name, err.max(), B))
    assert (err <= B).all()


def test_radius_and_order_do_not_change_an_answer(case):
    name, g, pts, res, _ = case
    radius = np.sqrt(res.d2.astype(np.float64)).astype(np.float32) * np.float32(1.5) + np.float32(1e-3)
    again = nr.nearest(g, pts, radius)
    perm = np.random.default_rng(1).permutation(len(pts))
    shuffled = nr.nearest(g, pts[perm])
    for a, b, c in zip(res, again, shuffled):
        assert a.tobytes() == b.tobytes() and a[perm].tobytes() == c.tobytes()
