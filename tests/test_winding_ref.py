"""The generalised winding numbers' rule without a GPU (tests/winding_ref.py restates include/drt.h): hand cases, the fp32 rule against a
float64 brute force in exact mode and at beta = 2 and 4, the classification of closed and open meshes against the analytic shapes, and
the node moments.

Recorded on the seeded sets below (largest |w - float64 brute force| over 4 000 points in [-1.5, 1.5]^3; the tests assert twice these):

    scene        beta = inf   beta = 2    beta = 4
    cube         2.623e-06    3.127e-03   2.623e-06
    torus        1.729e-06    6.638e-02   4.609e-03
    sphere       1.252e-06    2.444e-02   2.799e-03
    degenerate   5.252e-06    6.791e-03   1.053e-03

Classification at beta = 2, threshold 0.5, points farther than 0.03 from the analytic surface: torus 143 of 4 000 left out, 0 mismatches,
smallest |w - 0.5| 0.434; sphere 134 left out, 0 mismatches, 0.477; the torus with 10 % of its triangles removed 143 left out, 0
mismatches, 0.122, first-order error at most 0.059 -- and inside_ref.votes misclassifies 29 of its 3 857 points under either rule.

The project's atan2 against float64 atan2 over 10^6 seeded pairs: 2.44e-07 absolute, 1.93e-07 relative at most.
"""
import numpy as np
import pytest

from tests import hostile_meshes as hm
from tests import inside_ref as ir
from tests import winding_ref as wr

F = np.float32
RECORDED = {"cube": {np.inf: 2.623e-06, 2.0: 3.127e-03, 4.0: 2.623e-06},
            "torus": {np.inf: 1.729e-06, 2.0: 6.638e-02, 4.0: 4.609e-03},
            "sphere": {np.inf: 1.252e-06, 2.0: 2.444e-02, 4.0: 2.799e-03},
            "degenerate": {np.inf: 5.252e-06, 2.0: 6.791e-03, 4.0: 1.053e-03}}
ATAN2_RECORDED = 2.44e-07
EXACT = 2 * 5.252e-06                            # the bound of the hand cases: twice the largest exact-mode error recorded above
_cache = {}


def scene(name):
    if name not in _cache:
        if name == "degenerate":
            _cache[name] = hm.oracle_scene(hm.degenerate())
        elif name == "open_torus":
            _cache[name] = ir.oracle_scene(open_torus(), 4)
        else:
            pos, leaf = {"cube": (ir.cube(), 2), "torus": (ir.torus(), 4), "sphere": (ir.sphere(), 4)}[name]
            _cache[name] = ir.oracle_scene(pos, leaf)
    return _cache[name]


def open_torus(seed=17):
    """inside_ref.torus() with 10 % of its triangles removed by a seeded draw."""
    pos = ir.torus()
    keep = np.ones(len(pos), bool)
    keep[np.random.default_rng(seed).choice(len(pos), len(pos) // 10, replace=False)] = False
    return pos[keep]


def points():
    return np.random.default_rng(11).uniform(-1.5, 1.5, (4000, 3)).astype(np.float32)


def test_atan2_against_float64_over_a_million_pairs():
    rng = np.random.default_rng(1)
    y = rng.normal(size=10 ** 6).astype(np.float32) * F(10.0) ** rng.integers(-6, 7, 10 ** 6).astype(np.float32)
    x = rng.normal(size=10 ** 6).astype(np.float32) * F(10.0) ** rng.integers(-6, 7, 10 ** 6).astype(np.float32)
    y[y == 0] = 1
    err = np.abs(wr.atan2(y, x).astype(np.float64) - np.arctan2(y.astype(np.float64), x.astype(np.float64))).max()
    print("atan2: largest absolute error %.3e" % err)
    assert err <= 2 * ATAN2_RECORDED
    # the axes and the diagonals, and a NaN stays a NaN
    assert abs(float(wr.atan2(F([1]), F([0]))[0]) - np.pi / 2) < 3e-7 and abs(float(wr.atan2(F([-1]), F([0]))[0]) + np.pi / 2) < 3e-7
    assert abs(float(wr.atan2(F([1]), F([-1]))[0]) - 3 * np.pi / 4) < 3e-7 and abs(float(wr.atan2(F([1e-30]), F([-1]))[0]) - np.pi) < 3e-7
    assert np.isnan(wr.atan2(F([1, np.nan, np.inf]), F([np.nan, 1, np.inf]))).all()


def test_hand_cases():
    cube = scene("cube")
    w = wr.winding(cube, F([[0, 0, 0], [40, -30, 25]]), np.inf)
    assert abs(float(w[0]) - 1) <= EXACT and abs(float(w[1])) <= EXACT
    # one triangle seen from on its axis: the vertices on the three axes subtend one octant at the origin, pi / 2 steradians
    v0, e1, e2 = F([[1, 0, 0]]), F([[-1, 1, 0]]), F([[-1, 0, 1]])
    om = wr.solid_angle(F([[0, 0, 0]]), v0, e1, e2)
    assert abs(float(om[0]) - np.pi / 2) <= 4 * np.pi * EXACT
    assert abs(float(wr.solid_angle(F([[0, 0, 0]]), v0, e2, e1)[0]) + np.pi / 2) <= 4 * np.pi * EXACT            # the other winding
    # a point in a triangle's plane gets exactly 0 from it
    flat = wr.solid_angle(F([[5, 5, 0], [0.25, 0.25, 0], [-3, 0.5, 0]]), np.tile(F([[0, 0, 0]]), (3, 1)), np.tile(F([[1, 0, 0]]), (3, 1)),
                          np.tile(F([[0, 1, 0]]), (3, 1)))
    assert (flat.view(np.uint32) == 0).all()
    # beta = 0: the root's dipole alone
    torus = scene("torus")
    mom = wr.moments(torus)
    q = F([[0.3, -0.2, 0.9], [1.0, 0.1, 0.05], [4, 4, 4]])
    d = mom[-1, 4:7] - q
    dd = wr.dot(d, d)
    want = (wr.dot(d, mom[-1, 0:3][None]) / (dd * np.sqrt(dd)) * F(wr.INV_4PI)).astype(np.float32)
    vis = np.zeros((3, 2), np.int64)
    got = wr.winding(torus, q, 0.0, mom, visits=vis)
    assert (got.view(np.uint32) == want.view(np.uint32)).all() and (vis == [1, 0]).all()
    # a NaN or an infinity answers NaN, an empty scene 0
    assert np.isnan(wr.winding(cube, F([[np.nan, 0, 0], [0, np.inf, 0]]))).all()
    empty = ir.types.SimpleNamespace(nodes=cube.nodes[:0], tris=cube.tris[:0])
    assert (wr.winding(empty, F([[0, 0, 0]])) == 0).all()


@pytest.mark.parametrize("name", ["cube", "torus", "sphere", "degenerate"])
def test_the_fp32_rule_against_a_float64_brute_force(name):
    osc, pts = scene(name), points()
    w64 = wr.brute_force64(osc.tris["p"], pts)
    mom = wr.moments(osc)
    for beta in (np.inf, 2.0, 4.0):
        vis = np.zeros((len(pts), 2), np.int64)
        w = wr.winding(osc, pts, beta, mom, visits=vis)
        err = np.abs(w.astype(np.float64) - w64).max()
        print("%s beta %s: largest |w - float64| %.3e; nodes and triangles per point %.1f, %.1f of %d" %
              (name, beta, err, vis[:, 0].mean(), vis[:, 1].mean(), len(osc.tris)))
        assert err <= 2 * RECORDED[name][beta], (name, beta, err)
        if beta == np.inf:
            assert (vis[:, 1] == len(osc.tris)).all()              # the exact sum visits every triangle


@pytest.mark.parametrize("name", ["torus", "sphere", "open_torus"])
def test_classification_against_the_analytic_shape(name):
    osc, pts = scene(name), points()
    dist = ir.sphere_distance(pts) if name == "sphere" else ir.torus_distance(pts)
    use = np.abs(dist) > 0.03
    print("%s: %d of %d points within 0.03 of the analytic surface are left out" % (name, (~use).sum(), len(pts)))
    assert (~use).sum() <= 0.05 * len(pts)
    w = wr.winding(osc, pts, 2.0)
    wrong = (w[use] >= 0.5) != (dist[use] < 0)
    err = np.abs(w.astype(np.float64) - wr.brute_force64(osc.tris["p"], pts)).max()
    print("%s: %d mismatches, smallest |w - 0.5| %.3f, first-order error at beta = 2 at most %.3f" %
          (name, wrong.sum(), np.abs(w[use] - 0.5).min(), err))
    for rule in ("parity", "winding"):
        print("%s: inside_ref.votes misclassifies %d of %d points under rule %s" %
              (name, ((ir.votes(osc, pts[use], rule) >= 2) != (dist[use] < 0)).sum(), use.sum(), rule))
    assert wrong.sum() == 0
    assert (wr.inside(osc, pts, 2.0)[use] == (dist[use] < 0)).all()


@pytest.mark.parametrize("name", ["cube", "torus", "degenerate"])
def test_moments_bottom_up_equal_a_direct_sum_per_node(name):
    osc = scene(name)
    mom, tri = wr.moments(osc), wr.stored(osc)
    for i in range(len(osc.nodes)):
        direct = wr.moment_direct(osc, i, tri)
        assert direct.view(np.uint32).tolist() == mom[i].view(np.uint32).tolist(), (name, i)
    assert (mom[:, 7] == 0).all() and (mom[:, 3] >= 0).all()
    # on a closed mesh the root's area vector vanishes up to rounding; r2 reaches the farthest corner of the root's box
    if name != "degenerate":
        assert np.abs(mom[-1, 0:3]).max() < 1e-5
    lo, hi, p = osc.nodes[-1]["bmin"], osc.nodes[-1]["bmax"], mom[-1, 4:7]
    corners = np.float64([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    assert np.isclose(mom[-1, 3], ((corners - p) ** 2).sum(axis=1).max(), rtol=1e-5)


@pytest.mark.filterwarnings("ignore::RuntimeWarning")               # (the helpers that make normals for the overflowing triangles)
def test_a_zero_area_node_falls_back_to_the_box_centre():
    # three triangles without area: a point, and two with collinear vertices
    pos = F([[[1, 1, 1]] * 3, [[0, 0, 0], [1, 0, 0], [3, 0, 0]], [[0, 2, 0], [0, 2, 2], [0, 2, 1]]])
    osc = ir.oracle_scene(pos, 4)
    mom = wr.moments(osc)
    root = osc.nodes[-1]
    assert (mom[-1, 0:3] == 0).all() and (mom[-1, 4:7] == F(0.5) * (root["bmin"] + root["bmax"])).all() and mom[-1, 3] > 0
    assert (wr.winding(osc, F([[0.5, 0.5, 0.5], [9, 9, 9]]), 2.0) == 0).all() and (wr.winding(osc, F([[0.5, 0.5, 0.5]]), np.inf) == 0).all()
    # and a node whose sums overflow: the area is not finite
    big = F([[[0, 0, 0], [3e19, 0, 0], [0, 3e19, 0]], [[1, 0, 0], [3e19, 0, 1], [0, 3e19, 1]]])
    osc = ir.oracle_scene(big, 4)
    mom = wr.moments(osc)
    root = osc.nodes[-1]
    assert (mom[-1, 4:7] == F(0.5) * (root["bmin"] + root["bmax"])).all()
