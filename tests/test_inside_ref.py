"""The crossing-count rule of include/drt.h as tests/inside_ref.py restates it (CPU only): hand-derived counts on a cube, the
analytic inside of a torus and a sphere, a lattice whose rays run along the cube's edges and through its vertices, the traversal
against a brute force over all triangles, and the wedge on which the nearest triangle's plane gives the wrong sign."""
import numpy as np
import pytest

import oracle
from tests import inside_ref as ir
from tests import nearest_ref as nr
from tests import ray_query_ref as rq
from tests.scenes import scene_path

RULE_NAMES = ["parity", "winding"]


def test_the_meshes_are_closed_and_outward():
    for name, pos, n in (("cube", ir.cube(), 12), ("torus", ir.torus(), 1024), ("sphere", ir.sphere(), 512), ("wedge", ir.wedge(), 8)):
        assert len(pos) == n and ir.mesh_is_closed_and_outward(pos), name
    assert np.allclose(np.linalg.norm(ir.sphere().reshape(-1, 3), axis=1), 1, atol=1e-6)


def test_hand_derived_counts_on_the_cube():
    osc = ir.oracle_scene(ir.cube(), 2)
    assert oracle.tree_depth(osc.nodes) >= 3
    # the centre: every ray leaves through exactly one face, an exit (+1)
    for d in ir.DIRS:
        c = ir.crossings(osc, np.zeros((1, 3), np.float32), d[None])
        assert (c.count.tolist(), c.winding.tolist()) == ([1], [1])
        assert c.count.dtype == np.uint32 and c.winding.dtype == np.int32
    assert ir.votes(osc, np.zeros((1, 3), np.float32)).tolist() == [3] and ir.votes(osc, np.zeros((1, 3), np.float32), "winding").tolist() == [3]
    # outside: a ray passes through (one entry, one exit) or by
    out = np.float32([[-3, -2.5, -3.5], [3, 0.25, 0.5], [0.25, 5, 0.125], [-2, -1.25, -2]])
    seen = set()
    for d in ir.DIRS:
        c = ir.crossings(osc, out, np.tile(d, (len(out), 1)))
        assert np.isin(c.count, (0, 2)).all() and (c.winding == 0).all()
        seen |= set(c.count.tolist())
    assert seen == {0, 2}
    for rule in RULE_NAMES:
        assert ir.votes(osc, out, rule).tolist() == [0] * len(out)
    # an interval that ends inside the cube keeps the entry only; one that starts inside keeps the exit only
    org, d = np.float32([[-3, 0.25, 0.5]]), np.float32([[1, 0, 0]])          # enters at t = 2, leaves at t = 4 (the boxes see no 0 * inf:
    c = ir.crossings(osc, org, d, 0.0, 3.0)                                     #  the origin is on no box plane)
    assert (c.count.tolist(), c.winding.tolist()) == ([1], [-1])
    c = ir.crossings(osc, org, d, 3.0, np.inf)
    assert (c.count.tolist(), c.winding.tolist()) == ([1], [1])
    c = ir.crossings(osc, org, d, 2.0, 4.0)                                     # strict at both ends
    assert (c.count.tolist(), c.winding.tolist()) == ([0], [0])
    # NaN rays and an empty scene
    bad = np.float32([[np.nan, 0, 0]])
    c = ir.crossings(osc, bad, ir.DIRS[:1])
    assert (c.count.tolist(), c.winding.tolist()) == ([0], [0])
    c = ir.crossings(osc, np.zeros((1, 3), np.float32), ir.DIRS[:1], 0.0, np.nan)
    assert (c.count.tolist(), c.winding.tolist()) == ([0], [0])
    empty = oracle.Scene(np.zeros(0, oracle.TRI_DTYPE), [((0.8, 0.8, 0.8), -1)], [])
    c = ir.crossings(empty, out, np.tile(ir.DIRS[0], (len(out), 1)))
    assert not c.count.any() and not c.winding.any() and not ir.votes(empty, out).any()


@pytest.mark.parametrize("shape", ["torus", "sphere"])
def test_analytic_shapes_are_classified_without_a_mismatch(shape):
    """4 000 seeded points; every one farther than 0.03 from the analytic surface (the faceting error of these meshes is below 0.02)
    is classified as the analytic shape says, under both rules."""
    pos, dist = (ir.torus(), ir.torus_distance) if shape == "torus" else (ir.sphere(), ir.sphere_distance)
    osc = ir.oracle_scene(pos, 4)
    pts = np.random.default_rng(5).uniform(-1.5, 1.5, (4000, 3)).astype(np.float32)
    d = dist(pts)
    clear = np.abs(d) > 0.03
    assert clear.sum() > 3000 and (d[clear] < 0).sum() > 100
    for rule in RULE_NAMES:
        v = ir.votes(osc, pts, rule)
        wrong = ((v >= 2) != (d < 0)) & clear
        split = ((v == 1) | (v == 2)) & clear
        print("%s, %s: %d of %d clear points misclassified, %d votes not unanimous" % (shape, rule, wrong.sum(), clear.sum(), split.sum()))
        assert wrong.sum() == 0


def test_the_cube_lattice():
    """13^3 points over [-1.5, 1.5]^3 around the cube [-1, 1]^3, the ones on its surface left out: rays from lattice points run along
    edges and through vertices as often as any input will."""
    osc = ir.oracle_scene(ir.cube(), 2)
    axis = (np.arange(13, dtype=np.float32) * np.float32(0.25) - np.float32(1.5)).astype(np.float32)
    pts = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), axis=-1).reshape(-1, 3)
    big = np.abs(pts).max(axis=1)
    pts, big = pts[big != 1], big[big != 1]
    assert len(pts) == 13 ** 3 - (9 ** 3 - 7 ** 3)
    for rule in RULE_NAMES:
        v = ir.votes(osc, pts, rule)
        wrong = (v >= 2) != (big < 1)
        print("lattice, %s: %d of %d misclassified, %d votes not unanimous" % (rule, wrong.sum(), len(pts), ((v == 1) | (v == 2)).sum()))
        assert wrong.sum() == 0


@pytest.fixture(scope="module", params=["cornell_box", "soup"])
def scene(request):
    if request.param == "soup":
        return request.param, nr.oracle_soup(3000, 5, 2, 8)
    return request.param, oracle.Scene.load_glb(scene_path("cornell_box")).build_bvh(20, 8)


def test_traversal_counts_equal_a_brute_force_over_all_triangles(scene):
    """Every ray of rq.surface_rays and rq.interval_rays; the share of rays a slab test at a box boundary may send past a triangle is
    the one tests/test_ray_query_ref.py allows its closest-hit check: max(2, n // 200)."""
    name, osc = scene
    rng = np.random.default_rng(11)
    n = 1200
    org, dirs = rq.surface_rays(osc, n, rng)
    sets = [("surface rays", org, dirs, np.float32(0), ir.INF)]
    org, dirs, tmin, tmax = rq.interval_rays(osc, n, rng)
    sets.append(("random intervals", org, dirs, tmin, tmax))
    for what, org, dirs, tmin, tmax in sets:
        got, bf = ir.crossings(osc, org, dirs, tmin, tmax), ir.brute_force(osc, org, dirs, tmin, tmax)
        differ = (got.count != bf.count) | (got.winding != bf.winding)
        print("%s, %s: %d of %d rays differ from the brute force, %d crossings in all" % (name, what, differ.sum(), n, bf.count.sum()))
        assert bf.count.sum() > 50
        assert (got.count[differ] < bf.count[differ]).all()                     # the boxes can only drop a triangle
        assert differ.sum() <= max(2, n // 200), what
    # the vote over the tree and over all triangles: the same share of the points
    pts = nr.box_points(nr.from_oracle(osc), 300, rng, 1.2)
    for rule in RULE_NAMES:
        assert (ir.votes(osc, pts, rule) != ir.votes(osc, pts, rule, ir.brute_force)).sum() <= max(2, len(pts) // 200)


def test_the_wedge_where_the_nearest_plane_gives_the_wrong_sign():
    """Two mirror-image points outside the wedge, just beyond its edge.  The edge's two triangles tie exactly (the coordinates are
    dyadic), the first one tested wins, and its plane puts exactly one of the two points behind it.  The vote does not care."""
    pos = ir.wedge()
    osc = ir.oracle_scene(pos, 4)
    g = nr.from_oracle(osc)
    # the derivation: both edge triangles are at d2 = (1/16)^2 + (1/64)^2 from both points, at c = (0, 0, 1/2)
    edge_tris = [k for k in range(len(g.v0)) if np.array_equal(g.v0[k], [0, 0, 0]) and (np.array_equal(g.v0[k] + g.e1[k], [0, 0, 1]) or np.array_equal(g.v0[k] + g.e2[k], [0, 0, 1]))]
    assert len(edge_tris) == 2
    want = np.float32(1 / 256 + 1 / 4096)
    for k in edge_tris:
        d2, _, _, c = nr.closest_on_triangle(ir.WEDGE_POINTS, g.v0[k][None], g.e1[k][None], g.e2[k][None])
        assert d2.tolist() == [want, want] and c.tolist() == [[0, 0, 0.5]] * 2
        side = np.where(nr.dot(ir.WEDGE_POINTS - c, g.fn[k][None]) < 0, -1, 1)
        assert sorted(side.tolist()) == [-1, 1]                                # each plane has one of the two points behind it
    near = nr.nearest(g, ir.WEDGE_POINTS)
    assert near.d2.tolist() == [want, want] and near.prim[0] == near.prim[1] and near.prim[0] in edge_tris
    assert sorted(near.side.tolist()) == [-1.0, 1.0]                            # nearest: one of the two outside points is "behind"
    for rule in RULE_NAMES:
        assert ir.votes(osc, ir.WEDGE_POINTS, rule).tolist() == [0, 0]
        sd = ir.signed_distance(osc, ir.WEDGE_POINTS, rule=rule)
        assert sd.side.tolist() == [1.0, 1.0]                                   # the signed distance is positive for both
        for f in ("point", "d2", "prim", "u", "v"):
            assert getattr(sd, f).tobytes() == getattr(near, f).tobytes()
    inner = np.float32([[0.5, 0, 0.5], [0.75, 0.0625, 0.25]])
    assert ir.signed_distance(osc, inner).side.tolist() == [-1.0, -1.0]
    assert ir.signed_distance(osc, inner, max_dist=0.0).side.tolist() == [-1.0, -1.0]      # a miss record carries the sign too
    assert (ir.signed_distance(osc, inner, max_dist=0.0).prim == -1).all()
