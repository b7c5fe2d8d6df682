"""tests/simplify_ref.py, the numpy restatement of include/drt.h "mesh simplification", checked on its own: hand cases for every
clause of the rule, the integer identities of a closed mesh on a sphere and a cube, quadric against mean placement by volume, the
cube's corners and edges coming back, and the singleton-grid identity."""
import numpy as np
import pytest

from tests import simplify_ref as sr

F = np.float32
NAN = float("nan")

SPHERE_GRIDS = (4, 6, 8, 12)
CUBE_GRIDS = (3, 4, 5)
_cache = {}


def solid(name):
    if name not in _cache:
        _cache[name] = sr.sphere() if name == "sphere" else sr.cube()
    return _cache[name]


def run(name, res, placement):
    """the restatement's result on the default grid of `res`^3 cells, computed once"""
    k = (name, res, placement)
    if k not in _cache:
        v, f = solid(name)
        _cache[k] = sr.simplify(v, f, *sr.default_grid(v, res), placement)
    return _cache[k]


def euler(s):
    edges = np.sort(np.stack([s.faces, np.roll(s.faces, -1, axis=1)], axis=-1).reshape(-1, 2), axis=1)
    return len(s.vertices) - len(np.unique(edges, axis=0)) + len(s.faces)


def test_two_vertices_in_one_cell_become_their_mean():
    v = F([[0.25, 0.5, 0.5], [0.75, 0.5, 0.25], [1.5, 0.5, 0.5]])
    f = np.int32([[0, 1, 2]])
    for placement in (sr.MEAN, sr.QUADRIC):
        s = sr.simplify(v, f, [0, 0, 0], [1, 1, 1], [2, 1, 1], placement)
        assert s.counts == (2, 0) and s.cluster.tolist() == [0, 0, 1] and s.first.tolist() == [0, 2]
        assert s.sums[0, 0] == 2 and s.sums[0, 1:4].tolist() == [0, 0, -(1 << 28)]      # r = (-.25, 0, 0) and (.25, 0, -.25), times 2^30
        assert s.vertices[1].tobytes() == v[2].tobytes()                      # one member: its 12 bytes
        if placement == sr.MEAN:
            assert s.vertices[0].tolist() == [0.5, 0.5, 0.375] and not s.sums[:, 4:].any()
        else:                                                                 # one plane through both members: its optimum is their mean
            assert s.sums[0, 4:].any() and not s.sums[1, 4:].any() and np.abs(s.vertices[0] - F([0.5, 0.5, 0.375])).max() < 1e-6


def test_a_vertex_on_lo_is_in_and_one_on_the_far_face_is_out():
    lo, cell, dims = F([-1, -1, -1]), F([0.5, 0.5, 0.5]), [4, 4, 4]
    v = F([[-1, -1, -1], [-0.9, -0.9, -0.9], [1, 0, 0], [0.9, 0.1, 0.1], [-1.0000001, 0, 0], [0, 0, np.nextafter(F(1), F(0))]])
    key, idx = sr.keys_of(v, lo, cell, dims)
    # the last one lies below the far face, but p - lo = 2 - 2^-24 rounds to 2 and f = 4 is not below dims: out, by the f rule
    assert key.tolist() == [0, 0, sr.OUTSIDE, 3 + 4 * (2 + 4 * 2), sr.OUTSIDE, sr.OUTSIDE]
    assert sr.keys_of(F([[0, 0, 0.99]]), lo, cell, dims)[0].tolist() == [2 + 4 * (2 + 4 * 3)]
    s = sr.simplify(v, np.zeros((0, 3), np.int32), lo, cell, dims)
    assert s.counts == (5, 0) and s.cluster.tolist() == [0, 0, 1, 2, 3, 4] and s.first.tolist() == [0, 2, 3, 4, 5]
    assert s.vertices[1:].tobytes() == v[2:].tobytes()                        # nothing is clamped, nothing outside is moved


def test_vertices_that_are_not_finite_are_singletons_with_their_bytes():
    v = F([[0.1, 0.1, 0.1], [NAN, 0.1, 0.1], [0.2, 0.2, 0.2], [np.inf, 0, 0], [NAN, 0.1, 0.1], [0.1, -np.inf, 0.1]])
    v.view(np.uint32)[4, 0] = 0x7FC00123                                      # another NaN's bits
    s = sr.simplify(v, np.int32([[0, 1, 3], [0, 2, 4]]), [0, 0, 0], [1, 1, 1], [1, 1, 1])
    assert s.cluster.tolist() == [0, 1, 0, 2, 3, 4] and s.first.tolist() == [0, 1, 3, 4, 5]
    assert s.vertices[1:].tobytes() == v[[1, 3, 4, 5]].tobytes()
    assert s.faces.tolist() == [[0, 1, 2]] and s.source.tolist() == [0]        # the second names cluster 0 twice
    assert np.isfinite(s.vertices[0]).all()                                    # the triangles with a NaN corner add nothing


def test_triangles_are_dropped_kept_in_order_and_truncated():
    v = F([[0.1, 0.1, 0.1], [0.2, 0.1, 0.1], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5], [0.5, 1.5, 0.5], [2.5, 0.6, 0.5]])
    f = np.int32([[0, 2, 3], [0, 1, 2], [2, 3, 4], [2, 6, 4], [-1, 2, 3], [4, 3, 2], [2, 2, 4], [2, 3, 5], [1, 4, 3], [2, 3, 4]])
    grid = ([0, 0, 0], [1, 1, 1], [3, 2, 1])
    s = sr.simplify(v, f, *grid)
    assert s.cluster.tolist() == [0, 0, 1, 2, 3, 2] and s.counts == (4, 5)
    assert s.source.tolist() == [0, 2, 5, 8, 9]                                # two corners in one cluster, an index out of range: dropped
    assert s.faces.tolist() == [[0, 1, 2], [1, 2, 3], [3, 2, 1], [0, 3, 2], [1, 2, 3]]      # a duplicate stays
    for vc, tc in ((0, 0), (1, 2), (3, 5), (4, 4), (9, 9)):
        c = sr.simplify(v, f, *grid, vertex_capacity=vc, tri_capacity=tc)
        assert c.counts == (4, 5) and c.cluster.tolist() == s.cluster.tolist()
        assert c.vertices.tobytes() == s.vertices[:vc].tobytes() and c.first.tolist() == s.first[:vc].tolist()
        assert c.faces.tolist() == s.faces[:tc].tolist() and c.source.tolist() == s.source[:tc].tolist()


def test_no_vertices_and_no_triangles():
    s = sr.simplify(np.zeros((0, 3), F), np.zeros((0, 3), np.int32), [0, 0, 0], [1, 1, 1], [1, 1, 1])
    assert s.counts == (0, 0) and s.vertices.shape == (0, 3) and s.faces.shape == (0, 3)
    s = sr.simplify(np.zeros((0, 3), F), np.int32([[0, 1, 2]]), [0, 0, 0], [1, 1, 1], [1, 1, 1])
    assert s.counts == (0, 0)


def test_the_solids_are_what_the_tests_take_them_for():
    v, f = solid("sphere")
    assert len(f) == 3968 and sr.directed_edge_balance(f) and abs(sr.volume(v, f) - 2.136) < 1e-3
    v, f = solid("cube")
    assert len(f) == 3072 and sr.directed_edge_balance(f) and abs(sr.volume(v, f) - 1.0) < 1e-6


@pytest.mark.parametrize("placement", [sr.MEAN, sr.QUADRIC])
@pytest.mark.parametrize("name,grids", [("sphere", SPHERE_GRIDS), ("cube", CUBE_GRIDS)])
def test_directed_edges_balance_and_the_outputs_are_spheres(name, grids, placement):
    v, f = solid(name)
    for res in grids:
        s = run(name, res, placement)
        assert s.counts[0] < len(v) and 0 < s.counts[1] < len(f)
        assert sr.directed_edge_balance(s.faces), res                          # by integers: a closed input gives a closed output
        assert (s.cluster[f[s.source]] == s.faces).all()
        # these outputs are manifolds (every edge used once in each direction), so Euler's formula holds
        edges, uses = np.unique(np.sort(np.stack([s.faces, np.roll(s.faces, -1, axis=1)], axis=-1).reshape(-1, 2), axis=1), axis=0, return_counts=True)
        assert (uses == 2).all() and euler(s) == 2, res


@pytest.mark.parametrize("name,grids", [("sphere", SPHERE_GRIDS), ("cube", CUBE_GRIDS)])
def test_quadric_placement_keeps_more_of_the_volume_than_the_mean(name, grids):
    v, f = solid(name)
    want = sr.volume(v, f)
    for res in grids:
        mean, quadric = (sr.volume(run(name, res, p).vertices, run(name, res, p).faces) for p in (sr.MEAN, sr.QUADRIC))
        print("%s %d^3: input %.4f mean %.4f quadric %.4f" % (name, res, want, mean, quadric))
        assert abs(quadric - want) < abs(mean - want), (res, mean, quadric)


def cube_distance(p):
    """the distance of points to the surface of [0, 1]^3, float64"""
    p = np.asarray(p, np.float64)
    inside = np.minimum(p, 1 - p).min(axis=1)
    outside = np.linalg.norm(np.maximum(np.maximum(-p, p - 1), 0), axis=1)
    return np.where(inside >= 0, inside, outside)


# the restatement measures 3.31e-4 (3^3), 2.69e-4 (4^3) and 2.07e-4 (5^3): the pull of lam = tr 2^-10 towards the mean, which lies
# inside the cube at corners and edges.  Only rounding differs between the restatement and the device, so four times the largest.
CUBE_SURFACE_BOUND = 4 * 3.31e-4


def test_quadric_placement_puts_the_cubes_vertices_on_its_surface():
    for res in CUBE_GRIDS:
        quadric, mean = cube_distance(run("cube", res, sr.QUADRIC).vertices).max(), cube_distance(run("cube", res, sr.MEAN).vertices).max()
        print("cube %d^3: largest distance to the surface, quadric %.3g, mean %.3g" % (res, quadric, mean))
        assert quadric < CUBE_SURFACE_BOUND and mean > 0.05                    # the mean chamfers corners and edges
    # the eight corners come back: the 3^3 grid has one cluster at each
    s = run("cube", 3, sr.QUADRIC)
    corners = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float64)
    nearest = np.linalg.norm(s.vertices.astype(np.float64)[None] - corners[:, None], axis=2).min(axis=1)
    assert nearest.max() < CUBE_SURFACE_BOUND * np.sqrt(3)


@pytest.mark.parametrize("placement", [sr.MEAN, sr.QUADRIC])
def test_a_grid_of_singletons_returns_the_input_byte_for_byte(placement):
    v, f = solid("sphere")
    f = np.concatenate([f, np.int32([[0, 0, 1], [5, len(v), 6]])])             # ... and the surviving faces
    lo, cell, dims = sr.default_grid(v, 1024)
    s = sr.simplify(v, f, lo, cell, dims, placement)
    assert s.counts == (len(v), len(f) - 2)
    assert s.vertices.tobytes() == v.tobytes() and s.faces.tobytes() == f[:-2].tobytes()
    assert s.first.tolist() == list(range(len(v))) == s.cluster.tolist() and s.source.tolist() == list(range(len(f) - 2))


def test_the_default_grid_holds_every_finite_vertex():
    rng = np.random.default_rng(5)
    for scale, shift in ((1.0, 0.0), (2.0 ** -100, 0.0), (2.0 ** 100, 0.0), (1e-3, 1000.0), (1.0, -7.5)):
        v = (rng.standard_normal((500, 3)) * scale + shift).astype(F)
        v[7] = NAN
        v[:, 2] = v[0, 2]                                                       # a flat axis
        for res, cell in ((1, None), (7, None), ((3, 1000, 2), None), (None, float(np.ptp(v[np.isfinite(v).all(axis=1)], axis=0).max()) / 9)):
            lo, c, dims = sr.default_grid(v, res, cell)
            key, _ = sr.keys_of(v, lo, c, dims)
            assert (key != sr.OUTSIDE).sum() == 499 and key[7] == sr.OUTSIDE, (scale, shift, res)
