"""The isosurface rule of include/drt.h, pinned on the float32 restatement (tests/isosurface_ref.py) without a GPU and independently of
the kernel: hand cases on one cube with coordinates derived on paper, topology by integers (unique bit patterns and
drt.triEdgeAdjacency, which runs on the host), orientation, volume against the analytic value, a random field with and without a
border, NaN, a sample equal to the level, the CSR helper, and the reference-only form of the end-to-end case."""
import numpy as np
import pytest

from tests import inside_ref as ir
from tests import isosurface_ref as iso
from tests import ray_query_ref as rq
from tests import winding_ref as wr

drt = pytest.importorskip("dustraytracer_amd")

SPHERE = ((-1.03, -1.1, -1.07), (1.05, 1.02, 1.09), 0.8)
TORUS = ((-1.13, -1.1, -0.57), (1.15, 1.12, 0.59), 0.7, 0.25)
SPHERE_VOLUME = 4.0 / 3.0 * np.pi * 0.8 ** 3
TORUS_VOLUME = 2.0 * np.pi ** 2 * 0.7 * 0.25 ** 2
_cache = {}


def shape(name, n):
    """(field, lo, cell, counts, records) of the sphere or the torus at n^3, made once."""
    if (name, n) not in _cache:
        if name == "sphere":
            f, cell = iso.sphere_sdf(n, *SPHERE)
            lo = SPHERE[0]
        else:
            f, cell = iso.torus_sdf(n, *TORUS)
            lo = TORUS[0]
        _cache[name, n] = (f, lo, cell) + iso.isosurface(f, 0.0, lo, cell)
    return _cache[name, n]


def tri(*pts):
    return np.float32(pts).reshape(3, 3)


def assert_records(recs, expected):
    """expected: (tetrahedron, case, [[x, y, z] x 3]) per record, in order."""
    assert len(recs) == len(expected), (len(recs), len(expected))
    for r, (t, case, v) in zip(recs, expected):
        assert r["cube"] == 0 and r["code"] == (t | case << 4) and r["zero"] == 0, (r, t, case)
        assert r["v"].tobytes() == tri(*v).tobytes(), (t, case, r["v"], v)


UNIT = dict(lo=(0, 0, 0), cell=(1, 1, 1))                  # the eight samples lie at 0.5 and 1.5 per axis


def corner_field(values):
    """[2, 2, 2] field from eight values by corner number c = dx + 2 dy + 4 dz."""
    return np.float32(values).reshape(2, 2, 2)


def test_one_corner_above_six_triangles_around_it():
    # corner 0 = +3, the rest -1, level 0: every edge from corner 0 is cut at t = (0 - 3) / (-1 - 3) = 0.75, 0.5 + 0.75 = 1.25.  Corner 0
    # is local vertex 0 of all six tetrahedra (0, B, C, 7): case 1, triangle (e01, e03, e02) = the cuts towards (B, 7, C), and towards
    # (B, C, 7) in the mirror images 1, 2, 5
    counts, recs = iso.isosurface(corner_field([3, -1, -1, -1, -1, -1, -1, -1]), 0.0, **UNIT)
    a, b = 0.5, 1.25
    p = {1: (b, a, a), 2: (a, b, a), 3: (b, b, a), 4: (a, a, b), 5: (b, a, b), 6: (a, b, b), 7: (b, b, b)}
    assert_records(recs, [(0, 1, [p[1], p[7], p[3]]), (1, 1, [p[1], p[5], p[7]]), (2, 1, [p[2], p[3], p[7]]),
                          (3, 1, [p[2], p[7], p[6]]), (4, 1, [p[4], p[7], p[5]]), (5, 1, [p[4], p[6], p[7]])])
    assert counts.tolist() == [6]
    # the normals point to the above side: towards corner 0
    v = recs["v"].astype(np.float64)
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    assert ((n * (np.float64([0.5, 0.5, 0.5]) - v[:, 0])).sum(axis=1) > 0).all()


def test_one_corner_below_six_triangles_around_it():
    # corner 7 = -1, the rest +3: corner 7 is local vertex 3 everywhere: case 7, triangle (e03, e23, e13) = the cuts from (0, C, B)
    # towards 7, always interpolated FROM the smaller corner: a + (1.5 - a) * 0.75 = 1.25 where the axis moves, else 1.5
    counts, recs = iso.isosurface(corner_field([3, 3, 3, 3, 3, 3, 3, -1]), 0.0, **UNIT)
    m, h = 1.25, 1.5
    q = {0: (m, m, m), 1: (h, m, m), 2: (m, h, m), 3: (h, h, m), 4: (m, m, h), 5: (h, m, h), 6: (m, h, h)}
    assert_records(recs, [(0, 7, [q[0], q[3], q[1]]), (1, 7, [q[0], q[1], q[5]]), (2, 7, [q[0], q[2], q[3]]),
                          (3, 7, [q[0], q[6], q[2]]), (4, 7, [q[0], q[5], q[4]]), (5, 7, [q[0], q[4], q[6]])])
    assert counts.tolist() == [6]


PLANE = [(0, 1, [(1, .5, .5), (1, 1, 1), (1, 1, .5)]),
         (1, 1, [(1, .5, .5), (1, .5, 1), (1, 1, 1)]),
         (2, 3, [(1, 1, .5), (1, 1.5, 1), (1, 1.5, .5)]), (2, 3, [(1, 1, .5), (1, 1, 1), (1, 1.5, 1)]),
         (3, 7, [(1, 1, 1), (1, 1.5, 1.5), (1, 1.5, 1)]),
         (4, 3, [(1, .5, 1), (1, .5, 1.5), (1, 1, 1.5)]), (4, 3, [(1, .5, 1), (1, 1, 1.5), (1, 1, 1)]),
         (5, 7, [(1, 1, 1), (1, 1, 1.5), (1, 1.5, 1.5)])]


def test_a_two_two_split_is_a_quad_split_along_a_fixed_diagonal():
    # f = +1 at x = 0.5 and -1 at x = 1.5: the plane x = 1, every cut at a midpoint.  Tetrahedra 0 and 1 have corner 0 alone above (case 1),
    # 3 and 5 have corner 7 alone below (case 7), 2 = (0,2,3,7) and 4 = (0,4,5,7) have their local vertices 0 and 1 above: case 3, the quad
    # (e02, e12, e13, e03) as (e02, e12, e13) and (e02, e13, e03), the second and third vertex exchanged in the mirror image 2
    counts, recs = iso.isosurface(corner_field([1, -1, 1, -1, 1, -1, 1, -1]), 0.0, **UNIT)
    assert_records(recs, PLANE)
    assert counts.tolist() == [8]
    v = recs["v"].astype(np.float64)
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    assert (n[:, 0] < 0).all() and (n[:, 1:] == 0).all()          # towards the above side, x = 0.5
    assert 0.5 * np.abs(n[:, 0]).sum() == 1.0                     # the unit square between the samples, tiled once


def test_flip_exchanges_the_second_and_third_vertex_of_every_triangle():
    _, recs = iso.isosurface(corner_field([1, -1, 1, -1, 1, -1, 1, -1]), 0.0, flip=True, **UNIT)
    assert_records(recs, [(t, c, [v[0], v[2], v[1]]) for t, c, v in PLANE])


@pytest.mark.parametrize("name,sizes,chi,tris16", [("sphere", (8, 16, 24, 32), 2, 4124), ("torus", (16, 24, 32), 0, 4624)])
def test_topology_by_integers(name, sizes, chi, tris16):
    for n in sizes:
        _, _, _, counts, recs = shape(name, n)
        t = iso.triangles(recs)
        adj = drt.triEdgeAdjacency(t)
        assert (adj >= 0).all(), (name, n, (adj == -1).sum(), (adj == -2).sum())       # every half-edge has exactly one twin
        flat = adj.reshape(-1)
        assert (flat[flat] == np.arange(len(flat))).all()
        e = t[:, [1, 2, 0]] - t
        assert (np.abs(e).max(axis=2) > 0).all()                                        # no zero-length edge
        area2 = np.cross(t[:, 1].astype(np.float64) - t[:, 0], t[:, 2].astype(np.float64) - t[:, 0])
        assert ((area2 * area2).sum(axis=1) > 0).all()                                  # no zero-area triangle
        V, E, F = iso.euler(t)
        assert V - E + F == chi, (name, n, V, E, F)
        assert counts.sum() == len(recs) and len(counts) == (n - 1) ** 2
        if n == 16:
            assert len(recs) == tris16


def test_orientation_by_the_signed_volume():
    f, lo, cell, _, recs = shape("sphere", 16)
    vol = iso.signed_volume(iso.triangles(recs))
    assert vol > 0                                                                      # an SDF, default orientation: outward faces
    _, flipped = iso.isosurface(f, 0.0, lo, cell, flip=True)
    assert iso.signed_volume(iso.triangles(flipped)) == pytest.approx(-vol, rel=1e-12)
    _, neg = iso.isosurface(-f, 0.0, lo, cell, flip=True)                               # large inside, as winding numbers are
    assert iso.signed_volume(iso.triangles(neg)) > 0


# relative volume error in percent as the restatement gives it (measured), and the bound: 1.5 times that.  The surface of the linear
# interpolant is inscribed, so the error is negative, and it falls with h^2.
VOLUME = {("sphere", 16): (-1.3703, 2.0555), ("sphere", 24): (-0.6101, 0.9152), ("sphere", 32): (-0.3433, 0.5150),
          ("torus", 16): (-3.4072, 5.1108), ("torus", 24): (-1.5008, 2.2512), ("torus", 32): (-0.8376, 1.2564)}


@pytest.mark.parametrize("name,exact", [("sphere", SPHERE_VOLUME), ("torus", TORUS_VOLUME)])
def test_volume_against_the_analytic_value(name, exact):
    err = {}
    for n in (16, 24, 32):
        vol = iso.signed_volume(iso.triangles(shape(name, n)[4]))
        err[n] = 100.0 * (vol - exact) / exact
        measured, bound = VOLUME[name, n]
        print("%s %d^3: volume error %.4f %% (measured %.4f %%, bound -%.4f %%)" % (name, n, err[n], measured, bound))
        assert -bound <= err[n] < 0, (name, n, err[n])
        assert bound == pytest.approx(1.5 * -measured, abs=1e-4)
    assert abs(err[32]) < abs(err[24]) < abs(err[16])


def test_a_random_field_is_open_without_a_border_and_closed_with_one():
    f = np.random.default_rng(1).standard_normal((5, 7, 9)).astype(np.float32)
    counts, recs = iso.isosurface(f, 0.1, (0, 0, 0), (1, 1, 1))
    adj = drt.triEdgeAdjacency(iso.triangles(recs))
    assert len(counts) == 6 * 4 and (adj == -1).sum() > 0 and (adj == -2).sum() == 0    # 314 boundary half-edges for this seed
    counts, recs = iso.isosurface(f, 0.1, (0, 0, 0), (1, 1, 1), border=-1.0)
    adj = drt.triEdgeAdjacency(iso.triangles(recs))
    assert len(counts) == 8 * 6 and recs["cube"].max() < 10 * 8 * 6
    assert (adj >= 0).all()                                                             # closed, no duplicate half-edges
    assert iso.signed_volume(iso.triangles(recs)) < 0                                   # (above is inside here: the faces look inwards)


def test_a_nan_silences_exactly_the_tetrahedra_that_touch_it():
    f, lo, cell, _, recs = shape("sphere", 8)
    for bad in (np.nan, np.inf, -np.inf):
        g = f.copy()
        z, y, x = 2, 3, 1                                                               # a sample next to the surface
        g[z, y, x] = bad
        _, got = iso.isosurface(g, 0.0, lo, cell)
        nx = ny = 7
        touched = set()
        for c in range(8):                                                              # the cubes that have the sample as corner c
            cx, cy, cz = x - (c & 1), y - ((c >> 1) & 1), z - (c >> 2)
            if 0 <= cx < nx and 0 <= cy < ny and 0 <= cz < 7:
                touched |= {(cx + nx * (cy + ny * cz), t) for t, tet in enumerate(iso.TETS) if c in tet}
        keep = np.array([(int(r["cube"]), int(r["code"]) & 15) not in touched for r in recs])
        assert 0 < keep.sum() < len(recs)
        assert got.tobytes() == recs[keep].tobytes()


def test_a_sample_equal_to_the_level_is_above_and_gives_zero_area_triangles():
    f, lo, cell, _, _ = shape("sphere", 8)
    f = f.copy()
    # a sample outside the sphere (above) whose +x, +y and +z neighbours are inside: the smaller end of three cut edges
    above = (f[:-1, :-1, :-1] > 0) & (f[:-1, :-1, 1:] < 0) & (f[:-1, 1:, :-1] < 0) & (f[1:, :-1, :-1] < 0)
    z, y, x = np.argwhere(above)[0]
    f[z, y, x] = 0.0
    counts, recs = iso.isosurface(f, 0.0, lo, cell)
    t = iso.triangles(recs)
    own = np.float32([iso.positions(np.float32(lo[k]), cell[k], 8, 0)[i] for k, i in enumerate((x, y, z))])
    at_corner = (t.view(np.uint32) == own.view(np.uint32)).all(axis=2)                  # t = 0: the corner's own position, bit for bit
    assert at_corner.sum() >= 3
    zero_area = at_corner.sum(axis=1) >= 2
    assert zero_area.sum() > 0
    adj = drt.triEdgeAdjacency(t)
    assert (adj[zero_area] == -2).any() and (adj == -1).sum() == 0
    assert counts.sum() == len(recs)


def test_capacity_clamping_and_miss_records_of_the_csr_helper():
    f = np.random.default_rng(3).standard_normal((3, 4, 5)).astype(np.float32)
    counts, recs = iso.isosurface(f, 0.0, (0, 0, 0), (1, 1, 1))
    rows, total = len(counts), len(recs)
    assert rows == 3 * 2 and total == counts.sum() and counts.min() > 0
    exact = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    assert iso.fill(counts, recs, exact, total).tobytes() == recs.tobytes()
    # every row two slots: truncated lists and padded ones
    two = (np.arange(rows + 1) * 2).astype(np.uint32)
    out = iso.fill(counts, recs, two, 2 * rows)
    for r in range(rows):
        n = min(2, int(counts[r]))
        assert out[2 * r:2 * r + n].tobytes() == recs[exact[r]:exact[r] + n].tobytes()
        assert (out[2 * r + n:2 * r + 2]["cube"] == iso.MISS_CUBE).all()
    # a capacity below the offsets clamps; a decreasing pair owns nothing; slots nobody owns keep their content
    big = (np.arange(rows + 1) * 40).astype(np.uint32)
    sentinel = np.zeros(100, iso.RECORD)
    sentinel["cube"] = 7
    out = iso.fill(counts, recs, big, 100, out=sentinel)
    assert out[0:counts[0]].tobytes() == recs[0:counts[0]].tobytes() and (out[counts[0]:40]["cube"] == iso.MISS_CUBE).all()
    assert (out[80 + min(20, int(counts[2])):100]["cube"] == iso.MISS_CUBE).all()        # row 2 is clamped to 20 slots, rows 3.. own none
    miss = out[39]
    assert miss["cube"] == iso.MISS_CUBE and not miss["v"].any() and miss["code"] == 0 and miss["zero"] == 0
    down = np.uint32([5, 0, 0, 0, 0, 0, 0])
    assert iso.fill(counts, recs, down, 100, out=sentinel).tobytes() == sentinel.tobytes()


# ---- the end-to-end case on the references alone: what tests/test_gpu_isosurface.py asserts on the device must hold here first ----
def open_torus(seed=17):
    pos = ir.torus()
    keep = np.ones(len(pos), bool)
    keep[np.random.default_rng(seed).choice(len(pos), len(pos) // 10, replace=False)] = False
    return pos[keep]


def remesh_grid(lo, hi, resolution, margin):
    """Renderer.remesh's padded grid: (lo, hi, res)."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    cell = ((hi - lo) / np.float32(resolution)).astype(np.float32)
    return (lo - np.float32(margin) * cell).astype(np.float32), (hi + np.float32(margin) * cell).astype(np.float32), resolution + 2 * margin


def end_to_end_points(cell, n=600, seed=5):
    """Points of the padded box at least two cells (and the facets' sag) from the torus's surface."""
    p = np.random.default_rng(seed).uniform((-1.6, -1.6, -0.5), (1.6, 1.6, 0.5), (n, 3)).astype(np.float32)
    far = np.abs(ir.torus_distance(p)) >= 2.0 * float(np.max(cell)) + 0.01
    return p[far]


def test_the_end_to_end_case_holds_on_the_references_alone():
    sc, osc = rq.programmatic_scene(drt, *ir.streams(open_torus()), 4, 8)
    root = osc.nodes[-1]
    lo, hi, res = remesh_grid(root["bmin"], root["bmax"], 24, 1)
    cell = iso.cell_of(lo, hi, (res,) * 3)
    assert np.allclose(cell, iso.cell_of(root["bmin"], root["bmax"], (24,) * 3), rtol=1e-6)      # the padding keeps the cell size
    ax = [iso.positions(lo[k], cell[k], res, 0) for k in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    w = wr.winding(osc, np.stack([x, y, z], axis=-1).reshape(-1, 3), 2.0).reshape(res, res, res)
    counts, recs = iso.isosurface(w, 0.5, lo, cell, flip=True, border=0.0)
    t = iso.triangles(recs)
    adj = drt.triEdgeAdjacency(t)
    assert (adj >= 0).all()
    V, E, F = iso.euler(t)
    assert V - E + F == 0 and iso.signed_volume(t) > 0
    pts = end_to_end_points(iso.cell_of(root["bmin"], root["bmax"], (24,) * 3))
    print("end to end: %d triangles, %d test points" % (len(t), len(pts)))
    assert len(pts) == 218                                          # the point count: fixed by the seed, the box and the margin
    remeshed = ir.oracle_scene(t, 4)
    inside_new = ir.inside(remeshed, pts, "parity")
    inside_old = wr.inside(osc, pts, 2.0, 0.5)
    print("inside: %d of %d" % (inside_old.sum(), len(pts)))
    assert inside_old.any() and (~inside_old).any()
    assert (inside_new == inside_old).all()
