"""The plane-section rule of include/drt.h as tests/section_ref.py restates it (CPU only): hand-derived cuts of a tetrahedron in which
every operation is exact, the traversal against the brute force, the monotonicity that the node cull rests on, the orientation of
every segment, a tree with exchanged children, and invalid planes."""
import numpy as np
import pytest

import oracle
from tests import nearest_ref as nr
from tests import section_ref as sr
from tests.scenes import scene_path
from tests.tri_overlap_scenes import TETRAHEDRON

NAN, INF = np.float32(np.nan), np.float32(np.inf)


def tetra():
    return nr.from_triangles(TETRAHEDRON)


def one(g, n, d):
    pl = sr.pack([n], [d])
    rec, counts = sr.whole(g, pl)
    return pl, rec, counts


def segs(rec):
    return [(tuple(r["p"].tolist()), tuple(r["q"].tolist())) for r in rec]


def test_hand_cases_on_the_tetrahedron():
    """TETRAHEDRON's faces, in load order: 0 the base z = 0, 1 in y = 0, 2 in x = 0, 3 in x + y + z = 4; vertices (0, 0, 0), (4, 0, 0),
    (0, 4, 0), (0, 0, 4).  All values are small integers and halves: every operation of the rule is exact."""
    g = tetra()
    # z = 2: the triangle (0, 0, 2), (2, 0, 2), (0, 2, 2), counter-clockwise seen from +z; area 2
    pl, rec, counts = one(g, (0, 0, 1), 2)
    assert counts.tolist() == [3] and rec["prim"].tolist() == [1, 2, 3] and rec["code"].tolist() == [6, 5, 6]
    assert segs(rec) == [((0, 0, 2), (2, 0, 2)), ((0, 2, 2), (0, 0, 2)), ((2, 0, 2), (0, 2, 2))]
    assert sr.areas(pl, rec, counts).tolist() == [2.0]
    # the same plane with the opposite normal: the same triangles, reversed segments; what was above is below
    pl, rec, counts = one(g, (0, 0, -1), -2)
    assert rec["prim"].tolist() == [1, 2, 3] and rec["code"].tolist() == [2, 1, 2]
    assert segs(rec) == [((2, 0, 2), (0, 0, 2)), ((0, 0, 2), (0, 2, 2)), ((0, 2, 2), (2, 0, 2))]
    assert sr.areas(pl, rec, counts).tolist() == [2.0]
    # z = 0: the base lies in the plane (all above), and the other faces have two vertices on it and one above: nothing
    pl, rec, counts = one(g, (0, 0, 1), 0)
    assert counts.tolist() == [0] and len(rec) == 0 and sr.areas(pl, rec, counts).tolist() == [0.0]
    # z = 4: the apex (0, 0, 4) is on the plane, so above, the others below: three zero-length segments
    pl, rec, counts = one(g, (0, 0, 1), 4)
    assert counts.tolist() == [3] and rec["prim"].tolist() == [1, 2, 3] and rec["code"].tolist() == [6, 5, 6]
    assert segs(rec) == [((0, 0, 4), (0, 0, 4))] * 3 and sr.areas(pl, rec, counts).tolist() == [0.0]
    # x + y + z = 4: face 3 lies in the plane and is not listed; the others give its three edges; area 8 sqrt(3)
    pl, rec, counts = one(g, (1, 1, 1), 4)
    assert rec["prim"].tolist() == [0, 1, 2] and rec["code"].tolist() == [0, 0, 0]
    assert segs(rec) == [((4, 0, 0), (0, 4, 0)), ((0, 0, 4), (4, 0, 0)), ((0, 4, 0), (0, 0, 4))]
    assert abs(sr.areas(pl, rec, counts)[0] - 8 * np.sqrt(3)) < 1e-12 * 8 * np.sqrt(3)
    # x = 1: a right triangle with legs 3; area 4.5
    pl, rec, counts = one(g, (1, 0, 0), 1)
    assert rec["prim"].tolist() == [0, 1, 3] and rec["code"].tolist() == [6, 5, 4]
    assert segs(rec) == [((1, 0, 0), (1, 3, 0)), ((1, 0, 3), (1, 0, 0)), ((1, 3, 0), (1, 0, 3))]
    assert sr.areas(pl, rec, counts).tolist() == [4.5]
    # the brute force agrees on all of them, and mode ANY is count > 0
    planes = sr.pack([(0, 0, 1), (0, 0, -1), (0, 0, 1), (0, 0, 1), (1, 1, 1), (1, 0, 0)], [2, -2, 0, 4, 4, 1])
    rec, counts = sr.whole(g, planes)
    brec, bcounts = sr.brute_force(g, planes, counts.astype(np.int64))
    assert counts.tolist() == [3, 3, 0, 3, 3, 3] and (bcounts == counts).all() and brec.tobytes() == rec.tobytes()
    assert sr.sections(g, planes, 0, sr.ANY)[1].tolist() == [1, 1, 0, 1, 1, 1]


def test_capacities_truncate_and_fill_with_the_miss_record():
    g = tetra()
    planes = sr.pack([(0, 0, 1), (0, 0, 1), (1, 0, 0)], [2, 0, 1])
    full, counts = sr.whole(g, planes)
    rec, c2 = sr.sections(g, planes, [2, 3, 5])
    assert (c2 == counts).all() and len(rec) == 10 and rec.dtype.itemsize == 32
    assert rec[:2].tobytes() == full[:2].tobytes()                            # the first cap records of the list
    assert rec[2:5].tobytes() == np.repeat(sr.MISS, 3).tobytes()              # nothing listed: miss records
    assert rec[5:8].tobytes() == full[3:6].tobytes() and rec[8:].tobytes() == np.repeat(sr.MISS, 2).tobytes()
    assert sr.MISS.tobytes() == bytes(12) + b"\xff\xff\xff\xff" + bytes(16)
    assert sr.caps_of([0, 2, 2, 9], 6).tolist() == [2, 0, 4]


def planes_for(g, n, seed):
    """About n planes: through vertices (s == 0 exactly for axis normals), random through the scene, scaled normals, far away, n = 0."""
    rng = np.random.default_rng(seed)
    lo, hi = nr.bounds(g)
    k = n // 4
    v = nr.tie_points(g, k, rng)
    axis = np.eye(3, dtype=np.float32)[rng.integers(0, 3, k)] * np.float32(rng.choice([-1, 1], k))[:, None]
    through = sr.pack(axis, nr.dot(axis, v))
    nn = rng.normal(size=(2 * k, 3)).astype(np.float32)
    pts = nr.box_points(g, 2 * k, rng)
    rand = sr.pack(nn, nr.dot(nn, pts))
    rand[::3] *= np.float32(1e-3)
    rand[1::3] *= np.float32(1e3)
    far = sr.pack(nn[:k], nr.dot(nn[:k], pts[:k]) + np.float32(100) * np.float32((hi - lo).max()) * np.linalg.norm(nn[:k], axis=1).astype(np.float32))
    zero = sr.pack(np.zeros((2, 3)), [0, 1])
    return np.concatenate([through, rand, far, zero]).astype(np.float32)


@pytest.fixture(scope="module", params=["cornell_box", "soup"])
def scene(request):
    if request.param == "soup":
        return nr.from_oracle(nr.oracle_soup(3000, 5, 2, 8))
    return nr.from_oracle(oracle.Scene.load_glb(scene_path("cornell_box")).build_bvh(20, 8))


def test_the_traversal_equals_the_brute_force(scene):
    """The cull is conservative for every triangle whose stored vertices lie in its leaf's box (monotonicity); what is left is the
    header's one-ulp remark, and on these scenes it does not occur: the two lists are the same bytes."""
    g = scene
    planes = planes_for(g, 120, 3)
    rec, counts = sr.whole(g, planes)
    brec, bcounts = sr.brute_force(g, planes, counts.astype(np.int64))
    print("%d planes, %d records, the longest list %d" % (len(planes), len(rec), counts.max()))
    assert counts.max() > (64 if len(g.v0) > 1000 else 16) and (counts == 0).any() and (bcounts == counts).all()
    assert brec.tobytes() == rec.tobytes()
    assert (sr.sections(g, planes, 0, sr.ANY)[1] == (counts > 0)).all()
    # ascending triangle index within every plane
    start = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    for i in range(len(planes)):
        assert (np.diff(rec["prim"][start[i]:start[i + 1]]) > 0).all()


def test_every_segment_runs_counter_clockwise_about_the_normal(scene):
    """dot(q - p, cross(n, fn)) >= 0 with fn = cross(e1, e2), evaluated in float64 on the fp32 records; rounding of the two cut points
    can turn a segment shorter than that rounding, so the bound is the rounding of the operands, not zero."""
    g = scene
    planes = planes_for(g, 120, 4)
    rec, counts = sr.whole(g, planes)
    owner = np.repeat(np.arange(len(planes)), counts.astype(np.int64))
    n = planes[owner, 0:3].astype(np.float64)
    t = rec["prim"]
    fn = np.cross(g.e1[t].astype(np.float64), g.e2[t].astype(np.float64))
    along = np.cross(n, fn)
    seg = rec["q"].astype(np.float64) - rec["p"].astype(np.float64)
    got = (seg * along).sum(axis=1)
    scale = np.abs(np.stack([rec["p"], rec["q"]])).max(axis=(0, 2)).astype(np.float64) * np.linalg.norm(along, axis=1)
    assert len(rec) > 500 and (got >= -8 * np.finfo(np.float32).eps * scale).all()
    assert (got > 0).mean() > 0.95


def test_the_cull_s_monotonicity_holds_in_fp32():
    """s(cmin) <= s(v) <= s(cmax) for every v inside the box, in fp32: each product and sum of s is monotone in each coordinate and
    rounding is monotone.  Random planes, boxes and points, with points on faces and corners and mixed signs and scales."""
    rng = np.random.default_rng(7)
    m = 400000
    scale = np.float32(10.0) ** rng.integers(-3, 4, (m, 1)).astype(np.float32)
    a, b = (rng.normal(size=(m, 3)).astype(np.float32) * scale), (rng.normal(size=(m, 3)).astype(np.float32) * scale)
    bmin, bmax = np.minimum(a, b), np.maximum(a, b)
    u = rng.uniform(0, 1, (m, 3)).astype(np.float32)
    u[rng.uniform(size=(m, 3)) < 0.2] = 0
    u[rng.uniform(size=(m, 3)) < 0.2] = 1
    v = np.clip(bmin + (bmax - bmin) * u, bmin, bmax).astype(np.float32)
    n = (rng.normal(size=(m, 3)) * 10.0 ** rng.integers(-3, 4, (m, 1))).astype(np.float32)
    n[rng.uniform(size=(m, 3)) < 0.1] = 0
    n[rng.uniform(size=(m, 3)) < 0.05] = np.float32(-0.0)
    d = (rng.normal(size=m) * 10.0 ** rng.integers(-3, 4, m)).astype(np.float32)
    cmin, cmax = sr.cull_corners(n, bmin, bmax)
    s_lo, s_v, s_hi = sr.signed(n, d, cmin), sr.signed(n, d, v), sr.signed(n, d, cmax)
    assert (s_lo <= s_v).all() and (s_v <= s_hi).all()
    # so a box whose cull fails holds no vertex on one of the two sides
    passes = sr.cull_passes(n, d, bmin, bmax)
    assert passes.any() and (~passes).any()
    assert (((s_lo >= 0) & (s_v >= 0)) | ((s_hi < 0) & (s_v < 0)))[~passes].all()


def test_a_tree_with_exchanged_children_gives_the_same_ascending_lists(scene):
    g = scene
    swapped = g._replace(child1=g.child2, child2=g.child1)
    planes = planes_for(g, 60, 5)
    for caps in (3, np.random.default_rng(1).integers(0, 9, len(planes))):
        rec, counts = sr.sections(g, planes, caps)
        rec2, counts2 = sr.sections(swapped, planes, caps)
        assert rec.tobytes() == rec2.tobytes() and (counts == counts2).all()
    rec, counts = sr.whole(swapped, planes)
    start = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    assert all((np.diff(rec["prim"][start[i]:start[i + 1]]) > 0).all() for i in range(len(planes)))


def test_invalid_planes_and_a_zero_normal_list_nothing():
    g = tetra()
    good = sr.pack([(0, 0, 1)], [2])
    assert sr.sections(g, good, 0)[1].tolist() == [3]
    for word in range(4):
        for value in (NAN, INF, -INF):
            bad = good.copy()
            bad[0, word] = value
            assert not sr.valid(bad).any()
            visits = np.zeros(1, np.int64)
            rec, counts = sr.sections(g, bad, 2, visits=visits)
            assert counts.tolist() == [0] and rec.tobytes() == np.repeat(sr.MISS, 2).tobytes() and not visits.any()   # nothing is pushed
            assert sr.sections(g, bad, 0, sr.ANY)[1].tolist() == [0] and sr.brute_force(g, bad, 0)[1].tolist() == [0]
    assert sr.valid(np.full((1, 4), np.finfo(np.float32).max, np.float32)).all()       # FLT_MAX itself is valid
    for d in (0, 1, -1):                                                                 # n = 0 is valid and cuts nothing
        zero = sr.pack([(0, 0, 0)], [d])
        assert sr.valid(zero).all() and sr.sections(g, zero, 0)[1].tolist() == [0] and sr.brute_force(g, zero, 0)[1].tolist() == [0]
    # -0.0 components are >= 0: the same corners, the same records as +0.0
    a, b = sr.pack([(0.0, 0.0, 1)], [2]), sr.pack([(-0.0, -0.0, 1)], [2])
    assert sr.whole(g, a)[0].tobytes() == sr.whole(g, b)[0].tobytes()
    # an empty scene and no planes
    empty = nr.from_triangles(np.zeros((0, 3, 3)))
    rec, counts = sr.sections(empty, good, 3)
    assert rec.tobytes() == np.repeat(sr.MISS, 3).tobytes() and counts.tolist() == [0]
    rec, counts = sr.sections(g, np.zeros((0, 4), np.float32), 2)
    assert len(rec) == 0 and len(counts) == 0 and counts.dtype == np.uint32 and rec.dtype == sr.SECTION
