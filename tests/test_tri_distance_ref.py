"""What the restatement of the triangle distance query (tests/tri_distance_ref.py, include/drt.h drt_renderer_triangle_distance) is
worth, without a GPU: hand cases with the deciding candidate, zero-area and non-finite input, an exact check on small integers in
fractions.Fraction, the tree against the brute force and against the same rule in float64, and the working range.
tests/test_gpu_tri_distance.py compares the kernel with this restatement bit for bit."""
from fractions import Fraction

import numpy as np
import pytest

import oracle
from tests import nearest_ref as nr
from tests import tri_distance_ref as td
from tests import tri_overlap_ref as tv
from tests.scenes import scene_path
from tests.test_tri_overlap_ref import area_is_zero, as_tuples, triangles_meet

NAN, INF = np.float32(np.nan), np.float32(np.inf)
T = np.float32([[[0, 0, 0], [4, 0, 0], [0, 4, 0]]])             # the scene of the hand cases

# (query, d2, feature) against T.  feature = the deciding candidate, | 16 where the pair touches.
HAND_CASES = [
    ([(1, 1, 2), (1, 2, 3), (2, 1, 3)], 4.0, 0),                # vertex-face: the query's vertex 0 over the interior
    ([(1, 2, 3), (1, 1, 2), (2, 1, 3)], 4.0, 1),                # ... its vertex 1
    ([(-10, -10, 1), (20, -10, 1), (-10, 20, 1)], 1.0, 3),      # face-vertex: a large query above, the scene's v0 below its interior
    ([(5, -1, 1), (5, 5, 1), (9, 2, 1)], 2.0, 4),               # ... the scene's v1 under the query's edge 0: the vertex comes first
    ([(2, -1, 1), (2, -1, 3), (2, -3, 1)], 2.0, 0),             # a vertex against the edge v0 v1
    ([(1, -2, 1), (3, -2, 3), (2, -6, 2)], 5.0, 0),             # the query's vertex 0 is nearest, outside the edge
    ([(1, -1, 1), (3, -1, -1), (2, -5, 0)], 1.0, 6),            # crossed edges: query edge 0 over scene edge 0, both interiors
    ([(3, 3, 1), (5, 5, 3), (5, 5, -1)], 3.0, 0),               # (vertex 0 against the hypotenuse: (3, 3, 1) to (2, 2, 0))
    ([(1, -1, 0), (3, -1, 0), (2, -3, 0)], 1.0, 0),             # parallel edges in the plane: the first of the tied candidates
    ([(5, 5, 0), (9, 5, 0), (5, 9, 0)], 18.0, 0),               # parallel coplanar offset triangles
    ([(0, 0, 1), (4, 0, 1), (0, 4, 1)], 1.0, 0),                # parallel planes, the same triangle one above
    ([(0, 0, 0), (-4, 0, 1), (0, -4, 1)], 0.0, 16),             # a shared vertex
    ([(0, 0, 0), (4, 0, 0), (0, 0, 4)], 0.0, 16),               # a shared edge
    ([(1, 1, -1), (1, 1, 1), (1.25, 1.125, 1)], 0.0, 16),       # an edge through the interior: 0 by the predicate alone
    ([(0, 0, 0), (4, 0, 0), (0, 4, 0)], 0.0, 16),               # identical
]


def one(q, max_dist=None, mode=td.NEAREST, scene=T):
    return td.distance(nr.from_triangles(scene), np.float32(q).reshape(-1, 3, 3), max_dist, mode)


def test_hand_cases_and_their_deciding_candidates():
    q = np.float32([c[0] for c in HAND_CASES])
    res = one(q)
    assert res.d2.tolist() == [c[1] for c in HAND_CASES]
    assert res.feature.tolist() == [c[2] for c in HAND_CASES]
    assert (res.prim == 0).all()
    # the witness points lie on the two triangles and are d2 apart where the pair does not touch; (u, v) are point_t's
    apart = res.feature < 16
    diff = (res.point_q - res.point_t)[apart]
    assert (nr.dot(diff, diff) == res.d2[apart]).all()
    g = nr.from_triangles(T)
    assert (res.point_t == (g.v0[0] + g.e1[0] * res.u[:, None]) + g.e2[0] * res.v[:, None]).all()
    assert res.point_q[0].tolist() == [1, 1, 2] and res.point_t[0].tolist() == [1, 1, 0] and (res.u[0], res.v[0]) == (0.25, 0.25)
    assert res.point_q[2].tolist() == [0, 0, 1] and res.point_t[2].tolist() == [0, 0, 0]
    assert res.point_q[6].tolist() == [2, -1, 0] and res.point_t[6].tolist() == [2, 0, 0] and (res.u[6], res.v[6]) == (0.5, 0)
    # the edge through the interior: every one of the fifteen candidates is positive, the predicate alone says 0; the witness is
    # that of the best candidate and is not a contact point
    pierce = q[13]
    each = np.array([c[0] for c in td.candidates(pierce[0], pierce[1], pierce[2], g.v0[0], g.e1[0], g.e2[0])])
    assert each.shape == (15,) and (each > 0).all()
    p = td.pair(pierce[0], pierce[1], pierce[2], g.v0[0], g.e1[0], g.e2[0])
    assert p.candidates_d2 == each.min() > 0 and p.d2 == 0 and p.feature == 16 + int(each.argmin())
    assert (res.point_q[13] != res.point_t[13]).any()
    # mode ANY on one triangle is the same record; a distance below the pair's finds nothing, the pair's own neither (strict <)
    assert td.records(one(q, mode=td.ANY)).tobytes() == td.records(res).tobytes()
    assert one(q[0], 2.0).prim[0] == -1 and one(q[0], 2.0).d2[0] == 4.0 and one(q[0], np.float32(2.0001)).prim[0] == 0


def test_zero_area_triangles_on_either_side_are_segments_and_points():
    seg = [(1, 1, 3), (3, 1, 3), (3, 1, 3)]                      # q1 = q2: a segment above the interior
    pt = [(1, 1, 2)] * 3
    res = one([seg, pt, [(6, 0, 0), (8, 0, 0), (7, 0, 0)], [(1, 1, 0)] * 3])
    assert res.d2.tolist() == [9.0, 4.0, 4.0, 0.0] and res.prim.tolist() == [0] * 4 and res.feature[3] >= 16
    # a scene of a segment and a point
    flat = np.float32([[[0, 0, 0], [4, 0, 0], [4, 0, 0]], [[0, 5, 0]] * 3])
    res = one([[(1, 0, 2), (2, 0, 2), (1, 1, 2)], [(0, 5, 3), (1, 5, 3), (0, 6, 3)]], scene=flat)
    assert res.d2.tolist() == [4.0, 9.0] and res.prim.tolist() == [0, 1]
    # v0 = v1 in the scene: candidates whose case divides 0 by 0 are NaNs and never win; the others still measure the segment
    res = one([[(1, 0, 2), (2, 0, 2), (1, 1, 2)]], scene=np.float32([[[0, 0, 0], [0, 0, 0], [4, 0, 0]]]))
    assert res.d2.tolist() == [4.0] and res.prim.tolist() == [0]


def test_non_finite_input_and_the_miss_record():
    q = np.float32([[(1, 1, 2), (1, 2, 3), (2, 1, 3)]] * 6)
    q[1, 0, 1], q[2, 2, 2], q[3, 1, 0] = NAN, INF, -INF
    md = np.float32([INF, INF, INF, INF, NAN, 0])
    for mode in (td.NEAREST, td.ANY):
        rec = td.records(one(q, md, mode))
        assert rec[0, 3] == 4 and rec.view(np.int32)[0, 7] == 0
        miss = rec[1:]
        assert (miss.view(np.int32)[:, 7] == -1).all() and not miss[:, [0, 1, 2, 4, 5, 6, 8, 9, 10, 11]].any()
        assert np.isinf(miss[:3, 3]).all() and np.isnan(miss[3, 3]) and miss[4, 3] == 0          # d2 = max_dist * max_dist
    # an empty scene and an empty batch
    none = td.distance(nr.from_triangles(np.zeros((0, 3, 3))), q, 3.0)
    assert (none.prim == -1).all() and (none.d2 == 9).all() and not none.point_q.any()
    assert len(td.distance(nr.from_triangles(T), np.zeros((0, 3, 3), np.float32)).d2) == 0
    # a negative max_dist searches as its absolute value does
    assert td.records(one(q[:1], -3.0)).tobytes() == td.records(one(q[:1], 3.0)).tobytes()
    # overflow does not raise: the products are infinities and NaNs, and a NaN never wins
    big = one(np.float32([[(1e30, 1e30, -1e30), (1e30, 1e30, 1e30), (5e30, 5e30, 0)]]))
    assert big.prim[0] == -1 and np.isinf(big.d2[0])


# ---- the exact distance of two integer triangles in fractions.Fraction, by another route than the rule's: a point against a triangle is
# the plane distance where the foot lies inside and else the nearest of the three edges; two segments are the distance of their lines
# where both feet lie inside and else the nearest of the four ends against the other segment.
def _sub(a, b):
    return tuple(x - y for x, y in zip(a, b))


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def point_segment2(p, a, b):
    d = _sub(b, a)
    t = min(max(Fraction(_dot(_sub(p, a), d), _dot(d, d)), 0), 1) if _dot(d, d) else Fraction(0)
    w = tuple(x - (y + t * z) for x, y, z in zip(p, a, d))
    return _dot(w, w)


def point_triangle2(p, t):
    n = _cross(_sub(t[1], t[0]), _sub(t[2], t[0]))
    if all(_dot(_cross(_sub(t[(i + 1) % 3], t[i]), _sub(p, t[i])), n) >= 0 for i in range(3)):
        return Fraction(_dot(_sub(p, t[0]), n) ** 2, _dot(n, n))
    return min(point_segment2(p, t[i], t[(i + 1) % 3]) for i in range(3))


def segment_segment2(a, b, c, d):
    d1, d2, r = _sub(b, a), _sub(d, c), _sub(a, c)
    n = _cross(d1, d2)
    best = min(point_segment2(a, c, d), point_segment2(b, c, d), point_segment2(c, a, b), point_segment2(d, a, b))
    if n != (0, 0, 0):
        A, E, F, C, B = _dot(d1, d1), _dot(d2, d2), _dot(d2, r), _dot(d1, r), _dot(d1, d2)
        den = A * E - B * B
        s, t = Fraction(B * F - C * E, den), Fraction(A * F - B * C, den)
        if 0 <= s <= 1 and 0 <= t <= 1:
            best = min(best, Fraction(_dot(r, n) ** 2, _dot(n, n)))
    return best


def exact_distance2(a, b):
    """Of two integer triangles of non-zero area that do not meet."""
    edges = lambda t: [(t[i], t[(i + 1) % 3]) for i in range(3)]
    return min([point_triangle2(p, b) for p in a] + [point_triangle2(p, a) for p in b] +
               [segment_segment2(*e, *f) for e in edges(a) for f in edges(b)])


# What fp32 adds to the exact answer on integers of magnitude <= 4: the dot products, va, vb, vc and den are integers below 2^24 and
# exact, so every case is the exact one; the quotients u, v, s, t round (2^-24 relative, times an edge of length <= 14), and each
# coordinate of a witness point takes two products and two sums, each within half an ulp of a value below 16 (2^-21).  That is at
# most 5 * 2^-21 per coordinate and point, 10 * 2^-21 for the difference, sqrt(3) of it for the vector: below 18 * 2^-21 = 2^-17 * 1.1.
# The three squares and two sums of dist2 add 2^-22 relative.  The bound below is 2^-16.
EXACT_BOUND = 2.0 ** -16


@pytest.mark.parametrize("span, n", [(2, 700), (4, 1500)])
def test_on_small_integers_the_pair_distance_is_the_exact_one(span, n):
    rng = np.random.default_rng(40 + span)
    A, B = rng.integers(-span, span + 1, (n, 3, 3)), rng.integers(-span, span + 1, (n, 3, 3))
    B[::2] += rng.integers(-2, 3, (len(B[::2]), 1, 3)) * span                 # half of them further apart: fewer pairs that meet
    a32, b32 = A.astype(np.float32), B.astype(np.float32)
    p = td.pair(a32[:, 0], a32[:, 1], a32[:, 2], b32[:, 0], b32[:, 1] - b32[:, 0], b32[:, 2] - b32[:, 0])
    pairs = meets = equal = 0
    worst = 0.0
    for a, b, d2, feature in zip(as_tuples(A), as_tuples(B), p.d2.tolist(), p.feature.tolist()):
        if area_is_zero(a) or area_is_zero(b):
            continue
        pairs += 1
        meet = triangles_meet(a, b)
        meets += meet
        assert (d2 == 0) == meet and (feature >= 16) == meet, (a, b, d2, feature)   # 0 exactly where the exact test says they meet
        if not meet:
            exact = exact_distance2(a, b)
            equal += Fraction(d2) == exact
            worst = max(worst, abs(d2 ** 0.5 - float(exact) ** 0.5))
    print("[-%d, %d]: %d pairs, %d meet, %d of the %d others bit-exact, worst |dist - exact| = %.3g (bound %.3g)" %
          (span, span, pairs, meets, equal, pairs - meets, worst, EXACT_BOUND))
    assert pairs > n // 2 and pairs // 10 < meets < pairs * 9 // 10 and equal > 0
    assert worst <= EXACT_BOUND


# ---- the tree against the brute force and the float64 yardstick
# B of the accuracy bound |sqrt(d2) - sqrt(d2_float64)| <= B * 2^-23 * M, M the largest absolute coordinate of query and scene: four
# times the largest ratio measured with the float64 yardstick on the two scenes below (DESIGN 5.27 has both numbers), as 5.15 does.
MEASURED_RATIO = {"soup": 0.73, "cornell_box": 0.69}
B = 4 * max(MEASURED_RATIO.values())
MISMATCH_CAP = 0.005
_scenes = {}


def scene(name):
    if name not in _scenes:
        osc = nr.oracle_soup(3000, 5, 2, 8) if name == "soup" else oracle.Scene.load_glb(scene_path(name)).build_bvh(20, 8)
        _scenes[name] = nr.from_oracle(osc)
    return _scenes[name]


@pytest.mark.parametrize("name, seed, n", [("soup", 1, 300), ("cornell_box", 2, 300)])
def test_the_tree_equals_the_brute_force_and_stays_within_the_accuracy_bound(name, seed, n):
    g = scene(name)
    q = td.query_triangles(g, n, np.random.default_rng(seed))
    visits, tests = np.zeros(len(q), np.int64), np.zeros(len(q), np.int64)
    tree = td.distance(g, q, visits=visits, tests=tests)
    brute, brute_prim, _ = td.brute_force(g, q)
    exact, _, _ = td.brute_force(g, q, dtype=np.float64)
    M = td.scale_of(g, q)
    err = lambda d2: np.abs(np.sqrt(d2.astype(np.float64)) - np.sqrt(exact)) / (2.0 ** -23 * M)
    differ = tree.d2 != brute
    print("%s: %d queries, %d differ from the brute force; %.1f nodes (max %d) and %.1f pairs per query; largest ratio tree %.3f, brute %.3f; "
          "%d touch" % (name, len(q), differ.sum(), visits.mean(), visits.max(), tests.mean(), err(tree.d2).max(), err(brute).max(), (tree.d2 == 0).sum()))
    assert (tree.prim >= 0).all() and (tree.d2 >= brute).all()                # the tree tests a subset of the pairs
    assert differ.mean() <= MISMATCH_CAP
    assert (err(tree.d2) <= B).all() and (err(brute) <= B).all()
    assert err(brute).max() <= MEASURED_RATIO[name] <= 1.05 * err(brute).max() + 0.01    # the figure in DESIGN 5.27 is this one
    # with a distance: the same answers below it, the miss record at and beyond
    md = (np.sqrt(np.median(brute)) * np.ones(len(q))).astype(np.float32)
    near = td.distance(g, q, md)
    inside = tree.d2 < md * md
    assert (near.prim[inside] == tree.prim[inside]).all() and (near.d2[inside] == tree.d2[inside]).all()
    assert (near.prim[~inside] == -1).all() and (near.d2[~inside] == md[~inside] * md[~inside]).all() and inside.any() and (~inside).any()
    # mode ANY: the boolean is the same, the record is a pair within the distance and is the first one the traversal meets
    first = td.distance(g, q, md, td.ANY)
    assert ((first.prim >= 0) == inside).all() and (first.d2[inside] < (md * md)[inside]).all() and (first.d2 >= near.d2)[inside].all()
    assert (first.prim != near.prim).any()


# ---- the working range (include/drt.h "working range of the mesh queries")
SCALE_RANGE = (-30, 26)           # exponents of two between which every answer is the plain answer scaled, in steps of 2^2


def test_working_range_scaling_by_powers_of_two():
    """A mesh with edges of 2^-2 to 2^4 and queries up to 2^7 from it, as the header's paragraph describes the other queries' mesh."""
    rng = np.random.default_rng(6)
    n = 60
    size = np.float32(2.0) ** rng.integers(-2, 5, (n, 1, 1)).astype(np.float32)
    mesh = (rng.uniform(-40, 40, (n, 1, 3)) + rng.uniform(-1, 1, (n, 3, 3)) * size).astype(np.float32)
    qsize = np.float32(2.0) ** rng.integers(-2, 5, (n, 1, 1)).astype(np.float32)
    q = (rng.uniform(-128, 128, (n, 1, 3)) + rng.uniform(-1, 1, (n, 3, 3)) * qsize).astype(np.float32)
    q[:12] = mesh[:12] + np.float32(0.125)                                    # close pairs, and some that touch
    q[12:18] = mesh[12:18]
    base = td.distance(nr.from_triangles(mesh), q)
    assert (base.prim >= 0).all() and (base.d2 == 0).any() and (base.d2 > 0).any()

    def unchanged(e):
        s = np.float32(2.0) ** np.float32(e)
        r = td.distance(nr.from_triangles(mesh * s), q * s)
        return ((r.prim == base.prim).all() and (r.feature == base.feature).all() and (r.u == base.u).all() and (r.v == base.v).all() and
                (r.d2 == base.d2 * s * s).all() and (r.point_q == base.point_q * s).all() and (r.point_t == base.point_t * s).all())

    ok = {e: unchanged(e) for e in range(-40, 38, 2)}
    lo = min(e for e in ok if all(ok[x] for x in ok if e <= x <= 0))
    hi = max(e for e in ok if all(ok[x] for x in ok if 0 <= x <= e))
    print("unchanged for 2^%d to 2^%d" % (lo, hi))
    assert (lo, hi) == SCALE_RANGE
    assert not ok[lo - 2] and not ok[hi + 2]
