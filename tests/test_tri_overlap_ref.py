"""The triangle overlap rule of include/drt.h as tests/tri_overlap_ref.py restates it (CPU only): against an independent exact test in
Python integers on inputs where every fp32 intermediate is exact, hand cases, zero-area queries, non-finite and overflowing
coordinates, the traversal against the brute force, and the insert over a tree with exchanged children."""
import os
import re
import warnings

import numpy as np
import pytest

import oracle
from tests import nearest_ref as nr
from tests import ray_query_ref as rq
from tests import refit_ref as rf
from tests import tri_overlap_ref as tv
from tests.scenes import ROOT, scene_path

NAN, INF = np.float32(np.nan), np.float32(np.inf)


# ---- the exact test: Python integers only.  Two closed triangles of non-zero area meet iff an edge of one meets the other closed
# triangle (if they share a point, follow the intersection set, a point, a segment or a polygon, to its boundary: an end of it lies on
# an edge of one of the two).  A segment P Q against a triangle T with normal n: the signed heights dp, dq of P and Q over T's
# plane; both on one side: no; both zero: the 2-D branch in the plane; else the one crossing point X, compared with T's three edges.
def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _orient(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def _on_segment(a, b, c):
    """c, known collinear with a b, lies on the closed segment a b."""
    return min(a[0], b[0]) <= c[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= c[1] <= max(a[1], b[1])


def _segments_meet_2d(a, b, c, d):
    o1, o2, o3, o4 = _orient(a, b, c), _orient(a, b, d), _orient(c, d, a), _orient(c, d, b)
    if ((o1 > 0 and o2 < 0) or (o1 < 0 and o2 > 0)) and ((o3 > 0 and o4 < 0) or (o3 < 0 and o4 > 0)):
        return True
    return (o1 == 0 and _on_segment(a, b, c)) or (o2 == 0 and _on_segment(a, b, d)) or (o3 == 0 and _on_segment(c, d, a)) or (o4 == 0 and _on_segment(c, d, b))


def _point_in_triangle_2d(p, t):
    o = [_orient(t[0], t[1], p), _orient(t[1], t[2], p), _orient(t[2], t[0], p)]
    return all(x >= 0 for x in o) or all(x <= 0 for x in o)


def segment_meets_triangle(P, Q, T):
    """The closed segment P Q (P == Q: a point) meets the closed triangle T of non-zero area.  Integers in, exact."""
    n = _cross(_sub(T[1], T[0]), _sub(T[2], T[0]))
    assert n != (0, 0, 0)
    dp, dq = _dot(n, _sub(P, T[0])), _dot(n, _sub(Q, T[0]))
    if (dp > 0 and dq > 0) or (dp < 0 and dq < 0):
        return False
    if dp == 0 and dq == 0:                                     # the segment lies in the plane: drop the normal's largest axis
        k = max(range(3), key=lambda i: abs(n[i]))
        flat = lambda v: tuple(v[i] for i in range(3) if i != k)
        p, q, t = flat(P), flat(Q), [flat(v) for v in T]
        return (_point_in_triangle_2d(p, t) or _point_in_triangle_2d(q, t) or
                any(_segments_meet_2d(p, q, t[i], t[(i + 1) % 3]) for i in range(3)))
    # X = P + (dp / D) (Q - P), D = dp - dq != 0; XD = X * D is integral.  X is in T iff, for each edge a b,
    # dot(cross(b - a, X - a), n) >= 0, and X - a = (XD - a D) / D: multiply by D's sign.
    D = dp - dq
    d = _sub(Q, P)
    XD = (P[0] * D + dp * d[0], P[1] * D + dp * d[1], P[2] * D + dp * d[2])
    sign = 1 if D > 0 else -1
    for i in range(3):
        a, b = T[i], T[(i + 1) % 3]
        rel = (XD[0] - a[0] * D, XD[1] - a[1] * D, XD[2] - a[2] * D)
        if sign * _dot(_cross(_sub(b, a), rel), n) < 0:
            return False
    return True


def area_is_zero(T):
    return _cross(_sub(T[1], T[0]), _sub(T[2], T[0])) == (0, 0, 0)


def triangles_meet(A, B):
    return (any(segment_meets_triangle(A[i], A[(i + 1) % 3], B) for i in range(3)) or
            any(segment_meets_triangle(B[i], B[(i + 1) % 3], A) for i in range(3)))


def rule(A, B):
    """bool [N]: the restated rule on query A[i] against triangle B[i] (integer arrays [N, 3, 3])."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    return tv.triangle_listed(A[:, 0], A[:, 1], A[:, 2], B[:, 0], B[:, 1] - B[:, 0], B[:, 2] - B[:, 0])


def as_tuples(a):
    return [tuple(tuple(int(x) for x in v) for v in t) for t in a]


@pytest.mark.parametrize("span, flat, n", [(3, False, 60000), (2, False, 60000), (6, False, 60000), (4, True, 60000)])
def test_the_rule_is_the_exact_test_where_fp32_is_exact(span, flat, n):
    """Integer coordinates of magnitude <= 6: differences <= 12, the axes' components <= 2 * 12^2 (the normals) and <= 2 * 12 * 288
    (cross(n, edge)), a projection <= 3 * 6912 * 12 < 2^18 -- every fp32 intermediate is an integer below 2^24, so the rule computes in
    real arithmetic, and for triangles of non-zero area it must EQUAL the exact test: no tolerance."""
    rng = np.random.default_rng(100 + span + (50 if flat else 0))
    A, B = rng.integers(-span, span + 1, (n, 3, 3)), rng.integers(-span, span + 1, (n, 3, 3))
    if flat:
        A[:, :, 2] = 0
        B[:, :, 2] = 0
    got = rule(A, B)
    pairs = missed = extra = meets = 0
    for a, b, listed in zip(as_tuples(A), as_tuples(B), got.tolist()):
        if area_is_zero(a) or area_is_zero(b):
            continue
        exact = triangles_meet(a, b)
        pairs += 1
        meets += exact
        missed += exact and not listed
        extra += listed and not exact
    print("[-%d, %d]%s: %d pairs, %d intersect, %d missed, %d extra" % (span, span, " coplanar" if flat else "", pairs, meets, missed, extra))
    assert pairs > n // 2 and pairs // 5 < meets < pairs * 9 // 10
    assert missed == 0 and extra == 0


def test_the_restatement_s_axes_are_the_header_s_in_its_order():
    """triangle_axes returns the seventeen axes in the order in which include/drt.h numbers them, which is what lets the hand cases
    below name the groups by index: 0 nq, 1 nt, 2..10 cross(A, E) with A outer, 11..13 cross(nq, A), 14..16 cross(nt, E)."""
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    sec = re.sub(r"\s*\n \*\s*", " ", text[text.index("triangle overlap queries (new"):text.index("typedef struct drt_tri ")])
    at = [sec.index(p) for p in ("Seventeen axes L, in this order", "1. nq", "2. nt", "3. cross(A, E) for A in (a1, g, a2) (outer) and E in (e1, h, e2) (inner)",
                                 "4. cross(nq, A) for A in (a1, g, a2)", "5. cross(nt, E) for E in (e1, h, e2)", "listed iff all seventeen are ok")]
    assert at == sorted(at)
    # one pair per group that only that group separates, found by the restatement: the index ranges are the header's groups
    q = np.float32([[(0, 0, 1), (4, 0, 1), (0, 4, 1)],             # parallel planes: the normals (and cross products of non-parallel edges)
                    [(3, 3, 0), (5, 3, 0), (3, 5, 0)]])            # coplanar and apart: in-plane edge normals only
    t = np.float32([[(0, 0, 0), (4, 0, 0), (0, 4, 0)]] * 2)
    ok = tv.triangle_axes(q[:, 0], q[:, 1], q[:, 2], t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    assert ok.shape == (2, 17)
    assert not ok[0, 0] and not ok[0, 1] and ok[0, 11:].all()
    assert ok[1, :11].all() and not ok[1, 11:].all()
    # cross(a1, e1) with a1 = (4, 0, 0), e1 = (4, 0, 0) vanishes (axis 2 passes); cross(a1, h), h = (-4, 4, 0), is (0, 0, 16) and separates
    assert ok[0, 2] and not ok[0, 3]


T = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]
HAND = [("shared vertex", [(0, 0, 0), (-4, 0, 1), (0, -4, 1)], True),          # Q lies in x <= 0, y <= 0: it meets T at the origin only
        ("shared edge", [(0, 0, 0), (4, 0, 0), (0, 0, 4)], True),               # Q stands on the edge y = 0 of T
        ("edge through interior", [(1, 1, -1), (1, 1, 1), (5, 5, 0)], True),    # the edge x = y = 1 crosses z = 0 at (1, 1, 0), 1 + 1 < 4
        ("coplanar contained", [(1, 1, 0), (2, 1, 0), (1, 2, 0)], True),        # x + y <= 3 < 4
        ("coplanar disjoint", [(3, 3, 0), (5, 3, 0), (3, 5, 0)], False),        # x + y >= 6 > 4
        ("parallel planes", [(0, 0, 1), (4, 0, 1), (0, 4, 1)], False),          # T lifted by 1
        ("identical", T, True)]


def test_hand_cases():
    for name, Q, want in HAND:
        assert triangles_meet(Q, T) == want, name
        assert rule([Q], [T]).tolist() == [want], name
        assert rule([T], [Q]).tolist() == [want], name                          # either one may be the query
    q = lambda name: np.float32([[Q for n, Q, _ in HAND if n == name][0]])
    t = np.float32([T])
    axes = lambda Q: tv.triangle_axes(Q[:, 0], Q[:, 1], Q[:, 2], t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])[0]
    # coplanar and disjoint: the two normals see height 0 on both sides and the nine cross products are parallel to z and vanish
    # on every in-plane vector -- the 11 standard axes pass with 0 <= 0 and only in-plane edge normals separate
    ok = axes(q("coplanar disjoint"))
    assert ok[:11].all() and not ok[11:].all()
    # parallel planes: both normals are (0, 0, 16): sq = (0, 0, 0), st = (-16, -16, -16) and the reverse; the nine cross products of
    # in-plane edges are parallel to z too and separate as well, where they do not vanish (parallel edges)
    ok = axes(q("parallel planes"))
    assert not ok[0] and not ok[1] and ok[11:].all()
    # the scene's own triangle lists itself: every axis passes
    assert axes(q("identical")).all()


def test_zero_area_queries_never_miss():
    """A segment or a point as the query against a triangle of non-zero area: conservative -- where the exact test says touch, the
    rule lists (it may list more, in the triangle's own plane)."""
    t = np.float32([T])
    cases = [("a segment through the interior", [(1, 1, -2), (1, 1, 2), (1, 1, 2)], True),
             ("a collinear triple through the interior", [(1, 1, -2), (1, 1, 0), (1, 1, 2)], True),
             ("a segment that ends on the triangle", [(1, 1, 0), (1, 1, 3), (1, 1, 0)], True),
             ("a segment above", [(1, 1, 1), (2, 1, 1), (2, 1, 1)], False),
             ("a segment beside, crossing the plane", [(5, 5, -1), (5, 5, 1), (5, 5, 1)], False),
             ("a point on it", [(1, 1, 0)] * 3, True), ("a point on a vertex", [(4, 0, 0)] * 3, True),
             ("a point above it", [(1, 1, 1)] * 3, False), ("a point in its plane, outside", [(3, 3, 0)] * 3, False)]
    for name, Q, want in cases:
        ends = sorted(set(Q))
        assert segment_meets_triangle(ends[0], ends[-1], T) == want, name
        assert rule([Q], [T]).tolist() == [want], name
        assert rule([T], [Q]).tolist() == [want], name                          # a zero-area triangle of the mesh, too
    # random integer segments and points: exact says touch => listed; what the rule lists beyond is counted
    rng = np.random.default_rng(5)
    n = 4000
    P, Q = rng.integers(-3, 4, (n, 3)), rng.integers(-3, 4, (n, 3))
    Q[: n // 4] = P[: n // 4]                                                   # points
    B = rng.integers(-3, 4, (n, 3, 3))
    A = np.stack([P, Q, Q], axis=1)
    got = rule(A, B)
    touches = extra = 0
    for p, q, b, listed in zip(as_tuples(P[:, None])[:], as_tuples(Q[:, None]), as_tuples(B), got.tolist()):
        if area_is_zero(b):
            continue
        exact = segment_meets_triangle(p[0], q[0], b)
        touches += exact
        assert listed or not exact, (p, q, b)
        extra += listed and not exact
    print("zero-area queries: %d touch, the rule lists %d more" % (touches, extra))
    assert touches > 100


def test_non_finite_queries_list_nothing_and_overflow_does_not_raise():
    g = nr.from_triangles(np.float32([T]))
    good = np.float32([[(1, 1, -1), (1, 1, 1), (5, 5, 0)]])
    assert tv.overlap(g, good, 1)[1].tolist() == [1] and tv.brute_force(g, good, 1)[1].tolist() == [1]
    for word in range(9):
        for value in (NAN, INF, -INF):
            bad = tv.pack(good)
            bad[0, word] = value
            assert not tv.valid(tv.unpack(bad)).any()
            visits = np.zeros(1, np.int64)
            prims, counts = tv.overlap(g, bad, 2, visits=visits)
            assert counts.tolist() == [0] and prims.tolist() == [-1, -1] and not visits.any(), word      # nothing is pushed
            assert tv.overlap(g, bad, 0, tv.ANY)[1].tolist() == [0] and tv.brute_force(g, bad, 2)[1].tolist() == [0]
    # without the validity rule fminf would drop a NaN vertex from the bounds: they are finite
    bad = tv.unpack(good).copy()
    bad[0, 2] = NAN
    lo, hi = tv.bounds_of(bad)
    assert np.isfinite(lo).all() and np.isfinite(hi).all()
    for word in (9, 10, 11):                                                    # the pad words are ignored
        pad = tv.pack(good)
        pad[0, word] = NAN
        assert tv.overlap(g, pad, 1)[1].tolist() == [1]
    # FLT_MAX itself is valid
    assert tv.valid(np.full((1, 3, 3), np.finfo(np.float32).max, np.float32)).all()
    # coordinates about 1e30: the normals overflow to infinities, their projections to NaN, and a NaN comparison fails
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        big = nr.from_triangles(np.float32([T]) * np.float32(1e30))
        for q in (good * np.float32(1e30), np.float32([T]) * np.float32(1e30), good):
            assert tv.valid(q).all()
            assert tv.overlap(big, q, 1)[1].tolist() == [0] and tv.brute_force(big, q, 1)[1].tolist() == [0]
        assert tv.overlap(g, good * np.float32(1e30), 1)[1].tolist() == [0]
    # an empty scene and no queries
    empty = nr.from_triangles(np.zeros((0, 3, 3)))
    prims, counts = tv.overlap(empty, good, 3)
    assert prims.tolist() == [-1] * 3 and counts.tolist() == [0] and tv.brute_force(empty, good, 3)[1].tolist() == [0]
    prims, counts = tv.overlap(g, np.zeros((0, 3, 3), np.float32), 2)
    assert len(prims) == 0 and len(counts) == 0 and counts.dtype == np.uint32 and prims.dtype == np.int32


def integer_soup(n, seed, leaf=2):
    """n small triangles of non-zero area with integer coordinates in [-6, 6], under the oracle's tree."""
    rng = np.random.default_rng(seed)
    pos = rng.integers(-5, 6, (2 * n, 1, 3)) + rng.integers(-1, 2, (2 * n, 3, 3))
    pos = pos[[not area_is_zero(t) for t in as_tuples(pos)]][:n].astype(np.float32)
    assert len(pos) == n and np.abs(pos).max() <= 6
    _, nrm, uv, mat, materials, textures = rq.soup(n, seed)
    return nr.from_oracle(oracle.Scene(rf.triangles(pos, nrm, uv, mat), materials, textures).build_bvh(leaf, 8))


def integer_queries(n, seed):
    """Triangles of non-zero area with integer coordinates in [-6, 6], from one cell to most of the scene."""
    rng = np.random.default_rng(seed)
    reach = rng.choice([1, 1, 2, 4], (2 * n, 1, 1))
    q = np.clip(rng.integers(-5, 6, (2 * n, 1, 3)) + rng.integers(-4, 5, (2 * n, 3, 3)) * reach // 4, -6, 6)
    return q[[not area_is_zero(t) for t in as_tuples(q)]][:n].astype(np.float32)


def missed_by_the_traversal(g, q):
    """(pairs the brute force lists, pairs the traversal lists), after asserting the subset exactly and the counts' consistency."""
    _, totals = tv.overlap(g, q, 0)
    prims, counts = tv.overlap(g, q, totals)
    assert (counts == totals).all()
    _, btotals = tv.brute_force(g, q, 0)
    bprims, _ = tv.brute_force(g, q, btotals)
    mine, brute = tv.pair_sets(prims, totals), tv.pair_sets(bprims, btotals)
    assert mine <= brute                                                        # the cull only ever removes
    assert (tv.overlap(g, q, 0, tv.ANY)[1] == (totals > 0)).all()               # ANY is LIST's count > 0
    return brute, mine, totals


def test_on_small_integers_the_traversal_equals_the_brute_force():
    """Integer coordinates in [-6, 6] and no zero-area triangle on either side: the rule computes in real arithmetic (see above), so
    a listed pair really intersects, its two bounding boxes therefore meet, a node's box holds its triangles' real vertices
    (v0 + e1 is exact), and every ancestor passes the cull: nothing the brute force lists can be missed."""
    g = integer_soup(500, 3)
    q = integer_queries(160, 4)
    brute, mine, totals = missed_by_the_traversal(g, q)
    assert brute == mine
    assert totals.max() >= 20 and (totals == 0).any()


def test_the_list_does_not_depend_on_the_order_in_which_the_leaves_arrive():
    """The builder's trees hand a query its triangles in ascending order, so every insert is an append.  With the children of every
    node exchanged they arrive in descending runs: small capacities meet inserts before stored records and evictions, and every
    slot and count is the same."""
    g = integer_soup(500, 3)
    q = integer_queries(160, 4)
    swapped = g._replace(child1=g.child2, child2=g.child1)
    for caps in (4, 1, np.random.default_rng(1).integers(0, 9, len(q))):
        ev, ev_swapped = {}, {}
        prims, counts = tv.overlap(g, q, caps, events=ev)
        prims2, counts2 = tv.overlap(swapped, q, caps, events=ev_swapped)
        assert (prims == prims2).all() and (counts == counts2).all()
        assert not ev["out_of_order"].any() and not ev["evicted"].any()
        assert ev_swapped["evicted"].sum() >= 5                                 # (that they occur, not how often)
        if not np.isscalar(caps) or caps > 1:                                   # (a list of one slot has no middle)
            assert ev_swapped["out_of_order"].sum() >= 5
        assert (tv.overlap(swapped, q, 0, tv.ANY)[1] == (counts > 0)).all()


def sweep_queries(g, rng, n=300, own=100):
    """About n small random triangles centred on surface_points / tie_points / box_points, of size U^3 * 0.3 * extent, and `own` of
    the scene's own triangles."""
    lo, hi = nr.bounds(g)
    extent = np.float32((hi - lo).max())
    center = np.concatenate([nr.surface_points(g, n // 2, rng), nr.tie_points(g, n // 4, rng), nr.box_points(g, n // 4, rng)]).astype(np.float32)
    m = len(center)
    size = (rng.uniform(0, 1, (m, 1, 1)) ** 3 * 0.3 * extent).astype(np.float32)
    q = (center[:, None, :] + rng.uniform(-1, 1, (m, 3, 3)).astype(np.float32) * size).astype(np.float32)
    mine = tv.scene_triangles(g)[rng.choice(len(g.v0), min(own, len(g.v0)), replace=False)]
    return np.concatenate([q, mine]).astype(np.float32)


@pytest.mark.parametrize("name", ["cornell_box", "soup"])
def test_elsewhere_the_traversal_misses_nothing_of_the_brute_force(name):
    """Random floats: the subset is asserted, and on these inputs the number of pairs the traversal misses is asserted zero.  A miss
    could only be the one-ulp cull case of the header (v0 + e1 rounded outside a node box), or a rounded near miss that the brute
    force lists although the bounds do not meet; DESIGN 5.21 records the figures."""
    if name == "soup":
        g = nr.from_oracle(nr.oracle_soup(3000, 5, 2, 8))
    else:
        g = nr.from_oracle(oracle.Scene.load_glb(scene_path("cornell_box")).build_bvh(20, 8))
    q = sweep_queries(g, np.random.default_rng(11))
    brute, mine, totals = missed_by_the_traversal(g, q)
    print("%s: the brute force lists %d (query, triangle) pairs over %d queries, the traversal misses %d of them, the longest list is %d"
          % (name, len(brute), len(q), len(brute - mine), totals.max()))
    assert len(mine) > 300
    assert len(brute - mine) == 0


def test_self_pairs_of_two_crossing_quads_and_a_tetrahedron():
    """The restatement of Renderer.selfIntersections, on the scenes tests/test_gpu_tri_overlap.py derives by hand."""
    from tests.tri_overlap_scenes import CROSSING_QUADS, CROSSING_PAIRS, TETRAHEDRON
    g = nr.from_triangles(CROSSING_QUADS)
    assert sorted(map(tuple, tv.self_pairs(g, CROSSING_QUADS).tolist())) == CROSSING_PAIRS
    assert len(tv.self_pairs(nr.from_triangles(TETRAHEDRON), TETRAHEDRON)) == 0
