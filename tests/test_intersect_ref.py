"""The rule of the triangle intersection segments (include/drt.h drt_renderer_intersect_triangles) on its restatement alone
(tests/intersect_ref.py; CPU only): the hand cases of two crossing quads, endpoints on shared edges bit-equal from both neighbours,
the set of pairs with a record against the overlap predicate, the endpoints against both triangles in float64, what lists nothing,
the exchange of roles, the traversal against the brute force, and the range of scales the header states."""
import numpy as np

from tests import hostile_meshes as hm
from tests import intersect_ref as ix
from tests import nearest_ref as nr
from tests import tri_overlap_ref as tv
from tests.test_tri_overlap_ref import sweep_queries
from tests.tri_overlap_scenes import CROSSING_QUADS, TETRAHEDRON

NAN, INF = np.float32(np.nan), np.float32(np.inf)


def rule(q, t):
    """segment() on query triangles q [N, 3, 3] against triangles t [N, 3, 3] stored as (v0, v1 - v0, v2 - v0), pair by pair."""
    q, t = np.float32(q), np.float32(t)
    return ix.segment(q[:, 0], q[:, 1], q[:, 2], t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])


def fields(rec):
    return rec[:, 0:3], rec[:, 4:7], rec.view(np.int32)[:, 3], rec.view(np.int32)[:, 7]


def test_the_crossing_quads_by_hand():
    """Queries A0, A1 (z = 0) against a scene of B0, B1 (x = 1).  nq = (0, 0, 16), nt = (4, 0, 0), D = (0, 64, 0): axis y, and the
    segments run towards +y.  Integer coordinates and t in {1/2, 3/4} make every operation exact.
    A0-B0: B0's apex is w2 = (1, 1, 1): T1 = cut(2, 0) = (1, 0, 0) on edge 2, T2 = cut(2, 1) = (1, 1, 0) on edge 1.  A0's apex is q0:
    Q1 = (1, -2, 0) on edge 0, Q2 = (1, 1, 0) on edge 2.  lo = T1 (0 > -2 fails), hi = T2 (a tie: the scene's): (1,0,0) -> (1,1,0),
    code 2 + 16 * 1.
    A0-B1: B1's apex is w0 = (1, -1, -1): T1 = cut(0, 1) = (1, 0, 0) on edge 0, T2 = cut(0, 2) = (1, -1, 0) on edge 2:
    (1,-1,0) -> (1,0,0), code 2 + 16 * 0.
    A1-B0: A1's apex is q1: Q1 = cut(1, 2) = (1, 2, 0) on edge 1, Q2 = cut(1, 0) = (1, 1, 0) on edge 0; lo = Q2 (1 > 0), hi = T2 =
    (1, 1, 0): a zero-length segment, code 4 + 16 * 1.
    A1-B1: B1's interval is y in [-1, 0], A1's is [1, 2]: lo = (1, 1, 0), hi = (1, 0, 0), 1 <= 0 fails: no record."""
    g = nr.from_triangles(CROSSING_QUADS[2:])
    splits, rec = ix.whole(g, CROSSING_QUADS[:2])
    p, q, prim, code = fields(rec)
    assert splits.tolist() == [0, 2, 3]
    assert prim.tolist() == [0, 1, 0] and code.tolist() == [2 + 16 * 1, 2 + 16 * 0, 4 + 16 * 1]
    assert p.tolist() == [[1, 0, 0], [1, -1, 0], [1, 1, 0]] and q.tolist() == [[1, 1, 0], [1, 0, 0], [1, 1, 0]]
    brute, counts = ix.brute_force(g, CROSSING_QUADS[:2], 2)
    assert counts.tolist() == [2, 1] and ix.is_miss(brute[3]).all() and brute[:3].tobytes() == rec.tobytes()
    # truncation keeps the first records; the miss record is all zeros with prim = -1
    one, counts = ix.intersect(g, CROSSING_QUADS[:2], 1)
    assert counts.tolist() == [2, 1] and one.tobytes() == rec[[0, 2]].tobytes()
    assert ix.MISS.view(np.int32).tolist() == [0, 0, 0, -1, 0, 0, 0, 0]


def _edge_points(rec, owner, tris, low):
    """{(owner, undirected edge of tris as a pair of vertex bit patterns): [endpoint bit patterns]} over the endpoints of the records
    whose code digit is in low .. low + 2: the edges of `tris[which]`, which = prim for the scene's edges (low = 0) and the query's
    index for the query's (low = 4).  `owner` is the other side of the pair."""
    p, q, prim, code = fields(rec)
    found = {}
    for pt, digit in ((p, code & 15), (q, code >> 4)):
        for r in np.nonzero((digit >= low) & (digit < low + 3))[0]:
            which = prim[r] if low == 0 else owner[r]
            other = owner[r] if low == 0 else prim[r]
            e = int(digit[r]) - low
            a, b = tris[which][e].tobytes(), tris[which][(e + 1) % 3].tobytes()
            found.setdefault((int(other), min(a, b), max(a, b)), []).append(pt[r].tobytes())
    return found


def test_an_endpoint_on_a_shared_edge_is_the_same_bits_from_both_neighbours():
    """The tetrahedron's six edges each lie in two faces.  Wherever a record ends on a scene edge, the adjacent face has a record of
    the same query that ends on that edge too, with bit-equal coordinates: s of a shared vertex depends on that vertex and the query
    alone, and the cut runs from the below vertex to the above one in both faces.  The same with the roles exchanged, for the query's
    edges: u of a shared vertex depends on that vertex and the scene triangle alone."""
    tris = np.random.default_rng(7).uniform(-1, 5, (300, 3, 3)).astype(np.float32)
    g = nr.from_triangles(TETRAHEDRON)
    assert (tv.scene_triangles(g) == TETRAHEDRON).all()                         # (integer coordinates: v0 + e1 is v1)
    splits, rec = ix.whole(g, tris)
    owner = np.repeat(np.arange(len(tris)), np.diff(splits))
    found = _edge_points(rec, owner, TETRAHEDRON, 0)
    print("scene edges: %d (query, edge) groups" % len(found))
    assert len(found) >= 100
    assert all(len(v) == 2 and v[0] == v[1] for v in found.values())
    # the roles exchanged: the tetrahedron's faces are the queries, the 300 triangles the scene (one leaf: tree order is load order)
    g = nr.from_triangles(tris)
    splits, rec = ix.whole(g, TETRAHEDRON)
    owner = np.repeat(np.arange(4), np.diff(splits))
    found = _edge_points(rec, owner, TETRAHEDRON, 4)
    print("query edges: %d (scene triangle, edge) groups" % len(found))
    assert len(found) >= 100
    assert all(len(v) == 2 and v[0] == v[1] for v in found.values())


def _random_pairs():
    t = np.random.default_rng(1).uniform(-1, 1, (20000, 2, 3, 3)).astype(np.float32)
    return t[:, 0], t[:, 1]


def test_the_pairs_with_a_record_are_the_pairs_the_overlap_predicate_lists():
    """20 000 pairs of random triangles in [-1, 1]^3: none is coplanar or of zero area, so in real arithmetic a record exists iff the
    closed triangles meet, which is what the seventeen axes decide.  In fp32 the two sets could differ for pairs within rounding of
    touching; on these pairs they do not."""
    q, t = _random_pairs()
    has = rule(q, t)[0]
    listed = tv.triangle_listed(q[:, 0], q[:, 1], q[:, 2], t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    print("%d pairs with a record, %d listed by the predicate, %d differ" % (has.sum(), listed.sum(), (has != listed).sum()))
    assert has.sum() > 5000 and (has == listed).all()


def _distance64(x, v):
    """float64 distance of points x [N, 3] from triangles v [N, 3, 3]: the plane where the projection is inside, else the edges."""
    a, b, c = v[:, 0], v[:, 1], v[:, 2]
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(axis=1)
    d = ((x - a) * n).sum(axis=1) / nn
    proj = x - d[:, None] * n
    inside = np.ones(len(x), bool)
    for u, w in ((a, b), (b, c), (c, a)):
        inside &= (np.cross(w - u, proj - u) * n).sum(axis=1) >= 0
    best = np.where(inside, np.abs(d) * np.sqrt(nn), np.inf)
    for u, w in ((a, b), (b, c), (c, a)):
        e = w - u
        s = np.clip(((x - u) * e).sum(axis=1) / (e * e).sum(axis=1), 0, 1)
        best = np.minimum(best, np.linalg.norm(x - (u + s[:, None] * e), axis=1))
    return best


def test_every_endpoint_lies_near_both_triangles_in_float64():
    """On the 5 510 records of the random pairs the worst float64 distance of an endpoint from either triangle of its pair is
    5.82e-7 with this restatement (coordinates of magnitude up to 1, so about five units of 2^-23: the cut points divide by
    s_lo - s_hi, which cancels for a vertex near the other plane).  The bound is four times that, 2.328e-6: the factor covers another
    libm or another summation order in this float64 check, not the rule."""
    q, t = _random_pairs()
    has, p, e, _ = rule(q, t)
    q64, t64 = q[has].astype(np.float64), t[has].astype(np.float64)
    worst = max(_distance64(x[has].astype(np.float64), v).max() for x in (p, e) for v in (q64, t64))
    print("worst distance of an endpoint from a triangle of its pair: %.3e over %d records" % (worst, has.sum()))
    assert worst <= 4 * 5.82e-7


def test_coplanar_zero_area_and_invalid_queries_list_nothing():
    T = np.float32([[0, 0, 0], [4, 0, 0], [0, 4, 0]])
    g = nr.from_triangles(T[None])
    good = np.float32([[(1, 1, -1), (1, 1, 1), (5, 5, 0)]])
    rec, counts = ix.intersect(g, good, 1)
    assert counts.tolist() == [1] and ix.brute_force(g, good, 1)[0].tobytes() == rec.tobytes()
    nothing = [[(1, 1, 0), (2, 1, 0), (1, 2, 0)], [(0, 0, 0), (4, 0, 0), (0, 4, 0)], [(3, 3, 0), (5, 3, 0), (3, 5, 0)],   # coplanar: inside, itself, apart
               [(0, 0, 1), (4, 0, 1), (0, 4, 1)],                                                                          # parallel
               [(1, 1, -2), (1, 1, 2), (1, 1, 2)], [(1, 1, 0)] * 3, [(1, 1, -1)] * 3,                                      # a segment through it, points
               [(1, 1, -1), (1, NAN, 1), (5, 5, 0)], [(1, 1, -1), (1, 1, 1), (INF, 5, 0)], [(-INF, 1, -1), (1, 1, 1), (5, 5, 0)]]
    q = np.float32(nothing)
    assert tv.overlap(g, q, 0)[1][[0, 1, 4, 5]].all()                          # the predicate lists these: the rule here is stricter
    for run in (ix.intersect, ix.brute_force):
        rec, counts = run(g, q, 2)
        assert not counts.any() and ix.is_miss(rec).all() and len(rec) == 2 * len(q)
    # a zero-area triangle in the scene
    for flat in ([[1, 1, -1], [1, 1, 1], [1, 1, 1]], [[1, 1, 0]] * 3):
        assert not ix.intersect(nr.from_triangles(np.float32([flat])), np.float32([T]), 1)[1].any()
    # every word of a valid query made non-finite in turn
    for word in range(9):
        for value in (NAN, INF, -INF):
            bad = tv.pack(good)
            bad[0, word] = value
            assert ix.intersect(g, bad, 0)[1].tolist() == [0] and ix.brute_force(g, bad, 0)[1].tolist() == [0]
    # valid, and every product overflows: a NaN fails the last comparison
    assert ix.intersect(g, good * np.float32(1e30), 0)[1].tolist() == [0]
    # an empty scene and no queries
    rec, counts = ix.intersect(nr.from_triangles(np.zeros((0, 3, 3))), good, 3)
    assert ix.is_miss(rec).all() and len(rec) == 3 and counts.tolist() == [0]
    rec, counts = ix.intersect(g, np.zeros((0, 3, 3), np.float32), 2)
    assert rec.shape == (0, 8) and len(counts) == 0 and counts.dtype == np.uint32


def test_exchanging_the_roles_of_a_pair_gives_the_same_points_with_p_and_q_exchanged():
    """Coordinates on a grid of 1/16 in [-4, 4], so v0 + (v1 - v0) is v1 and both roles see the same world vertices.  nq and nt
    change places, D changes its sign and keeps its axis, T and Q change places: the same four cut points, the same two chosen --
    except on a tie, where the scene's point is kept and the two roles may keep different ones (no pair here ties).  The codes
    exchange their digits, and an edge of the scene becomes 4 + that edge of the query."""
    rng = np.random.default_rng(3)
    a, b = (rng.integers(-64, 65, (4000, 3, 3)) / 16).astype(np.float32), (rng.integers(-64, 65, (4000, 3, 3)) / 16).astype(np.float32)
    h1, p1, q1, c1 = rule(a, b)
    h2, p2, q2, c2 = rule(b, a)
    assert (h1 == h2).all() and h1.sum() > 300
    assert p1[h1].tobytes() == q2[h1].tobytes() and q1[h1].tobytes() == p2[h1].tobytes()
    flip = lambda d: np.where(d >= 4, d - 4, d + 4)
    assert (flip(c1[h1] & 15) == c2[h1] >> 4).all() and (flip(c1[h1] >> 4) == (c2[h1] & 15)).all()


def test_on_the_soup_the_traversal_equals_the_brute_force():
    """The cull only ever removes, and on these inputs it removes nothing: every record, slot by slot."""
    g = nr.from_oracle(nr.oracle_soup(3000, 5, 2, 8))
    q = sweep_queries(g, np.random.default_rng(11))
    _, totals = ix.intersect(g, q, 0)
    rec, _ = ix.intersect(g, q, totals)
    _, btotals = ix.brute_force(g, q, 0)
    brec, _ = ix.brute_force(g, q, btotals)
    print("%d records over %d queries, the longest list is %d" % (len(rec), len(q), totals.max()))
    assert len(rec) > 300 and (totals == btotals).all() and rec.tobytes() == brec.tobytes()
    prim = fields(rec)[2]
    owner = np.repeat(np.arange(len(q)), totals.astype(np.int64))
    assert (np.diff(prim)[np.diff(owner) == 0] > 0).all()                       # ascending triangle index, at most one record per pair
    # a smaller capacity is the prefix, with the miss record behind a shorter list
    caps = np.minimum(totals, 2).astype(np.int64) + (np.arange(len(q)) % 2)
    part, counts = ix.intersect(g, q, caps)
    assert (counts == totals).all()
    base, start = np.concatenate([[0], np.cumsum(caps)]), np.concatenate([[0], np.cumsum(totals.astype(np.int64))])
    for i in range(len(q)):
        k = min(int(caps[i]), int(totals[i]))
        assert part[base[i]:base[i] + k].tobytes() == rec[start[i]:start[i] + k].tobytes()
        assert ix.is_miss(part[base[i] + k:base[i + 1]]).all()


# The range of k, in steps of 2, over which the degenerate mesh of tests/hostile_meshes.py scaled by 2^k, with its triangle queries
# scaled as well, gives the plain records scaled (p and q times 2^k, prim, code and every count the same): what the "Scale" paragraph
# of the header block states.  D = cross(nq, nt) is a fourth power of the lengths, as the overlap predicate's axes are.
SCALE_RANGE = (-24, 32)


def test_the_range_of_scales_in_which_no_record_changes():
    mesh = hm.degenerate()
    osc = hm.oracle_scene(mesh)
    g = nr.from_oracle(osc)
    kind, twin = hm.kinds_in_tree_order(osc, mesh)
    tris = hm.queries(g, osc, kind, twin, 11, general=100).tris
    splits, rec = ix.whole(g, tris)
    assert len(rec) > 100

    def same_at(k):
        s = np.float32(2.0 ** k)
        with np.errstate(all="ignore"):
            gk = nr.from_oracle(hm.oracle_scene(hm.scaled(mesh, k)))
            sk, rk = ix.whole(gk, tris * s)
            want = rec.copy()
            want[:, 0:3] *= s
            want[:, 4:7] *= s
        return (sk == splits).all() and rk.tobytes() == want.tobytes()

    ends = []
    for step in (-2, 2):
        k = 0
        while abs(k) < 60 and same_at(k + step):
            k += step
        ends.append(k)
    print("scaling by 2^k changes no record for k in [%d, %d]" % tuple(ends))
    assert tuple(ends) == SCALE_RANGE
