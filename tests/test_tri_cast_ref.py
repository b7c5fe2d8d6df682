"""What the restatement of the triangle cast (tests/tri_cast_ref.py, include/drt.h drt_renderer_triangle_cast) is worth, without a
GPU: hand cases with the deciding candidate and the normal, zero-area and non-finite input, an exact check on small integers against
a ray cast on the convex hull of the nine vertex differences in exact integer arithmetic, the tree against the brute force and against
the same rule in float64, and the working range.  tests/test_gpu_tri_cast.py compares the kernel with this restatement bit for bit."""
from fractions import Fraction
import itertools

import numpy as np
import pytest

import oracle
from tests import nearest_ref as nr
from tests import tri_cast_ref as tc
from tests.scenes import scene_path
from tests.test_tri_overlap_ref import area_is_zero, as_tuples, triangles_meet

NAN, INF = np.float32(np.nan), np.float32(np.inf)
T = np.float32([[[0, 0, 0], [4, 0, 0], [0, 4, 0]]])             # the scene of the hand cases
Q = [(1, 1, 2), (1, 2, 3), (2, 1, 3)]                           # a query above its interior, vertex 0 lowest
PIERCE = [(1, 1, -1), (1, 1, 1), (1.25, 1.125, 1)]              # an edge through the interior
DOWN = (0, 0, -1)

# (query, d, tmax, t, prim, feature, normal, point, (u, v)) against T.  feature = the deciding candidate, | 16 for a start overlap.
HAND_CASES = [
    (Q, DOWN, 4, 2.0, 0, 0, (0, 0, 16), (1, 1, 0), (0.25, 0.25)),                       # a vertex onto the face
    ([(-10, -10, 1), (20, -10, 4), (-10, 20, 4)], DOWN, 4, 3.0, 0, 3, (-90, -90, 900), (0, 0, 0), (0, 0)),   # the face onto the scene's v0
    ([(1, -1, 1), (3, -1, -1), (2, -5, 0)], (0, 1, 0), 4, 1.0, 0, 6, (0, -8, 0), (2, 0, 0), (0.5, 0)),      # crossed edges 0 and 0
    # a vertex onto an edge: candidate 0 (v = 0, closed) and the edge pairs 6 and 12 (s = 0, s = 1) share t = 1; the lowest wins
    ([(2, -1, 1), (1, -3, 2), (3, -3, 2)], (0, 1, -1), 4, 1.0, 0, 0, (0, 0, 16), (2, 0, 0), (0.5, 0)),
    # parallel planes approaching: all three vertices, all three scene vertices and the edge pairs share t = 1
    ([(0, 0, 1), (4, 0, 1), (0, 4, 1)], DOWN, 4, 1.0, 0, 0, (0, 0, 16), (0, 0, 0), (0, 0)),
    ([(0, 4, -1), (4, 0, -1), (0, 0, -1)], (0, 0, 2), 1, 0.5, 0, 0, (0, 0, -16), (0, 4, 0), (0, 1)),        # from below: the normal is flipped
    (Q, (0, 0, 1), 4, 4.0, -1, -1, (0, 0, 0), (0, 0, 0), (0, 0)),                       # motion away: a miss
    (Q, DOWN, 2, 2.0, -1, -1, (0, 0, 0), (0, 0, 0), (0, 0)),                            # contact exactly at tmax: [0, tmax) is half open
    (Q, DOWN, np.float32(2.0000002), 2.0, 0, 0, (0, 0, 16), (1, 1, 0), (0.25, 0.25)),   # ... and one ulp later it is found
    (PIERCE, (0.5, 0, 0), 1, 0.0, 0, 16 | 13, (0, 0, 0), (0, 0, 0), (0, 0)),            # a start overlap by an edge through the interior
    (PIERCE, (0, 0, 0), 1, 0.0, 0, 31, (0, 0, 0), (0, 0, 0), (0, 0)),                   # d = 0, touching: no candidate at all
    (Q, (0, 0, 0), 1, 1.0, -1, -1, (0, 0, 0), (0, 0, 0), (0, 0)),                       # d = 0, apart
    # coplanar sliding: the query's vertex 0 reaches the hypotenuse at t = 0.5, but every det is 0: a miss BY THE STATED LIMITATION
    ([(5, 1, 0), (7, 1, 0), (5, 3, 0)], (-4, 0, 0), 1, 1.0, -1, -1, (0, 0, 0), (0, 0, 0), (0, 0)),
    ([(1, 1, 3), (3, 1, 3), (3, 1, 3)], DOWN, 4, 3.0, 0, 0, (0, 0, 16), (1, 1, 0), (0.25, 0.25)),          # a zero-area query: a segment
    ([(1, 1, 2)] * 3, DOWN, 4, 2.0, 0, 0, (0, 0, 16), (1, 1, 0), (0.25, 0.25)),                            # ... and a point
]


def one(q, d, tmax=1.0, mode=tc.FIRST, scene=T):
    return tc.cast(nr.from_triangles(scene), np.float32(q).reshape(-1, 3, 3), d, tmax, mode)


def test_hand_cases_their_deciding_candidates_and_normals():
    q, d, tmax = np.float32([c[0] for c in HAND_CASES]), np.float32([c[1] for c in HAND_CASES]), np.float32([c[2] for c in HAND_CASES])
    res = one(q, d, tmax)
    assert res.t.tolist() == [c[3] for c in HAND_CASES]
    assert res.prim.tolist() == [c[4] for c in HAND_CASES]
    assert res.feature.tolist() == [c[5] for c in HAND_CASES]
    assert res.normal.tolist() == [list(map(float, c[6])) for c in HAND_CASES]
    assert (res.normal == np.float32([c[6] for c in HAND_CASES])).all() and (nr.dot(res.normal, d) <= 0).all()
    assert (res.point == np.float32([c[7] for c in HAND_CASES])).all()
    assert list(zip(res.u.tolist(), res.v.tolist())) == [tuple(map(float, c[8])) for c in HAND_CASES]
    # point is on the scene triangle at (u, v), and where a query vertex decided it is that vertex moved by d t
    g = nr.from_triangles(T)
    contact = (res.prim >= 0) & (res.feature < 16)
    assert (res.point == (g.v0[0] + g.e1[0] * res.u[:, None]) + g.e2[0] * res.v[:, None])[contact].all()
    assert (q[0, 0] + d[0] * res.t[0] == res.point[0]).all()
    # the ties: which candidates pass with the winning time
    def passing(i):
        return [k for k, (ok, tau, *_) in enumerate(tc.candidates(q[i, 0], q[i, 1], q[i, 2], d[i], g.v0[0], g.e1[0], g.e2[0])) if ok and tau == res.t[i]]
    assert passing(3) == [0, 6, 12]
    assert passing(4) == [0, 1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13]          # (edge i against edge i is parallel: det = 0 for 6, 10, 14)
    # the edge through the interior: every one of the fifteen candidates is absent or positive, the predicate alone says 0
    each = [(bool(ok), float(tau)) for ok, tau, *_ in tc.candidates(q[9, 0], q[9, 1], q[9, 2], d[9], g.v0[0], g.e1[0], g.e2[0])]
    assert len(each) == 15 and all(not ok or tau > 0 for ok, tau in each) and any(ok for ok, _ in each)
    p = tc.pair(q[9, 0], q[9, 1], q[9, 2], d[9], g.v0[0], g.e1[0], g.e2[0])
    assert p.tau == min(tau for ok, tau in each if ok) > 0 and p.t == 0 and p.feature == 16 + 13
    # d = 0: no candidate passes anywhere
    assert not any(ok for i in (10, 11) for ok, *_ in tc.candidates(q[i, 0], q[i, 1], q[i, 2], d[i], g.v0[0], g.e1[0], g.e2[0]))
    # coplanar sliding: no candidate passes although the triangles meet from t = 0.5 on
    assert not any(ok for ok, *_ in tc.candidates(q[12, 0], q[12, 1], q[12, 2], d[12], g.v0[0], g.e1[0], g.e2[0]))
    assert triangles_meet(as_tuples((q[12] + d[12] * np.float32(0.5)).astype(int)[None])[0], as_tuples(T.astype(int))[0])
    # mode ANY on one triangle is the same record, and the brute force agrees
    assert tc.records(one(q, d, tmax, tc.ANY)).tobytes() == tc.records(res).tobytes()
    bt, bp, bf = tc.brute_force(g, q, d, tmax)
    assert (bt == res.t).all() and (bp == res.prim).all() and (bf == res.feature).all()


def test_across_triangles_the_smaller_index_wins_a_tie_and_the_order_of_the_tree_does_not_matter():
    quad = np.float32([[[0, 0, 0], [4, 0, 0], [4, 4, 0]], [[0, 0, 0], [4, 4, 0], [0, 4, 0]]])
    q = np.float32([[(2, 2, 1), (2, 3, 2), (3, 2, 2)]])                      # vertex 0 lands on the diagonal: both triangles at t = 1
    for scene in (quad, quad[::-1]):
        res = one(q, DOWN, 4, scene=scene)
        assert res.t[0] == 1 and res.prim[0] == 0 and res.feature[0] == 0
    # a zero-area scene triangle is its edges and vertices: a segment is hit by an edge pair, a point as a vertex against the query's face
    flat = np.float32([[[0, 0, 0], [4, 0, 0], [4, 0, 0]], [[0, 5, 0]] * 3])
    res = one([[(1, -1, 2), (2, 1, 2), (3, -1, 2)], [(-1, 4, 2), (1, 4, 2), (0, 6, 2)]], DOWN, 4, scene=flat)
    assert res.t.tolist() == [2.0, 2.0] and res.prim.tolist() == [0, 1] and res.feature.tolist() == [6, 3]
    assert res.point[1].tolist() == [0, 5, 0] and res.normal[1].tolist() == [0, 0, 4]
    assert res.point[0].tolist() == [1.5, 0, 0] and (res.u[0], res.v[0]) == (0.375, 0)


def test_non_finite_input_non_positive_tmax_and_the_miss_record():
    q = np.float32([Q] * 10)
    d = np.float32([DOWN] * 10)
    tmax = np.float32([4] * 10)
    q[1, 0, 1], q[2, 2, 2], q[3, 1, 0] = NAN, INF, -INF
    d[4, 2], tmax[5], tmax[6], tmax[7], tmax[8] = NAN, NAN, 0, -1, INF
    d[9, 0] = INF
    for mode in (tc.FIRST, tc.ANY):
        rec = tc.records(one(q, d, tmax, mode))
        i = rec.view(np.int32)
        assert rec[0, 3] == 2 and i[0, 7] == 0 and rec[8, 3] == 2 and i[8, 7] == 0 and rec[8].tobytes() == rec[0].tobytes()
        miss = [1, 2, 3, 4, 5, 6, 7, 9]
        assert (i[miss, 7] == -1).all() and (i[miss, 10] == -1).all() and not rec[miss][:, [0, 1, 2, 4, 5, 6, 8, 9, 11]].any()
        assert rec[[1, 2, 3, 4, 9], 3].tolist() == [4] * 5 and np.isnan(rec[5, 3]) and rec[6, 3] == 0 and rec[7, 3] == -1     # t = tmax
    # tmax <= 0 finds nothing, not even a start overlap
    assert one([PIERCE] * 2, (0.5, 0, 0), np.float32([0, -2])).prim.tolist() == [-1, -1]
    # an empty scene and an empty batch
    none = tc.cast(nr.from_triangles(np.zeros((0, 3, 3))), q, d, 3.0)
    assert (none.prim == -1).all() and (none.t == 3).all() and (none.feature == -1).all() and not none.point.any()
    assert len(tc.cast(nr.from_triangles(T), np.zeros((0, 3, 3), np.float32), DOWN).t) == 0
    # overflow does not raise: the products are infinities and NaNs, and a NaN fails every test
    big = one(np.float32([[(1e30, 1e30, 1e30), (1e30, 2e30, 3e30), (5e30, 5e30, 3e30)]]), (0, 0, -3e38), INF)
    assert big.prim[0] == -1 and np.isinf(big.t[0])


# ---- the exact contact interval of two integer triangles under a translation, by another route than the rule's: the query at
# q + d tau touches the scene triangle iff tau d lies in the Minkowski difference T - Q, the convex hull of the nine differences
# pj - qi.  Its supporting planes are found by brute force over all 84 point triples in int64; the ray tau d is clipped against them in
# fractions.Fraction.
TRIPLES = np.array(list(itertools.combinations(range(9), 3)))


def hull_intervals(A, B, D):
    """Per pair: None if the nine differences are coplanar, else (enter, exit) of the line tau d in the hull as Fractions (enter > exit:
    not reached; +-inf as None ends)."""
    P = (B[:, None, :, :] - A[:, :, None, :]).reshape(len(A), 9, 3).astype(np.int64)
    a = P[:, TRIPLES[:, 0]]
    n = np.cross(P[:, TRIPLES[:, 1]] - a, P[:, TRIPLES[:, 2]] - a)                      # [N, 84, 3]
    s = np.einsum("ntk,ntpk->ntp", n, P[:, None, :, :] - a[:, :, None, :])             # the nine points against each plane
    below, above = (s <= 0).all(axis=2), (s >= 0).all(axis=2)
    nonzero = (n != 0).any(axis=2)
    face = nonzero & (below ^ above)                                                    # a plane through three points with all nine on one side
    flat = ~face.any(axis=1)                                                            # coplanar differences have no such plane
    sign = np.where(below, 1, -1)                                                       # outward normals: every point has n . (x - a) <= 0
    n, c = n * sign[:, :, None], np.einsum("ntk,ntk->nt", n, a) * sign
    nd = np.einsum("ntk,nk->nt", n, D.astype(np.int64))
    out = []
    for i in range(len(A)):
        if flat[i]:
            out.append(None)
            continue
        enter, exit_, reached = None, None, True
        for k in np.nonzero(face[i])[0]:
            nk, ck = int(nd[i, k]), int(c[i, k])
            if nk == 0:
                reached &= ck >= 0                                                      # parallel: inside iff 0 <= c
            elif nk > 0:
                exit_ = Fraction(ck, nk) if exit_ is None else min(exit_, Fraction(ck, nk))
            else:
                enter = Fraction(ck, nk) if enter is None else max(enter, Fraction(ck, nk))
        out.append((enter, exit_) if reached else (Fraction(1), Fraction(0)))
    return out


def nearest_float32(x):
    """The correctly rounded float32 of a Fraction."""
    f = np.float32(float(x))
    return min((f, np.nextafter(f, -INF), np.nextafter(f, INF)), key=lambda c: abs(Fraction(float(c)) - x))


@pytest.mark.parametrize("span, n, skip_cap", [(2, 1700, 0.02), (4, 1600, 0.005)])
def test_on_small_integers_the_pair_rule_is_the_exact_ray_cast_on_the_minkowski_difference(span, n, skip_cap):
    rng = np.random.default_rng(50 + span)
    A, B, D = rng.integers(-span, span + 1, (n, 3, 3)), rng.integers(-span, span + 1, (n, 3, 3)), rng.integers(-span, span + 1, (n, 3))
    for X in (A, B):                                                           # redrawn until neither triangle has zero area
        while True:
            bad = np.array([area_is_zero(t) for t in as_tuples(X)])
            if not bad.any():
                break
            X[bad] = rng.integers(-span, span + 1, (int(bad.sum()), 3, 3))
    B[::2] += rng.integers(-2, 3, (len(B[::2]), 1, 3)) * span                 # half of them further apart: fewer pairs that meet
    aim = np.rint(B.mean(axis=1) - A.mean(axis=1)).astype(np.int64)           # ... and a third of all aimed at the other triangle
    D[::3] = np.clip(aim, -span, span)[::3]
    tmax = rng.choice(np.float32([0.25, 0.5, 1, 2, 4, INF]), n)
    a32, b32 = A.astype(np.float32), B.astype(np.float32)
    p = tc.pair(a32[:, 0], a32[:, 1], a32[:, 2], D.astype(np.float32), b32[:, 0], b32[:, 1] - b32[:, 0], b32[:, 2] - b32[:, 0])
    hit = p.t < tmax                                                           # the pair against best = tmax
    skipped = starts = through = grazes = grazes_found = misses = 0
    for i, (a, b, iv) in enumerate(zip(as_tuples(A), as_tuples(B), hull_intervals(A, B, D))):
        if iv is None:
            skipped += 1
            continue
        enter, exit_ = iv
        t, feature, what = float(p.t[i]), int(p.feature[i]), (a, b, D[i].tolist(), float(tmax[i]), iv, float(p.t[i]), int(p.feature[i]))
        meet = triangles_meet(a, b)
        inside = (enter is None or enter <= 0) and (exit_ is None or exit_ >= 0)
        assert meet == inside, what                                            # the two exact routes agree on the start
        assert ((t == 0) and feature >= 16) == meet and (feature >= 16) == meet, what
        if meet:
            starts += 1
            continue
        # the origin is outside a bounded hull: the line enters it at a finite tau or not at all
        reached = enter is not None and exit_ is not None and enter <= exit_ and enter > 0 and (np.isinf(tmax[i]) or enter < Fraction(float(tmax[i])))
        if not reached:
            misses += 1
            assert not hit[i], what                                            # no false hit
        elif enter < exit_:
            through += 1
            assert hit[i] and p.t[i] == nearest_float32(enter), what           # the correctly rounded exact entry time
        else:
            grazes += 1
            grazes_found += bool(hit[i])
            assert not hit[i] or p.t[i] == nearest_float32(enter), what        # a grazing contact, if reported, has that time
    print("[-%d, %d]: %d pairs, %d skipped (coplanar differences), %d meet at the start, %d pass through the hull, %d graze it (%d found), "
          "%d miss" % (span, span, n, skipped, starts, through, grazes, grazes_found, misses))
    assert n - skipped >= 1500 and skipped <= skip_cap * n
    assert min(starts, through, misses) > n // 20 and grazes > 0


# ---- the tree against the brute force and the float64 yardstick
# B of the accuracy bound |t - t_float64| <= B * 2^-23 * M / |d|, M the largest absolute coordinate of query and scene: four times the
# largest ratio measured with the float64 yardstick on the two scenes below (DESIGN 5.28 has both numbers), as 5.27 does.
MEASURED_RATIO = {"soup": 1.91, "cornell_box": 0.50}
B = 4 * max(MEASURED_RATIO.values())
MISMATCH_CAP = 0.005
LEFT_OUT_CAP = 0.01
_scenes = {}


def scene(name):
    if name not in _scenes:
        osc = nr.oracle_soup(3000, 5, 2, 8) if name == "soup" else oracle.Scene.load_glb(scene_path(name)).build_bvh(20, 8)
        _scenes[name] = nr.from_oracle(osc)
    return _scenes[name]


@pytest.mark.parametrize("name, seed, n", [("soup", 1, 300), ("cornell_box", 2, 300)])
def test_the_tree_equals_the_brute_force_and_stays_within_the_accuracy_bound(name, seed, n):
    g = scene(name)
    q, d = tc.cast_sets(g, n, np.random.default_rng(seed))
    visits, tests = np.zeros(len(q), np.int64), np.zeros(len(q), np.int64)
    tree = tc.cast(g, q, d, 1.0, visits=visits, tests=tests)
    brute, brute_prim, brute_feature = tc.brute_force(g, q, d, 1.0)
    exact, exact_prim, _ = tc.brute_force(g, q, d, 1.0, dtype=np.float64)
    differ = (tree.t != brute) | (tree.prim != brute_prim)
    # the accuracy: float32 against the same rule in float64 over all triangles, wherever both name the same triangle
    same = (brute_prim == exact_prim) & (brute_prim >= 0)
    left_out = (brute_prim != exact_prim).sum()
    M = tc.scale_of(g, q)
    ratio = np.abs(brute.astype(np.float64) - exact)[same] / (2.0 ** -23 * M[same] / np.linalg.norm(d.astype(np.float64), axis=1)[same])
    print("%s: %d casts, %d hit, %d start in overlap, %d differ from the brute force; %.1f nodes (max %d) and %.1f pairs per cast; "
          "%d compared with float64, largest ratio %.4f, %d left out" %
          (name, len(q), (tree.prim >= 0).sum(), (tree.feature >= 16).sum(), differ.sum(), visits.mean(), visits.max(), tests.mean(), same.sum(), ratio.max(), left_out))
    assert (tree.t >= brute).all()                                            # the tree tests a subset of the pairs
    assert differ.mean() <= MISMATCH_CAP
    assert (tree.prim >= 0).sum() > n // 4 and (tree.prim < 0).sum() > n // 10 and same.sum() > n // 4
    assert left_out <= LEFT_OUT_CAP * len(q)
    assert (ratio <= B).all()
    assert ratio.max() <= MEASURED_RATIO[name] <= 1.05 * ratio.max() + 0.01   # the figure in DESIGN 5.28 is this one
    # a shorter tmax: the same answers below it, the miss record at and beyond
    half = tc.cast(g, q, d, 0.5)
    inside = tree.t < 0.5
    assert tc.records(half)[inside].tobytes() == tc.records(tree)[inside].tobytes()
    assert (half.prim[~inside] == -1).all() and (half.t[~inside] == 0.5).all() and inside.any() and (~inside).any()
    # mode ANY: the boolean is the same, the record is a pair before tmax and is the first one the traversal meets
    first = tc.cast(g, q, d, 1.0, tc.ANY)
    assert ((first.prim >= 0) == (tree.prim >= 0)).all() and (first.t >= tree.t).all()
    assert (first.prim != tree.prim).any()


# ---- the working range (include/drt.h "working range of the mesh queries")
SCALE_RANGE = (-42, 36)             # exponents of two between which every answer is the plain answer scaled, in steps of 2^2


def test_working_range_scaling_by_powers_of_two():
    """A mesh with edges of 2^-2 to 2^4 and queries up to 2^7 from it, as the header's paragraph describes the other queries' mesh; the
    directions are scaled with the mesh, so t stays and every det is a third power of the scale."""
    rng = np.random.default_rng(6)
    n = 60
    size = np.float32(2.0) ** rng.integers(-2, 5, (n, 1, 1)).astype(np.float32)
    mesh = (rng.uniform(-40, 40, (n, 1, 3)) + rng.uniform(-1, 1, (n, 3, 3)) * size).astype(np.float32)
    qsize = np.float32(2.0) ** rng.integers(-2, 5, (n, 1, 1)).astype(np.float32)
    q = (rng.uniform(-128, 128, (n, 1, 3)) + rng.uniform(-1, 1, (n, 3, 3)) * qsize).astype(np.float32)
    q[12:18] = mesh[12:18]                                                    # some that touch at the start
    d = ((mesh.mean(axis=1) - q.mean(axis=1)) * rng.uniform(1.2, 3, (n, 1))).astype(np.float32)    # towards a triangle each
    d[::7] *= np.float32(-1)                                                  # ... and away from it
    base = tc.cast(nr.from_triangles(mesh), q, d, 1.0)
    assert (base.prim >= 0).sum() > n // 2 and (base.prim < 0).any() and (base.feature >= 16).any() and (base.t > 0).any()

    def unchanged(e):
        s = np.float32(2.0) ** np.float32(e)
        r = tc.cast(nr.from_triangles(mesh * s), q * s, d * s, 1.0)
        return ((r.prim == base.prim).all() and (r.feature == base.feature).all() and (r.u == base.u).all() and (r.v == base.v).all() and
                (r.t == base.t).all() and (r.point == base.point * s).all() and (r.normal == base.normal * s * s).all())

    ok = {e: unchanged(e) for e in range(-60, 62, 2)}
    lo = min(e for e in ok if all(ok[x] for x in ok if e <= x <= 0))
    hi = max(e for e in ok if all(ok[x] for x in ok if 0 <= x <= e))
    print("unchanged for 2^%d to 2^%d" % (lo, hi))
    assert (lo, hi) == SCALE_RANGE
    assert not ok[lo - 2] and not ok[hi + 2]
