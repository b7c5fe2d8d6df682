"""The sphere-cast rule of include/drt.h as tests/sweep_ref.py restates it (CPU only): hand-derived contacts with each of the seven
features of one triangle, resting contact, seams, degenerate input and the miss record; then, on triangle soups and cornell_box, the
float32 all-triangles answer and three well-conditioned checks against the float64 yardstick."""
import numpy as np
import pytest

import oracle
from tests import nearest_ref as nr
from tests import ray_query_ref as rq
from tests import refit_ref as rf
from tests import sweep_ref as sw
from tests.scenes import scene_path

TRI, QUAD, DOWN = sw.TRI, sw.QUAD, sw.DOWN

HAND = sw.HAND


def assert_miss(res, tmax):
    n = len(res.t)
    assert (res.prim == -1).all() and (res.feature == -1).all()
    assert (res.t.view(np.uint32) == np.broadcast_to(np.float32(tmax), n).view(np.uint32)).all()
    for f in (res.u, res.v, res.point):
        assert (f.view(np.uint32) == 0).all()


def hand(k):
    return np.float32([h[k] for h in HAND])


def test_hand_derived_contacts_with_each_feature_of_one_triangle():
    g = nr.from_triangles(TRI)
    res = sw.sphere_cast(g, hand(0), hand(1), hand(2))
    assert (res.prim == 0).all()
    assert res.t.tolist() == [h[3] for h in HAND] and res.feature.tolist() == [h[4] for h in HAND]
    assert res.u.tolist() == [h[5] for h in HAND] and res.v.tolist() == [h[6] for h in HAND]
    assert res.point.tolist() == [list(map(float, h[7])) for h in HAND]
    assert set(res.feature.tolist()) == set(range(7)) | set(range(8, 15))
    for dtype in (np.float32, np.float64):
        t, prim, feat = sw.brute_force(g, hand(0), hand(1), hand(2), dtype=dtype)
        assert t.dtype == dtype and t.tolist() == [h[3] for h in HAND] and (prim == 0).all() and feat.tolist() == [h[4] for h in HAND]
    # tmin moves the start, not the answer: the first case from tmin = 0.25 (s = (0.25, 0.25, 0.75), tau = 0.5)
    res = sw.sphere_cast(g, hand(0)[:1], hand(1)[:1], 0.25, tmin=0.25)
    assert (res.t.tolist(), res.feature.tolist(), res.u.tolist()) == ([0.75], [0], [0.25])
    # ... and past the contact the sphere starts inside the slab: t = tmin, feature 8
    res = sw.sphere_cast(g, hand(0)[:1], hand(1)[:1], 0.25, tmin=0.875)
    assert (res.t.tolist(), res.feature.tolist()) == ([0.875], [8])
    # direction is used as given: twice the speed, half the time
    res = sw.sphere_cast(g, hand(0)[:7], hand(1)[:7] * np.float32(2), hand(2)[:7])
    assert res.t.tolist() == [h[3] / 2 for h in HAND[:7]] and res.feature.tolist() == [h[4] for h in HAND[:7]]


def test_tmax_is_exclusive_and_misses_carry_it():
    g = nr.from_triangles(TRI)
    o, d = hand(0)[:1], hand(1)[:1]
    assert_miss(sw.sphere_cast(g, o, d, 0.25, tmax=0.75), 0.75)                                   # t < tmax, strictly
    assert sw.sphere_cast(g, o, d, 0.25, tmax=np.nextafter(np.float32(0.75), np.float32(1))).t.tolist() == [0.75]
    assert_miss(sw.sphere_cast(g, o, d, 0.25, tmin=0.5, tmax=0.5), 0.5)                           # an empty range
    assert_miss(sw.sphere_cast(g, np.float32([[2, 2, 1]]), d, 0.25), np.inf)                      # passes beside the triangle
    assert_miss(sw.sphere_cast(g, o, -d, 0.25), np.inf)                                           # moves away
    assert_miss(sw.sphere_cast(g, o, d, 0.25, tmax=np.nan), np.nan)


def test_a_negative_or_nan_radius_a_nan_ray_and_an_empty_scene_miss():
    g = nr.from_triangles(TRI)
    o, d = hand(0)[:1], hand(1)[:1]
    for r in (-0.25, -0.0 - 1e-30, np.nan, -np.inf):
        assert_miss(sw.sphere_cast(g, o, d, r), np.inf)
        assert_miss(sw.sphere_cast(g, o, d, r, tmax=2.0), 2.0)
        assert sw.brute_force(g, o, d, r)[1].tolist() == [-1]
    for k in range(3):
        for arr in (0, 1):
            od = [o.copy(), d.copy()]
            od[arr][0, k] = np.nan
            assert_miss(sw.sphere_cast(g, od[0], od[1], 0.25, tmax=3.0), 3.0)
    assert_miss(sw.sphere_cast(g, o, d, 0.25, tmin=np.nan, tmax=3.0), 3.0)
    empty = nr.from_triangles(np.zeros((0, 3, 3)))
    assert_miss(sw.sphere_cast(empty, hand(0), hand(1), hand(2), tmax=5.0), 5.0)
    assert sw.brute_force(empty, hand(0), hand(1), hand(2), tmax=5.0)[1].tolist() == [-1] * len(HAND)


def test_a_zero_direction_is_the_static_overlap_test():
    g = nr.from_triangles(TRI)
    zero = np.zeros((len(HAND), 3), np.float32)
    res = sw.sphere_cast(g, hand(0), zero, hand(2), tmin=0.5)
    inside = np.array([h[4] >= 8 for h in HAND])
    assert (res.prim == np.where(inside, 0, -1)).all() and (res.feature == np.where(inside, hand(4).astype(np.int32), -1)).all()
    assert (res.t[inside] == 0.5).all() and np.isinf(res.t[~inside]).all()
    assert res.point[inside].tolist() == [list(map(float, h[7])) for h in HAND if h[4] >= 8]
    neg = np.float32([[-0.0, 0.0, -0.0]])
    assert sw.sphere_cast(g, hand(0)[7:8], neg, 0.25).feature.tolist() == [8]


def test_a_zero_area_triangle_has_edges_and_vertices_but_no_face():
    """v0 = v1: e1 = 0.  No face candidate (den = 0) and no edge-1 candidate (ee = 0: the edge is its two vertices); the segment's
    cylinder is edge 2's, which comes before the identical edge 3, and its ends are vertices."""
    sliver = np.float32([[[0, 0, 0], [0, 0, 0], [2, 0, 0]]])
    g = nr.from_triangles(sliver)
    res = sw.sphere_cast(g, np.float32([[1, 0, 1], [-0.1875, -0.25, 1.75], [2.1875, 0.25, 1.75], [1, 0, 0.125]]), np.float32([DOWN] * 4),
                         np.float32([0.25, 0.8125, 0.8125, 0.25]))
    assert res.t.tolist() == [0.75, 1.0, 1.0, 0.0] and res.feature.tolist() == [2, 4, 6, 10]
    assert res.point.tolist() == [[1, 0, 0], [0, 0, 0], [2, 0, 0], [1, 0, 0]] and not np.isnan(res.u).any() and not np.isnan(res.v).any()
    point = np.float32([[[1, 1, 0], [1, 1, 0], [1, 1, 0]]])                                     # all three vertices equal: a point
    res = sw.sphere_cast(nr.from_triangles(point), np.float32([[1, 1, 1], [1.5, 1, 1]]), np.float32([DOWN] * 2), 0.25)
    assert res.t.tolist() == [0.75, np.inf] and res.feature.tolist() == [4, -1]


def test_resting_contact_is_a_hit_at_tmin_for_every_rounding_of_the_gap():
    """Centres at r (1 + j 2^-24) above the face, j = -4 .. 4, pushed into it: tau = 0 by the slab's containment branch or a small
    positive quotient, never a miss."""
    g = nr.from_triangles(TRI * np.float32(4))
    for r in (0.3, 0.25, 1.7, 1e-3):
        for tmin in (0.0, 1.0):
            j = np.arange(-4, 5)
            z = (np.float64(np.float32(r)) * (1 + j * 2.0 ** -24) + tmin).astype(np.float32)
            o = np.stack([np.full(9, 1.1, np.float32), np.full(9, 0.9, np.float32), z], axis=1)
            for d in (DOWN, (0.25, -0.125, -1)):
                res = sw.sphere_cast(g, o, np.float32([d] * 9), r, tmin=tmin)
                assert (res.prim == 0).all() and (res.feature & 7 == 0).all(), (r, tmin, res)
                # the gap itself is up to 4 x 2^-24 r and the start centre is rounded once: four ulp-scale steps bound the sum
                assert (np.abs(res.t - np.float32(tmin)) <= 2.0 ** -21 * max(1.0, r + tmin)).all(), (r, tmin, res.t)
            # moving away from inside the slab is a containment hit; from outside it, a miss
            res = sw.sphere_cast(g, o, np.float32([(0, 0, 1)] * 9), r, tmin=tmin)
            assert ((res.feature == 8) | (res.prim == -1)).all() and (tmin != 0.0 or ((res.feature[:4] == 8).all() and (res.prim[6:] == -1).all()))


@pytest.mark.parametrize("r", [0.05, 1e-3])
def test_nothing_slips_through_a_seam(r):
    g = nr.from_triangles(QUAD)
    xy = sw.seam_casts(r)
    gap = np.hypot(np.maximum(np.maximum(-xy[:, 0], xy[:, 0] - 1), 0), np.maximum(np.maximum(-xy[:, 1], xy[:, 1] - 1), 0))
    keep = gap <= 0.95 * r                                             # the sphere's path meets the quad, not grazing
    xy, gap = xy[keep], gap[keep]
    assert len(xy) > 150
    o = np.concatenate([xy, np.ones((len(xy), 1))], axis=1).astype(np.float32)
    res = sw.sphere_cast(g, o, np.float32([DOWN] * len(o)), r, tmax=2.0)
    assert (res.prim >= 0).all(), "passed through at %r" % (xy[res.prim < 0],)
    x32 = o.astype(np.float64)
    gap = np.hypot(np.maximum(np.maximum(-x32[:, 0], x32[:, 0] - 1), 0), np.maximum(np.maximum(-x32[:, 1], x32[:, 1] - 1), 0))
    want = 1 - np.sqrt(np.float64(np.float32(r)) ** 2 - gap ** 2)
    assert np.abs(res.t - want).max() <= 2e-6
    assert {0, 1, 2, 3, 4, 5, 6} >= set(res.feature.tolist()) and len(set(res.feature.tolist())) >= 3
    # oblique casts aimed at the targets inside the quad cross its plane inside it: a hit before the plane
    ins = gap == 0
    d = np.float32([0.3, -0.2, -1])
    res = sw.sphere_cast(g, (np.concatenate([xy[ins], np.zeros((ins.sum(), 1))], axis=1) - d).astype(np.float32), np.tile(d, (ins.sum(), 1)), r, tmax=2.0)
    assert (res.prim >= 0).all() and (res.t < 1).all() and (res.t > 1 - 2 * r).all()


# ---------------------------------------------------------------- soups and cornell_box against the float64 yardstick

def soup_scene(n, seed, half, spread):
    pos, nrm, uv, mat, materials, textures = rq.soup(n, seed, half, spread)
    return oracle.Scene(rf.triangles(pos, nrm, uv, mat), materials, textures).build_bvh(2, 8)


KINDS = ("aimed", "near", "parallel", "far")


@pytest.fixture(scope="module", params=["soup", "dense_soup", "cornell_box"])
def case(request):
    if request.param == "soup":
        osc = soup_scene(1000, 5, 0.25, 4.0)
        assert oracle.tree_depth(osc.nodes) >= 10
    elif request.param == "dense_soup":
        osc = soup_scene(300, 7, 1.0, 2.0)                 # large triangles that cross each other
    else:
        osc = oracle.Scene.load_glb(scene_path("cornell_box")).build_bvh(20, 8)
    g = nr.from_oracle(osc)
    casts = sw.cast_sets(g, 600, np.random.default_rng(3))
    assert len(casts[0]) == 600
    visits = np.zeros(600, np.int64)
    res = sw.sphere_cast(g, *casts, visits=visits)
    t64, prim64, _ = sw.brute_force(g, *casts, dtype=np.float64)
    return request.param, g, casts, res, visits, (t64, prim64)


def test_tree_answer_is_the_float32_all_triangles_answer(case):
    name, g, casts, res, visits, _ = case
    t, prim, feat = sw.brute_force(g, *casts, dtype=np.float32)
    differs = (res.t.view(np.uint32) != t.view(np.uint32)) | (res.prim != prim) | (res.feature != feat)
    print("%s: %d hits of 600, the tree's answer differs from the float32 all-triangles answer on %d, %.1f of %d nodes visited per cast"
          % (name, (res.prim >= 0).sum(), differs.sum(), visits.mean(), len(g.bmin)))
    # the fp32 slab test of an inflated box is not exactly conservative: such casts are counted, and the float64 checks hold for them
    assert differs.sum() <= 0.01 * 600
    assert 150 < (res.prim >= 0).sum() < 570 and len(set(res.feature.tolist())) >= 9
    if name == "soup":
        assert visits.mean() < 0.25 * len(g.bmin)


def _ends(g, casts, res):
    """Per cast in float64: origin, direction, radius, the checked range [a, b] (a hit: [tmin, t]; a miss: [tmin, tmax] clipped to
    the root box inflated by r, b < a if empty) and M."""
    org, dirs, radius, tmin, tmax = casts
    o, d, r = org.astype(np.float64), dirs.astype(np.float64), radius.astype(np.float64)
    lo, hi = (x.astype(np.float64) for x in nr.bounds(g))
    with np.errstate(all="ignore"):
        t0, t1 = ((lo - r[:, None]) - o) / d, ((hi + r[:, None]) - o) / d
        enter, leave = np.fmin(t0, t1).max(axis=1), np.fmax(t0, t1).min(axis=1)
    hit = res.prim >= 0
    a = tmin.astype(np.float64)
    b = np.where(hit, res.t.astype(np.float64), np.minimum(tmax.astype(np.float64), leave))
    a = np.where(hit, a, np.maximum(a, enter))
    span = np.where((b >= a) & np.isfinite(b), b, a)
    with np.errstate(invalid="ignore"):                # (a miss that never reaches the inflated box has an infinite, empty range)
        M = np.fmax.reduce([np.abs(o + d * a[:, None]).max(axis=1), np.abs(o + d * span[:, None]).max(axis=1), r,
                            np.full(len(o), max(np.abs(lo).max(), np.abs(hi).max()))])
    return o, d, r, a, b, M


# The measured largest figures of the restatement on exactly these inputs (seed 3, 600 casts each), in units of 2^-23 M:
#   contact residual   soup 3.0514, dense_soup 4.2602, cornell_box 9.9843
#   clearance deficit  none: the smallest clearance margin is 54.1 (soup), 75.3 (dense_soup), 77.8 (cornell_box) above r
# B = four times the largest one; the margin covers other seeds.
B_MEASURED = 9.9843
B = 4 * B_MEASURED


def test_contact_residual_is_within_B_ulps(case):
    """1. For every hit that entered (feature < 8) the float64 distance from o + d t to the hit triangle is r."""
    name, g, casts, res, _, _ = case
    o, d, r, a, b, M = _ends(g, casts, res)
    sel = (res.prim >= 0) & (res.feature < 8)
    cc = o[sel] + d[sel] * res.t[sel].astype(np.float64)[:, None]
    err = np.abs(sw.dist_to_triangle(g, cc, res.prim[sel]) - r[sel]) / (2.0 ** -23 * M[sel])
    print("%s: largest contact residual / (2^-23 M) = %.4f over %d entering hits (B = %.4f)" % (name, err.max(), sel.sum(), B))
    assert sel.sum() > 100 and (err <= B).all()


def test_the_path_before_the_contact_is_clear_within_B_ulps(case):
    """2. At 16 evenly spaced parameters of [tmin, t) -- a miss: of [tmin, tmax] clipped to the inflated root box -- the float64 distance
    to the whole mesh is at least r."""
    name, g, casts, res, _, _ = case
    o, d, r, a, b, M = _ends(g, casts, res)
    hit = res.prim >= 0
    sel = np.nonzero(b > a)[0]
    k = np.where(hit[sel, None], np.arange(16)[None] / 16.0, np.arange(16)[None] / 15.0)
    with np.errstate(invalid="ignore"):
        t = np.where(np.isinf(b[sel, None]), a[sel, None], a[sel, None] + (b[sel] - a[sel])[:, None] * k)
    pts = o[sel, None, :] + d[sel, None, :] * t[:, :, None]
    dist = sw.dist_to_mesh(g, pts.reshape(-1, 3)).reshape(len(sel), 16)
    deficit = ((r[sel, None] - dist) / (2.0 ** -23 * M[sel, None])).max(axis=1)
    print("%s: largest clearance deficit / (2^-23 M) = %.4f over %d hits and %d misses (B = %.4f)"
          % (name, deficit.max(), hit[sel].sum(), (~hit[sel]).sum(), B))
    assert hit[sel].sum() > 100 and (~hit[sel]).sum() > 20 and (deficit <= B).all()


def test_hit_or_miss_agrees_with_the_float64_sweep_off_the_grazing_casts(case):
    """3. Wherever the float64 answer is the same at radii r (1 - 2^-12) and r (1 + 2^-12); the casts left out are the grazing ones, at
    most 2 % of each kind of cast, a cap that holds on the yardstick alone."""
    name, g, casts, res, _, (t64, prim64) = case
    org, dirs, radius, tmin, tmax = casts
    less = sw.brute_force(g, org, dirs, (radius.astype(np.float64) * (1 - 2.0 ** -12)), tmin, tmax, dtype=np.float64)[1] >= 0
    more = sw.brute_force(g, org, dirs, (radius.astype(np.float64) * (1 + 2.0 ** -12)), tmin, tmax, dtype=np.float64)[1] >= 0
    stable = (less == more) & (less == (prim64 >= 0))
    for k, kind in enumerate(KINDS):
        part = slice(150 * k, 150 * (k + 1))
        grazing = (~stable[part]).sum()
        print("%s / %s: %d grazing casts of 150, %d hits" % (name, kind, grazing, (prim64[part] >= 0).sum()))
        assert grazing <= 0.02 * 150
    assert ((res.prim >= 0) == (prim64 >= 0))[stable].all()


def test_bounds_and_order_do_not_change_an_answer(case):
    name, g, casts, res, _, _ = case
    org, dirs, radius, tmin, tmax = casts
    hit = res.prim >= 0
    # tmax just past the contact: the same answer; tmax = the contact: a miss by the strict <.  ("Just past" is 2^-12 of t, not one
    # ulp: where a wall lies in a face of its node's box the inflated box is entered at the contact itself, and the fp32 slab test
    # may put that entry an ulp after a tmax that tight -- the header's note on culling.)
    past = np.where(hit, res.t * np.float32(1 + 2.0 ** -12) + np.float32(2.0 ** -20), tmax).astype(np.float32)
    again = sw.sphere_cast(g, org, dirs, radius, tmin, past)
    assert all(x[hit].tobytes() == y[hit].tobytes() for x, y in zip(res, again))
    at = sw.sphere_cast(g, org, dirs, radius, tmin, np.where(hit, res.t, tmax).astype(np.float32))
    assert (at.prim == -1).all()
    perm = np.random.default_rng(1).permutation(600)
    shuffled = sw.sphere_cast(g, org[perm], dirs[perm], radius[perm], tmin[perm], tmax[perm])
    assert all(x[perm].tobytes() == y.tobytes() for x, y in zip(res, shuffled))
