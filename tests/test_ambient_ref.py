"""What the restatement of drt_renderer_ambient_occlusion (tests/ambient_ref.py) is worth, without a GPU: statistical hand cases whose
answers follow from the geometry, and exact cases of the rule's edges.  tests/test_gpu_ambient.py holds the kernel to the restatement
bit for bit."""
import numpy as np
import pytest

import oracle
from tests import ambient_ref as ar
from tests import ray_query_ref as rq
from tests.scenes import scene_path

drt = pytest.importorskip("dustraytracer_amd")

F = np.float32
S = 4096
SEEDS = (1, 7, 2024)
UP = F([[0, 0, 1]])
ORIGIN = F([[0, 0, 0]])
INF = F(np.inf)


@pytest.fixture(scope="module")
def wall():
    # the plane x = 0.01, 10^4 to either side and upwards: from o = (0, 0, 0.001) a direction is blocked exactly when d.x > 0.  (It
    # starts at z = -1, not -10^4: the diagonal its two triangles share then passes 5000 above the point and not through its foot, where
    # the triangle test, in fp32 on edges of 10^4, lets three of the 12288 directions through between the two.)
    return ar.flat_scene(drt, ar.rect((0.01, -1e4, -1), (0, 2e4, 0), (0, 0, 1e4 + 1)))[1]


@pytest.fixture(scope="module")
def lone_quad():
    return ar.flat_scene(drt, ar.quad(-1, 1, -1, 1, 0))[1]


@pytest.fixture(scope="module")
def room():
    # a closed box [-1, 1]^2 x [0, 2]; the query point is the middle of its floor
    return ar.flat_scene(drt, ar.box((-1, -1, 0), (1, 1, 2)))[1]


# ---------------------------------------------------------------- statistical hand cases: S = 4096, first = 0, point 0
# The rule is deterministic, so these are fixed counts; the bounds are five binomial standard deviations.

@pytest.mark.parametrize("seed,positive_x", list(zip(SEEDS, (2039, 2090, 2031))))
def test_a_wall_at_the_foot_blocks_half_the_hemisphere(wall, seed, positive_x):
    _, d, tries = ar.rays(ORIGIN, UP, 0.001, S, seed)
    # the counts the restatement gives: d.x > 0 on 2039, 2090 and 2031 of 4096 directions for seeds 1, 7 and 2024 (2048 expected, five
    # standard deviations = 160), no direction with d.z <= 0, the longest rejection run 25
    assert int((d[0, :, 0] > 0).sum()) == positive_x and abs(positive_x - 2048) <= 160
    assert (d[0, :, 2] > 0).all()
    assert 1 <= tries.max() <= 25
    rec = ar.ambient(wall, ORIGIN, UP, INF, 0.001, S, seed)[0]
    print("seed %d: d.x > 0 on %d, open %d, longest rejection run %d" % (seed, positive_x, rec[0], tries.max()))
    assert rec[0] == S - positive_x                                            # open: 2057, 2006, 2065
    assert abs(int(rec[0]) - 2048) <= 160
    assert rec[1] < 0                                                          # the bent normal leans away from the wall


@pytest.mark.parametrize("seed", SEEDS)
def test_a_lone_quad_sees_the_whole_sky_and_the_bent_normal_is_two_thirds_up(lone_quad, seed):
    rec = ar.ambient(lone_quad, ORIGIN, UP, INF, 0.001, S, seed)[0]
    assert rec[0] == S
    bent = rec[1:4].astype(np.float64) / (S * 65536.0)
    # measured: (-0.0027, 0.0064, 0.6670), (0.0051, 0.0080, 0.6729), (-0.0124, 0.0009, 0.6727) for seeds 1, 7 and 2024, against the
    # cosine-weighted mean (0, 0, 2/3); five standard deviations of the mean are 0.039 for x and y and 0.018 for z
    print("seed %d: bent / (S 65536) = (%.4f, %.4f, %.4f)" % ((seed,) + tuple(bent)))
    assert abs(bent[0]) <= 0.039 and abs(bent[1]) <= 0.039 and abs(bent[2] - 2.0 / 3.0) <= 0.018


# ---------------------------------------------------------------- exact cases

def test_a_closed_room_is_closed_and_a_short_reach_opens_it(room):
    for samples in (1, 64, 200):
        assert ar.ambient(room, ORIGIN, UP, INF, 0.001, samples, 5)[0, 0] == 0
        rec = ar.ambient(room, ORIGIN, UP, 0.9, 0.001, samples, 5)[0]           # every wall is at least 1 - 0.001 away
        assert rec[0] == samples
        _, d, _ = ar.rays(ORIGIN, UP, 0.001, samples, 5)
        assert (rec[1:4] == ar.bent_terms(d[0]).sum(axis=0)).all()
    # max_dist = 0: t < 0 never holds, every sample is open
    assert ar.ambient(room, ORIGIN, UP, 0.0, 0.001, 64, 5)[0, 0] == 64


def test_side_minus_one_looks_below_a_ceiling(lone_quad):
    # the quad as a ceiling: from below it, the flipped normal finds it and the plain one does not
    under = F([[0, 0, -0.5]])
    assert ar.ambient(lone_quad, under, UP, INF, 0.001, 64, 3)[0, 0] < 64       # up: the ceiling blocks what points at it
    assert ar.ambient(lone_quad, under, -UP, INF, 0.001, 64, 3)[0, 0] == 64     # side = -1: open below
    on_top = F([[0, 0, 0]])
    assert ar.ambient(lone_quad, on_top, -UP, INF, 0.001, 64, 3)[0, 0] == 64    # bias moves the origin below the quad
    assert ar.ambient(lone_quad, on_top, -UP, INF, -0.001, 64, 3)[0, 0] == 0    # ... and a negative one above it: all blocked


def test_skipped_points_and_non_finite_inputs(room):
    pts = np.repeat(ORIGIN, 6, axis=0)
    nrm = np.repeat(UP, 6, axis=0)
    max_dist = F([-1.0, np.nan, np.inf, np.inf, np.inf, -0.0])
    pts[2, 1] = np.nan                                                          # a NaN in p: o is a NaN, nothing is hit
    nrm[3, 0] = np.nan                                                          # a NaN in n: o and d are NaNs
    got = ar.ambient(room, pts, nrm, max_dist, 0.001, 64, 9)
    assert (got[0] == ar.SKIPPED).all() and (got[1] == ar.SKIPPED).all()
    # NaN p: every sample open, bent as for the finite point (d does not depend on p)
    _, d, _ = ar.rays(pts, nrm, 0.001, 64, 9)
    assert got[2, 0] == 64 and (got[2, 1:4] == ar.bent_terms(d[2]).sum(axis=0)).all()
    # NaN n: every sample open; the restatement's cast rule makes a NaN product add 0, so the sums are 0
    assert np.isnan(d[3]).all() and (got[3] == [64, 0, 0, 0]).all()
    assert got[4, 0] == 0
    assert got[5, 0] == 64                                                      # -0.0 >= 0: live, and max_dist = 0 is all open
    # the cast's rule at its edges
    assert list(ar.bent_terms(F([np.nan, np.inf, -np.inf, 1.0, -1.0, 0.99999, -0.5, 32767.99, 32768.0, -32768.0]))) == \
        [0, 0, 0, 65536, -65536, 65535, -32768, 2147483008, 0, 0]


def test_one_sample_and_the_streams_of_first(room):
    rng = np.random.default_rng(2)
    n = 40
    pts = np.concatenate([rng.uniform(-0.9, 0.9, (n, 2)), np.zeros((n, 1))], axis=1).astype(F)
    nrm = np.repeat(UP, n, axis=0)
    reach = rng.uniform(0.3, 2.5, n).astype(F)
    one = ar.ambient(room, pts, nrm, reach, 0.001, 1, 4)
    assert set(one[:, 0]) <= {0, 1} and 0 < one[:, 0].sum() < n
    whole = ar.ambient(room, pts, nrm, reach, 0.001, 16, 4, first=100)
    assert 0 <= whole[:, 0].min() < whole[:, 0].max() <= 16
    # two halves of a batch with `first` are the whole
    halves = np.concatenate([ar.ambient(room, pts[:17], nrm[:17], reach[:17], 0.001, 16, 4, first=100),
                             ar.ambient(room, pts[17:], nrm[17:], reach[17:], 0.001, 16, 4, first=117)])
    assert (halves == whole).all()
    # a permutation of the points with matching first offsets: point by point
    perm = rng.permutation(n)
    for k in perm[:10]:
        assert (ar.ambient(room, pts[k:k + 1], nrm[k:k + 1], reach[k:k + 1], 0.001, 16, 4, first=100 + int(k)) == whole[k]).all()
    # the last indices of a stream (the entry point refuses first + n > 2^32)
    assert (ar.ambient(room, pts[:2], nrm[:2], reach[:2], 0.001, 16, 4, first=2 ** 32 - 2) ==
            np.concatenate([ar.ambient(room, pts[k:k + 1], nrm[k:k + 1], reach[k:k + 1], 0.001, 16, 4, first=2 ** 32 - 2 + k) for k in (0, 1)])).all()


def test_cut_outs_are_seen_through():
    osc = oracle.Scene.load_glb(scene_path("mc_transparency")).build_bvh(20, 8)
    rng = np.random.default_rng(6)
    # points on up-facing triangles of the scene (the ground under the cut-out leaves among them)
    p = osc.tris["p"]
    fn = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    up = np.nonzero(fn[:, 1] > 0.5 * np.linalg.norm(fn, axis=1))[0]
    k = rng.choice(up, 60)
    pts = p[k].mean(axis=1).astype(F)
    nrm = np.tile(F([0, 1, 0]), (len(k), 1))
    live, occ, d = ar.sample_occlusion(osc, pts, nrm, INF, 0.001, 16, 11)
    _, occ_opaque, _ = ar.sample_occlusion(ar.opaque(osc), pts, nrm, INF, 0.001, 16, 11)
    assert live.all() and not (occ & ~occ_opaque).any()
    seen_through = occ_opaque & ~occ
    print("%d of %d samples blocked, %d more if the cut-outs were opaque" % (occ.sum(), occ.size, seen_through.sum()))
    assert seen_through.sum() > 0 and occ.sum() > 0
    got = ar.ambient(osc, pts, nrm, INF, 0.001, 16, 11)
    assert (got[:, 0] == 16 - occ.sum(axis=1)).all()
    o, d2, _ = ar.rays(pts, nrm, 0.001, 16, 11)
    direct = rq.occluded(osc, np.repeat(o, 16, axis=0), d2.reshape(-1, 3), F(0), INF).reshape(-1, 16)
    assert (direct == occ).all()
