"""The rule of adaptive sampling (include/drt.h) as tests/adaptive_ref.py restates it, on states made by hand: what the GPU tests
compare the kernels with has to be right on its own.  No GPU."""
import numpy as np
import pytest

from tests import adaptive_cases as ac
from tests import adaptive_ref as ar

F = np.float32
CAP = 16777215


def state_of(samples):
    """The state of pixels that received the given luminance-only samples (grey colours): samples = list of lists."""
    st = ar.empty_state(len(samples))
    for p, ys in enumerate(samples):
        for y in ys:
            c = np.array([y, y, y], F)
            Y = ar.lum(c)
            st.sum[p] = (st.sum[p] + c).astype(F)
            st.m1[p] = F(st.m1[p] + Y)
            st.m2[p] = F(st.m2[p] + F(Y * Y))
            st.n[p] += 1
    return st


def test_lum_is_the_headers():
    c = np.array([0.3, 0.6, 0.9], F)
    assert ar.lum(c) == F(F(F(0.2126) * c[0] + F(0.7152) * c[1]) + F(0.0722) * c[2])


def test_all_unknown_is_uniform():
    for pixels, budget in ((1, 1), (7, 7 * 3), (7, 7 * 3 + 6), (3072, 3 * 3072)):
        q, c = ar.plan(ar.empty_state(pixels), budget, max_spp=8)
        assert (q == CAP).all() and (c == budget // pixels).all()
    st = state_of([[0.5], [0.1], [0.9]])                 # one sample each: still unknown
    q, c = ar.plan(st, 30, min_spp=2)
    assert (q == CAP).all() and (c == 10).all()


def test_weight_by_hand():
    # two samples 0.25 and 0.75 of a grey pixel: Y = lum, mean = 0.5, var = 1/16, w = sqrt(1/32) / (0.5 + 0.01)
    st = state_of([[0.25, 0.75]])
    w = np.sqrt(1.0 / 32.0) / 0.51
    q = ar.weights(st)
    assert abs(int(q[0]) - w * 65536.0) <= 2 + w * 65536.0 * 4e-6    # (a handful of fp32 roundings; the bit-exact check is the GPU's)
    assert ar.weights(state_of([[0.5, 0.5, 0.5]]))[0] == 0        # no variance: converged, whatever the target is


def test_q_zero_fallback():
    st = state_of([[0.5, 0.5]] * 5)
    q, c = ar.plan(st, 5 * 2 + 13, min_spp=2, max_spp=64)         # Q == 0, target_error == 0: min_spp + extra / pixels
    assert (q == 0).all() and (c == 2 + 13 // 5).all()
    q, c = ar.plan(st, 5 * 2 + 500, min_spp=2, max_spp=7)
    assert (c == 7).all()
    q, c = ar.plan(st, 5 * 2 + 13, min_spp=2, target_error=1e-3)  # thresholded: every pixel is converged and gets nothing
    assert (q == 0).all() and (c == 0).all()


def test_one_hot_pixel_is_clamped_at_max_spp():
    st = state_of([[0.5, 0.5]] * 9 + [[0.0, 1.0]])
    q, c = ar.plan(st, 10 + 1000, max_spp=64)
    assert q[9] > 0 and (q[:9] == 0).all()
    assert c[9] == 64 and (c[:9] == 1).all()                      # target_error == 0: a converged pixel keeps min_spp
    assert c.sum() <= 1010                                        # what the clamp drops is not redistributed


def test_target_error_zeroes_pixels_below_it():
    st = state_of([[0.5, 0.5], [0.49, 0.51], [0.0, 1.0], [0.2]])
    w1 = (0.01 / np.sqrt(2.0)) / 0.51                             # pixel 1's relative standard error, about 0.0139
    q = ar.weights(st, target_error=2 * w1)
    assert q[0] == 0 and q[1] == 0 and q[2] > 0 and q[3] == CAP
    q = ar.weights(st, target_error=0.5 * w1)
    assert q[0] == 0 and q[1] > 0
    q, c = ar.plan(st, 4 + 40, target_error=2 * w1)
    assert c[0] == 0 and c[1] == 0 and c[2] >= 1 and c[3] >= 1 and c.sum() <= 44


def test_nan_and_inf_take_the_cap():
    st = ar.State(np.ones((5, 3), F), np.full(5, 4, np.uint32), np.array([np.nan, 1.0, 0.0, 1e-30, 2.0], F),
                  np.array([1.0, np.nan, np.inf, 1e30, 1.5], F))
    for te in (0.0, 0.1):
        q = ar.weights(st, target_error=te, luma_floor=1e-30)
        assert q[0] == CAP                                        # NaN mean: w is NaN
        assert q[2] == CAP                                        # infinite variance: w is +inf
        assert q[3] == CAP                                        # finite but huge: s >= 16777215
        assert 0 < q[4] < CAP
    assert ar.weights(st, luma_floor=1e-30)[1] == 0               # fmaxf(NaN, 0) = 0: no variance


@pytest.mark.parametrize("seed", range(6))
def test_counts_stay_within_the_budget(seed):
    rng = np.random.default_rng(seed)
    pixels = int(rng.integers(1, 3000))
    q = rng.integers(0, CAP + 1, pixels, dtype=np.uint32)
    q[rng.random(pixels) < 0.3] = 0
    q[rng.random(pixels) < 0.05] = CAP
    min_spp = int(rng.integers(0, 4))
    max_spp = min_spp + int(rng.integers(1, 64))
    budget = min_spp * pixels + int(rng.integers(0, 40 * pixels))
    for th in (False, True):
        c, Q = ar.counts(q, budget, min_spp, max_spp, thresholded=th)
        assert Q == sum(int(v) for v in q)
        assert int(c.sum(dtype=np.uint64)) <= budget and c.max() <= max_spp
        assert (c[q > 0] >= min_spp).all()
        assert (c[q == 0] == (0 if th else min_spp)).all() or Q == 0
    big = (1 << 31) - 1                                           # extra * q needs more than 32 bits
    c, Q = ar.counts(q, big, 0, big)
    assert int(c.sum(dtype=np.uint64)) <= big
    if Q:
        assert (c == [(big * int(v)) // Q for v in q]).all()


def test_floors_drop_less_than_one_sample_per_pixel():
    rng = np.random.default_rng(11)
    q = rng.integers(1, 1 << 20, 500, dtype=np.uint32)            # none converged, none near max_spp
    budget = 500 * 1 + 7777
    c, _ = ar.counts(q, budget, 1, 1 << 20)
    assert budget - 500 < int(c.sum()) <= budget


def test_offsets_fold_and_image():
    c = np.array([2, 0, 3, 0, 0, 1], np.uint32)
    assert (ar.offsets(c) == [0, 2, 2, 5, 5, 5]).all()
    assert (ar.offsets(np.array([5], np.uint32)) == [0]).all()
    frames = {k: np.full((3, 3), k, F) * np.array([[1], [10], [100]], F) for k in range(1, 8)}
    st = ar.fold(ar.empty_state(3), np.array([2, 0, 3], np.uint32), lambda k: frames[k])
    assert (st.n == [2, 0, 3]).all() and (st.sum[:, 0] == [3, 0, 600]).all()
    st = ar.fold(st, np.array([1, 2, 0], np.uint32), lambda k: frames[k])      # pixel 0 takes frame 3, pixel 1 frames 1 and 2
    assert (st.n == [3, 2, 3]).all() and (st.sum[:, 0] == [6, 30, 600]).all()
    assert st.m1[1] == F(ar.lum(frames[1][1]) + ar.lum(frames[2][1]))
    img = ar.image(st)
    assert (img[:, 0] == [2, 15, 200]).all() and (img[:, 3] == 1).all()
    assert (ar.image(ar.empty_state(2)) == [0, 0, 0, 1]).all()


# ---------------------------------------------------------------- the edge table of the weights stage (tests/adaptive_cases.py)

@pytest.mark.parametrize("luma_floor", ac.LUMA_FLOORS)
def test_the_weight_table_is_what_it_claims_to_be(luma_floor):
    t = ac.weight_table(luma_floor)
    P = len(t.n)
    assert P <= 3000, "the largest size of the GPU test has to hold the whole table"
    assert not (t.m1 < 0).any(), "negative m1 is left out (see adaptive_cases)"
    q = ar.weights(t, ac.TARGET_ERROR, luma_floor)
    for what, share in (("converged", (q == 0).mean()), ("cap", (q == CAP).mean()), ("in between", ((q > 0) & (q < CAP)).mean())):
        assert share >= 0.10, "%s: %.1f %% of the table" % (what, 100 * share)
    q0 = ar.weights(t, 0.0, luma_floor)
    assert ((q0 > 0) & (q == 0)).mean() >= 0.05, "target_error has to decide a fair share"
    # every n and every kind of moment the table promises
    assert set(ac.N_EDGES) <= set(int(v) for v in t.n)
    for n in ac.N_EDGES:
        assert ((t.n == n) & (t.m1 == 0) & (t.m2 == 0)).any(), n
    tiny = np.finfo(F).tiny
    big = (t.n >= 2)
    assert (big & np.isposinf(t.m2) & np.isfinite(t.m1)).any() and (big & np.isposinf(t.m1) & np.isposinf(t.m2)).any()
    assert (big & np.isnan(t.m1)).any() and (big & np.isnan(t.m2)).any()
    assert (big & (t.m1 > 0) & (t.m1 < tiny)).any() and (big & (t.m2 > 0) & (t.m2 < tiny)).any()
    with np.errstate(all="ignore"):
        mean = (t.m1 / t.n.astype(F)).astype(F)
        assert (big & np.isfinite(mean) & np.isinf((mean * mean).astype(F)) & np.isfinite((t.m2 / t.n.astype(F)).astype(F))).any(), \
            "mean * mean overflows while m2 / n does not"
    raw = ac.raw_variance(t)
    assert (big & np.isnan(raw) & ~np.isnan(t.m1) & ~np.isnan(t.m2)).any(), "inf - inf"
    # constant luminance: the clamp is reached by rounding alone, and missed by rounding alone
    c = ac.constant_luminance(np.random.default_rng(2024))
    raw = ac.raw_variance(c)
    assert (raw < 0).sum() >= 10 and (raw > 0).sum() >= 10 and (raw == 0).sum() >= 1


@pytest.mark.parametrize("luma_floor", ac.LUMA_FLOORS)
def test_both_border_runs_contain_the_flip(luma_floor):
    for run in ac.border_runs(luma_floor, "target"):
        assert len(run.n) == ac.RUN and (np.diff(run.m2.view(np.uint32).astype(np.int64)) == 1).all()      # consecutive float32 values
        q = ar.weights(run, ac.TARGET_ERROR, luma_floor)
        assert (q[:ac.RUN // 2] == 0).all() and (q[ac.RUN // 2:] > 0).all() and (q[ac.RUN // 2:] < CAP).all()
        assert (ar.weights(run, 0.0, luma_floor) > 0).all()
    assert sum(int((ac.w_of(run, luma_floor) == F(ac.TARGET_ERROR)).sum()) for run in ac.border_runs(luma_floor, "target")) >= 3, \
        "w == target_error itself has to be in the table: the one input that tells `<=` from `<`"
    for run in ac.border_runs(luma_floor, "cap"):
        assert len(run.n) == ac.RUN and (np.diff(run.m2.view(np.uint32).astype(np.int64)) == 1).all()
        for te in (0.0, ac.TARGET_ERROR):
            q = ar.weights(run, te, luma_floor)
            assert (q[:ac.RUN // 2] < CAP).all() and q[ac.RUN // 2 - 1] >= CAP - 8 and (q[ac.RUN // 2:] == CAP).all()
    t = ac.weight_table(luma_floor)                                # and the table holds them
    rows = set(zip(t.n.tolist(), t.m1.view(np.uint32).tolist(), t.m2.view(np.uint32).tolist()))
    for which in ("target", "cap"):
        for run in ac.border_runs(luma_floor, which):
            assert set(zip(run.n.tolist(), run.m1.view(np.uint32).tolist(), run.m2.view(np.uint32).tolist())) <= rows
