"""Made-up adaptive-sampling states for the weights stage (drt_debug_adaptive_weights): every branch and rounding border of the
weight rule in include/drt.h, as a table that tests/adaptive_ref.py decides and the kernel has to agree with bit for bit.  No tests
of its own: tests/test_adaptive_ref.py checks that the table is what it claims to be, tests/test_gpu_adaptive_edges.py runs it.

Negative m1 is left out on purpose.  The luminance of radiance is never negative, so the rule does not define it, and a negative s
is converted to uint32 differently by C on the host, by numpy (wraps) and by the device (saturates): the table encodes none of them.
"""
import numpy as np

from tests import adaptive_ref as ar

F = np.float32
TARGET_ERROR = 0.05                              # the positive target_error the table's `w <= target_error` runs are built for
LUMA_FLOORS = (0.01, 1e-30)                      # the default and a tiny one (mean + luma_floor == mean for all but denormal means)
N_EDGES = [0, 1, 2, 3, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31, 2 ** 32 - 1]
RUN = 64                                         # consecutive float32 values of m2 per border run
_tables = {}


def _state(n, m1, m2):
    n = np.asarray(n, np.uint64).astype(np.uint32)
    return ar.State(np.zeros((len(n), 3), F), n, np.asarray(m1, F), np.asarray(m2, F))


def raw_variance(state):
    """m2 / n - mean * mean before the clamp, as the rule rounds it (NaN and -inf included)."""
    with np.errstate(all="ignore"):
        fn = state.n.astype(F)
        mean = (state.m1 / fn).astype(F)
        return ((state.m2 / fn).astype(F) - (mean * mean).astype(F)).astype(F)


def w_of(state, luma_floor):
    """The rule's w (before the two decisions), float32."""
    with np.errstate(all="ignore"):
        fn = state.n.astype(F)
        mean = (state.m1 / fn).astype(F)
        var = np.fmax(raw_variance(state), F(0)).astype(F)
        return (np.sqrt((var / fn).astype(F)).astype(F) / (mean + F(luma_floor)).astype(F)).astype(F)


def constant_luminance(rng):
    """Pixels whose samples all had the same luminance Y: m2 / n and mean * mean differ by rounding only.  Sums accumulated sample by
    sample as the fold does (small n), and n * Y, n * (Y * Y) rounded once (any n)."""
    n, m1, m2 = [], [], []
    for count in (2, 3, 5, 6, 7, 10, 11, 13, 100, 1000):
        for y in rng.uniform(0.01, 4.0, 12).astype(F):
            a = b = F(0)
            for _ in range(count):
                a, b = F(a + y), F(b + F(y * y))
            n.append(count), m1.append(a), m2.append(b)
    for count in (3, 7, 2 ** 24 - 1, 2 ** 24 + 1, 2 ** 31, 2 ** 32 - 1):
        for y in rng.uniform(1e-3, 100.0, 12).astype(F):
            n.append(count), m1.append(F(F(count) * y)), m2.append(F(F(count) * F(y * y)))
    return _state(n, m1, m2)


def moment_edges():
    """Every n of N_EDGES with every pair of edge moments."""
    tiny, big = F(1e-45), F(3.0e38)                              # the smallest denormal; near FLT_MAX (3.4e38)
    pairs = [(0, 0),
             (1.0, np.inf), (np.inf, 1.0), (np.inf, np.inf), (np.nan, 1.0), (1.0, np.nan), (np.nan, np.nan),
             (tiny, tiny), (F(1e-40), tiny), (F(1e-40), F(1e-39)), (F(1e-38), F(1e-42)), (0, F(1e-39)), (0, tiny), (F(3e-39), F(9e-39)),
             (F(1.1754942e-38), F(1.1754942e-38)),                # the largest denormal
             (big, big), (big, F(3.4028235e38)), (F(3.4028235e38), big), (F(1e30), big), (F(1e20), F(1e38)), (F(2e19), F(3e38))]
    n = np.repeat(np.array(N_EDGES, np.uint64), len(pairs))
    m1 = np.tile(np.array([p[0] for p in pairs], F), len(N_EDGES))
    m2 = np.tile(np.array([p[1] for p in pairs], F), len(N_EDGES))
    return _state(n, m1, m2)


def noisy(rng, pixels=800):
    """States as renders make them: n samples of a luminance drawn around a per-pixel level, folded in order (n < 2: unknown)."""
    n = rng.integers(0, 40, pixels)
    level = rng.uniform(0.02, 2.0, pixels)
    spread = rng.choice([0.0, 0.01, 0.1, 0.5, 1.0, 3.0], pixels)
    m1, m2 = np.zeros(pixels, F), np.zeros(pixels, F)
    for p in range(pixels):
        ys = (level[p] * (1.0 + spread[p] * rng.uniform(-1, 1, n[p]) ** 3)).clip(0).astype(F)
        ys[rng.random(n[p]) < 0.02 * spread[p]] *= F(200.0)      # fireflies
        for y in ys:
            m1[p], m2[p] = F(m1[p] + y), F(m2[p] + F(y * y))
    return _state(n, m1, m2)


def border_run(n, m1, luma_floor, w_target, flips):
    """RUN consecutive float32 values of m2 around the one where flips(w) turns True, with n and m1 fixed.  w does not decrease
    with m2 (every operation of the rule is monotonic), so the flip is one point; adaptive_ref places it."""
    mean = float(F(m1) / F(n))
    guess = F(n * (n * (w_target * (mean + luma_floor)) ** 2 + mean * mean))
    span = 1 << 15
    bits = (int(guess.view(np.uint32)) + np.arange(-span, span)).astype(np.uint32)       # positive floats are ordered as their bits
    m2 = bits.view(F)
    st = _state(np.full(len(m2), n), np.full(len(m2), m1, F), m2)
    side = flips(w_of(st, luma_floor))
    assert not side[0] and side[-1] and (np.diff(side.astype(int)) >= 0).all(), "no single flip within 2^15 values of the estimate"
    at = int(np.argmax(side))
    take = slice(at - RUN // 2, at + RUN // 2)
    return _state(st.n[take], st.m1[take], st.m2[take])


def concat(states):
    return ar.State(*(np.concatenate([getattr(s, f) for s in states]) for f in ar.State._fields))


def border_runs(luma_floor, which):
    """The runs of one decision border, `which` = "target" (w <= target_error) or "cap" (s < 16777215.0f)."""
    te = F(TARGET_ERROR)
    bases = ((16, 8.0), (3, 0.75), (1000, 2500.0))
    if which == "target":
        # (the last three: var > mean * mean, so w moves by less than one float32 per value of m2 and takes the value target_error
        # itself, the one input that tells `<=` from `<`)
        bases += ((4096, 100.0), (100000, 3.0), (2 ** 24, 5.0e4))
        return [border_run(n, m1, luma_floor, float(te), lambda w: ~(w <= te)) for n, m1 in bases]
    return [border_run(n, m1 * 1e-3, luma_floor, 256.0, lambda w: ~((w * F(65536.0)).astype(F) < F(16777215.0))) for n, m1 in bases]


def weight_table(luma_floor):
    """The whole table for one luma_floor (the border runs depend on it), shuffled so that every class meets every wave border."""
    if luma_floor not in _tables:
        rng = np.random.default_rng(2024)
        t = concat([moment_edges(), constant_luminance(rng), noisy(rng)] + border_runs(luma_floor, "target") + border_runs(luma_floor, "cap"))
        order = rng.permutation(len(t.n))
        _tables[luma_floor] = ar.State(*(a[order] for a in t))
    return _tables[luma_floor]


def states(size, luma_floor):
    """`size` states: the table from its start, repeated where size is larger."""
    t = weight_table(luma_floor)
    idx = np.arange(size) % len(t.n)
    return ar.State(*(a[idx] for a in t))
