"""Restatement of drt_renderer_ambient_occlusion (include/drt.h) over the oracle's scene, for the tests.  No tests of its own.

One numpy operation per header operation, float32 throughout: pcg_hash is tests/radiance_ref.py's, the unit-sphere draw is the
oracle's pinned known-answer entry (oracle.kat_unitsphere, the renderer's routine with its guard), the traversal is
tests/ray_query_ref.py's occluded, and the record is integer sums.
"""
import numpy as np

import oracle
from tests import ray_query_ref as rq
from tests.radiance_ref import _normalize, pcg_hash

F = np.float32
SKIPPED = np.array([-1, 0, 0, 0], np.int32)
MAX_SAMPLES = 4096


def _u32(x):
    return np.asarray(x, np.uint64).astype(np.uint32)


def rays(points, normals, bias, samples, seed, first=0):
    """(o [N, 3], d [N, S, 3], tries [N, S]): the origin of every point and the direction of every sample, with the number of
    candidates the rejection loop drew."""
    points, normals = np.ascontiguousarray(points, F).reshape(-1, 3), np.ascontiguousarray(normals, F).reshape(-1, 3)
    n = len(points)
    bias = np.broadcast_to(np.asarray(bias, F), n)
    with np.errstate(all="ignore"):
        i = _u32((np.arange(n, dtype=np.uint64) + np.uint64(first)) & np.uint64(0xFFFFFFFF))
        h = pcg_hash(i ^ pcg_hash(_u32([seed]))[0])                                       # h = pcg((first + i) ^ pcg(seed))
        state = pcg_hash(np.arange(samples, dtype=np.uint32)[None, :] ^ h[:, None])        # state = pcg(j ^ h)
        fuzz, _, tries = oracle.kat_unitsphere(state.reshape(-1))                          # fuzz = randomUnitSphereVec3(state)
        d = _normalize((np.repeat(normals, samples, axis=0) + fuzz).astype(F))             # d = normalize(n + fuzz)
        o = (points + (normals * bias[:, None]).astype(F)).astype(F)                       # o = p + n * bias
    return o, d.reshape(n, samples, 3), tries.reshape(n, samples)


def bent_terms(d):
    """(int32_t)(d[k] * 65536.0f), truncated; a NaN or a product not below 2^31 in magnitude adds 0."""
    with np.errstate(all="ignore"):
        c = (np.asarray(d, F) * F(65536.0)).astype(F)
        ok = np.abs(c) < F(2147483648.0)
    return np.where(ok, c, F(0)).astype(np.int32)                                          # (astype truncates towards zero)


def sample_occlusion(osc, points, normals, max_dist, bias, samples, seed, first=0):
    """(live [N], occluded [N, S] bool, d [N, S, 3]): which samples drt_renderer_occluded calls occluded; nothing is traced for a
    skipped point."""
    o, d, _ = rays(points, normals, bias, samples, seed, first)
    n = len(o)
    max_dist = np.broadcast_to(np.asarray(max_dist, F), n)
    with np.errstate(invalid="ignore"):
        live = max_dist >= F(0)                                                            # !(max_dist >= 0): skipped
    occ = np.zeros((n, samples), bool)
    k = np.nonzero(live)[0]
    if len(k):
        with np.errstate(all="ignore"):
            occ[k] = rq.occluded(osc, np.repeat(o[k], samples, axis=0), d[k].reshape(-1, 3), F(0),
                                 np.repeat(max_dist[k], samples)).reshape(len(k), samples)
    return live, occ, d


def ambient(osc, points, normals, max_dist, bias, samples, seed, first=0):
    """drt_ao_result of every point: int32 [N, 4] = {open, bent[3]}."""
    assert 1 <= samples <= MAX_SAMPLES
    live, occ, d = sample_occlusion(osc, points, normals, max_dist, bias, samples, seed, first)
    is_open = ~occ & live[:, None]
    out = np.zeros((len(live), 4), np.int64)
    out[:, 0] = is_open.sum(axis=1)
    out[:, 1:4] = (bent_terms(d).astype(np.int64) * is_open[:, :, None]).sum(axis=1)
    out[~live] = SKIPPED
    assert np.abs(out).max(initial=0) <= 1 << 28
    return out.astype(np.int32)


def opaque(osc):
    """The same scene without its textures: every alpha test passes (what a traversal that ignored the cut-outs would see)."""
    import copy
    o = copy.copy(osc)
    o.mats = osc.mats.copy()
    o.mats["albedo_tex"] = -1
    return o


def flat_scene(drt, pos, normal=(0, 0, 1), leaf=2, bins=8):
    """(product scene, oracle scene) of untextured triangles pos [n, 3, 3]."""
    pos = np.ascontiguousarray(pos, F)
    n = len(pos)
    return rq.programmatic_scene(drt, pos, np.tile(F(normal), (n, 3, 1)), np.zeros((n, 3, 2), F), np.zeros(n, np.int32),
                                 [((0.8, 0.7, 0.6), -1)], [], leaf, bins)


def quad(x0, x1, y0, y1, z):
    """Two triangles spanning [x0, x1] x [y0, y1] at height z."""
    return F([[[x0, y0, z], [x1, y0, z], [x1, y1, z]], [[x0, y0, z], [x1, y1, z], [x0, y1, z]]])


def rect(a, b, c):
    """Two triangles spanning the parallelogram a, a + b, a + b + c, a + c."""
    a, b, c = (np.asarray(v, np.float64) for v in (a, b, c))
    return F([[a, a + b, a + b + c], [a, a + b + c, a + c]])


def box(lo, hi):
    """The twelve triangles of a closed axis-aligned box."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    e = np.diag(hi - lo)
    faces = []
    for axis in range(3):
        u, v = e[(axis + 1) % 3], e[(axis + 2) % 3]
        faces += [rect(lo, u, v), rect(lo + e[axis], u, v)]
    return np.concatenate(faces).astype(F)
