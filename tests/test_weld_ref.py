"""tests/weld_ref.py on its own, without a GPU: hand cases of the welding rule, the topology of welded isosurfaces by integers and
against the edge adjacency, the fixed-point normals against a float64 sum without fixed point, and what smoothing keeps and changes."""
import numpy as np
import pytest

from tests import isosurface_ref as iso
from tests import weld_ref as wd

drt = pytest.importorskip("dustraytracer_amd")

_cache = {}


def shape(name):
    """(tris [N, 3, 3], vertices, faces, first) of the restatement's isosurface of a sphere (two resolutions) or a torus, welded"""
    if name not in _cache:
        if name.startswith("sphere"):
            lo, hi = np.float32([-1.03, -1.01, -1.02]), np.float32([1.01, 1.04, 1.02])
            f, cell = iso.sphere_sdf(int(name[6:]), lo, hi, 0.8)
        else:
            lo, hi = np.float32([-1.45, -1.43, -0.47]), np.float32([1.47, 1.44, 0.45])
            f, cell = iso.torus_sdf(20, lo, hi, 0.9, 0.3)
        t = iso.triangles(iso.isosurface(f, 0.0, lo, cell)[1])
        _cache[name] = (t,) + wd.weld(t)[:3]
    return _cache[name]


def test_hand_cases():
    one = np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
    v, f, first, n = wd.weld(one)
    assert n == 3 and f.tolist() == [[0, 1, 2]] and first.tolist() == [0, 1, 2] and v.tobytes() == one.tobytes()
    two = np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[1, 0, 0], [1, 1, 0], [0, 1, 0]]])       # they share the edge (1,0,0)-(0,1,0)
    v, f, first, n = wd.weld(two)
    assert n == 4 and f.tolist() == [[0, 1, 2], [1, 3, 2]] and first.tolist() == [0, 1, 2, 4]
    assert v.tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]]
    assert wd.twins_of(f).tolist() == [[-1, 5, -1], [-1, -1, 1]] == drt.triEdgeAdjacency(two).tolist()
    zeros = np.zeros((1, 3, 3), np.float32)
    zeros[0, 1, 2] = -0.0                                                                         # -0.0 is another vertex than +0.0
    v, f, first, n = wd.weld(zeros)
    assert n == 2 and f.tolist() == [[0, 1, 0]] and np.signbit(v[1, 2]) and not np.signbit(v[0, 2])
    nans = np.zeros((1, 3, 3), np.float32)
    nans.view(np.uint32)[0, :, 0] = 0x7FC00000, 0x7FC00001, 0x7FC00000                           # NaNs are compared by their bits
    v, f, first, n = wd.weld(nans)
    assert n == 2 and f.tolist() == [[0, 1, 0]] and v.view(np.uint32)[:, 0].tolist() == [0x7FC00000, 0x7FC00001]
    thrice = np.full((1, 3, 3), 2.5, np.float32)
    v, f, first, n = wd.weld(thrice)
    assert n == 1 and f.tolist() == [[0, 0, 0]] and first.tolist() == [0]
    assert wd.weld(np.zeros((0, 3, 3), np.float32))[3] == 0
    packed = np.zeros((2, 12), np.float32)
    packed[:, 0:9], packed[:, 9:] = two.reshape(2, 9), 7.0
    assert wd.weld(packed)[1].tolist() == [[0, 1, 2], [1, 3, 2]]
    v, f, first, n = wd.weld(two, capacity=2)                                                     # truncated: faces and the count are whole
    assert n == 4 and len(v) == 2 and first.tolist() == [0, 1] and f.tolist() == [[0, 1, 2], [1, 3, 2]]


@pytest.mark.parametrize("name, chi", [("sphere14", 2), ("torus", 0)])
def test_welded_isosurfaces_are_closed_manifolds_by_integers(name, chi):
    t, v, f, first = shape(name)
    edges, uses = wd.edges_of(f)
    assert (uses == 2).all() and len(v) - len(edges) + len(f) == chi
    assert iso.euler(t) == (len(v), len(edges), len(f))
    assert v[f].tobytes() == t.tobytes() and (np.diff(first) > 0).all()     # the gather gives the soup back; first appearance
    adj = drt.triEdgeAdjacency(t)
    assert (adj >= 0).all() and wd.twins_of(f).tolist() == adj.tolist()      # the index buffer reproduces the adjacency's twins


def brute_normals(v, f, weight):
    """the same weights summed in float64 with numpy's arctan2 and no fixed point"""
    p = v.astype(np.float64)[f]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    length = np.linalg.norm(n, axis=1)
    ok = length > 0
    acc = np.zeros((len(v), 3))
    for k in range(3):
        a, b = p[:, (k + 1) % 3] - p[:, k], p[:, (k + 2) % 3] - p[:, k]
        w = n if weight == wd.AREA else np.arctan2(length, (a * b).sum(axis=1))[:, None] * n / np.where(ok, length, 1)[:, None]
        np.add.at(acc, f[ok, k], w[ok])
    total = np.linalg.norm(acc, axis=1, keepdims=True)
    return acc / np.where(total > 0, total, 1)


# The worst deviation per component measured on the CPU, times four for other fp32 roundings of the terms.  Measured: sphere14 angle
# 1.22e-6, area 3.67e-5; torus angle 2.53e-5, area 3.87e-2.  The area weights' figure is large because a vertex that only sliver
# triangles name sums fp32 cross products that cancel to a few bits: it is the rule's conditioning there, not the fixed point.
@pytest.mark.parametrize("name, weight, measured", [("sphere14", wd.ANGLE, 1.22e-6), ("sphere14", wd.AREA, 3.67e-5),
                                                    ("torus", wd.ANGLE, 2.53e-5), ("torus", wd.AREA, 3.87e-2)])
def test_normals_against_a_float64_sum_without_fixed_point(name, weight, measured):
    _, v, f, _ = shape(name)
    sums = np.zeros((len(v), 3), np.int64)
    n = wd.vertex_normals(v, f, weight, sums=sums)
    worst = np.abs(n - brute_normals(v, f, weight)).max()
    print("%s weight %d: worst deviation %.3g" % (name, weight, worst))
    assert worst <= 4 * measured
    assert np.abs(sums).max() < 2 ** 40 and np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() < 1e-6


@pytest.mark.parametrize("weight", [wd.ANGLE, wd.AREA])
def test_sphere_normals_come_closer_to_radial_with_resolution(weight):
    worst = []
    for name in ("sphere14", "sphere28"):
        _, v, f, _ = shape(name)
        radial = v.astype(np.float64) / np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)
        worst.append(np.abs(wd.vertex_normals(v, f, weight) - radial).max())
    print("worst deviation from radial: %.4f at 14^3, %.4f at 28^3" % tuple(worst))
    assert worst[1] < worst[0]                                              # the finer is closer; no absolute figure


def test_triangles_that_add_nothing():
    _, v, f, _ = shape("sphere14")
    v, f = np.concatenate([v, np.float32([[9, 9, 9]])]), f.copy()
    base = wd.vertex_normals(v, f)
    assert not base[-1].any()                                               # a vertex in no triangle: zeros
    g = np.concatenate([f, [[0, 1, len(v)], [-1, 2, 3], [4, 4, 5], [6, 7, 6]]]).astype(np.int32)
    for w in (wd.ANGLE, wd.AREA):                                           # out of range on both sides, no area: nothing changes
        assert wd.vertex_normals(v, g, w).tobytes() == wd.vertex_normals(v, f, w).tobytes()
    bad = v.copy()
    bad[f[10, 0]] = np.nan, 0, 0
    n = wd.vertex_normals(bad, f)
    touched = np.unique(f[(f == f[10, 0]).any(axis=1)])
    rest = np.setdiff1d(np.arange(len(v)), touched)
    assert n[rest].tobytes() == base[rest].tobytes() and not n[f[10, 0]].any() and np.isfinite(n).all()


def test_smoothing_keeps_what_it_must():
    _, v, f, _ = shape("sphere14")
    assert wd.smooth(v, f, []).tobytes() == v.tobytes() and wd.smooth(v, f, [0.0, 0.0]).tobytes() == v.tobytes()
    fixed = np.zeros(len(v), bool)
    fixed[::5] = True
    s = wd.smooth(v, f, [0.5, -0.53] * 3, fixed)
    assert s[fixed].tobytes() == v[fixed].tobytes() and (s[~fixed] != v[~fixed]).any(axis=1).mean() > 0.99
    # an index out of range and a NaN vertex change nothing else: the triangles that name them drop out, and nothing more
    g = f.copy()
    g[7, 1], g[9, 0] = len(v), -1
    keep = np.ones(len(f), bool)
    keep[[7, 9]] = False
    assert wd.smooth(v, g, [0.5, -0.53]).tobytes() == wd.smooth(v, f[keep], [0.5, -0.53]).tobytes()
    bad = v.copy()
    bad[f[10, 0], 2] = np.nan
    without = ~(f == f[10, 0]).any(axis=1)
    got, want = wd.smooth(bad, f, [0.5]), wd.smooth(bad, f[without], [0.5])
    assert got.tobytes() == want.tobytes() and got[f[10, 0]].tobytes() == bad[f[10, 0]].tobytes()
    # a mean of points inside the bounds stays inside them, and |q| < 2^28 whatever the scale
    for scale in (np.float32(2.0 ** -130), np.float32(1.0), np.float32(2.0 ** 120)):
        p = v * scale
        m = np.abs(p).max()
        assert np.abs(wd.fixed(p, 27 - wd.exponent(m))).max() < 2 ** 28
        assert np.abs(wd.smooth(p, f, [1.0])).max() <= m


def face_deviation(v, f):
    """area-weighted mean angle, in degrees, between a face's normal and the direction of its centroid"""
    t = v.astype(np.float64)[f]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    area, c = np.linalg.norm(n, axis=1), t.mean(axis=1)
    ok = area > 0
    cos = (n[ok] * c[ok]).sum(axis=1) / (area[ok] * np.linalg.norm(c[ok], axis=1))
    return float((np.degrees(np.arccos(np.clip(cos, -1, 1))) * area[ok]).sum() / area[ok].sum())


def test_a_taubin_smoothed_sphere_is_still_closed_and_rounder():
    _, v, f, _ = shape("sphere14")
    s = wd.smooth(v, f, [0.5, -0.53] * 10)
    t = s[f]
    assert (drt.triEdgeAdjacency(np.ascontiguousarray(t)) >= 0).all()       # one closed manifold, by the adjacency of the gathered soup
    vv, ff, _, n = wd.weld(t)
    edges, uses = wd.edges_of(ff)
    assert (uses == 2).all() and n - len(edges) + len(ff) == 2 and n == len(v)     # no two vertices fell together
    before, after = face_deviation(v, f), face_deviation(s, f)
    print("face normals against radial: %.3f degrees before, %.3f after; volume %.5f before, %.5f after (the ball's: %.5f)"
          % (before, after, iso.signed_volume(v[f]), iso.signed_volume(t), 4.0 / 3.0 * np.pi * 0.8 ** 3))
    assert after < before
