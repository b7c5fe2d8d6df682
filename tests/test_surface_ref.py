"""What the numpy restatement of the surface lookups and the area-weighted sampling (tests/surface_ref.py) is worth, without a GPU:
hand cases on a triangle with distinct uvs, normals and materials, hostile references, the oracle's texel lookups on the textured test
scenes, the integer weights against a plain cumulative sum and on degenerate meshes, the samples' exactness, their independence of the
batch split and their distribution.  tests/test_gpu_surface.py compares the kernels with it word for word."""
import math

import numpy as np
import pytest

import oracle
from tests import surface_ref as sr
from tests.scenes import scene_path

drt = pytest.importorskip("dustraytracer_amd")

F = np.float32
TINY = F(-1e-9)


def hand_scene():
    """Three triangles with integer corners, a flat, a 3-channel and a 4-channel material.  The vertex uvs of the textured ones are the
    interesting ones: exactly 1 (wraps to texel 0) and a tiny negative one (its fractional part rounds to 1: the padding texel)."""
    pos = np.float32([[[0, 0, 0], [4, 0, 0], [0, 4, 0]], [[8, 0, 0], [12, 0, 0], [8, 4, 0]], [[16, 0, 0], [20, 0, 0], [16, 4, 0]]])
    nrm = np.float32([[[1, 0, 0], [0, 1, 0], [0, 0, 1]]] * 3) * np.float32([1, 2, 3])[:, None, None]
    uv = np.float32([[[0.25, 0.5], [0.75, 0.5], [0.25, 1.5]], [[1.0, 0.5], [0.5, TINY], [TINY, 0.25]], [[1.0, 1.0], [0.3, TINY], [0.6, 0.6]]])
    rng = np.random.default_rng(1)
    textures = [rng.integers(1, 256, (4, 6, 3), dtype=np.uint8), rng.integers(1, 256, (5, 3, 4), dtype=np.uint8)]
    materials = [dict(albedo=(0.9, 0.5, 0.25), emissive=(1, 2, 3), roughness=0.5, metallic=True, refractive_index=1.25),
                 dict(albedo=(1, 1, 1), albedo_tex=0), dict(albedo=(1, 1, 1), albedo_tex=1, transmission=True)]
    sc = sr.product_scene(drt, pos, nrm, uv, np.int32([0, 1, 2]), materials, textures, leaf=1)
    return sc, pos, nrm, uv, textures


def by_load(s):
    """tree index of every load index"""
    inv = np.zeros(len(s.order), np.int64)
    inv[s.order] = np.arange(len(s.order))
    return inv


def test_hand_cases_corners_centroid_materials_and_the_padding_texel():
    sc, pos, nrm, uv, textures = hand_scene()
    s = sr.from_product(sc)
    tree = by_load(s)
    corners = [(0, 0), (1, 0), (0, 1)]
    for load in range(3):
        k = tree[load]
        rec = sr.lookup(s, [k] * 4, [0, 1, 0, 1 / 3], [0, 0, 1, 1 / 3])
        f = rec.view(F)
        for c in range(3):                                                                  # the corners are exact
            assert (f[c, sr.POSITION] == pos[load, c]).all() and (f[c, sr.SHADING] == nrm[load, c]).all() and (f[c, sr.UV] == uv[load, c]).all()
        third = pos[load].astype(np.float64).mean(axis=0)
        assert np.abs(f[3, sr.POSITION] - third).max() < 1e-5 and np.abs(f[3, sr.SHADING] - nrm[load].mean(axis=0)).max() < 1e-6
        assert (f[:, sr.NORMAL] == np.float32([0, 0, 1])).all()
        assert (rec[:, sr.MATERIAL] == load).all() and (rec[:, sr.LOAD_INDEX] == load).all()
        assert (rec[:, sr.TEXTURE].view(np.int32) == [-1, 0, 1][load]).all()
    flat = sr.lookup(s, [tree[0]], [0.25], [0.25])
    assert (flat.view(F)[0, sr.ALBEDO] == np.float32([0.9, 0.5, 0.25])).all() and flat.view(F)[0, sr.ALPHA] == 1
    assert (flat.view(F)[0, sr.EMISSIVE] == [1, 2, 3]).all() and flat.view(F)[0, sr.ROUGHNESS] == 0.5 and flat[0, sr.FLAGS] == 1
    assert flat.view(F)[0, sr.REFRACTIVE_INDEX] == 1.25
    sq = lambda c: (c.astype(F) / F(255)) * (c.astype(F) / F(255))
    # 3 channels, 6 x 4: uv (1, 0.5) -> x = 0 (1 wraps), y = 2; (0.5, tiny negative) -> y = height: the padding row; (tiny negative, 0.25) ->
    # x = width: the first texel of the next row
    t3 = sr.lookup(s, [tree[1]] * 3, [0, 1, 0], [0, 0, 1]).view(F)
    assert (t3[0, sr.ALBEDO] == sq(textures[0][2, 0])).all() and (t3[1, sr.ALBEDO] == 0).all() and (t3[2, sr.ALBEDO] == sq(textures[0][2, 0])).all()
    assert (t3[:, sr.ALPHA] == 1).all()
    # 4 channels, 3 x 5: (1, 1) -> texel (0, 0) with its alpha; (0.3, tiny negative) -> the padding: colour and alpha 0
    t4 = sr.lookup(s, [tree[2]] * 2, [0, 1], [0, 0])
    assert (t4.view(F)[0, sr.ALBEDO] == sq(textures[1][0, 0, :3])).all() and t4.view(F)[0, sr.ALPHA] == F(textures[1][0, 0, 3]) / F(255)
    assert (t4.view(F)[1, sr.ALBEDO] == 0).all() and t4.view(F)[1, sr.ALPHA] == 0 and (t4[:, sr.FLAGS] == 2).all()


def test_hostile_references():
    sc, pos, *_ = hand_scene()
    s = sr.from_product(sc)
    n = len(s.v0)
    miss = sr.lookup(s, [-1, n, -2 ** 31, 2 ** 31 - 1], [0.5] * 4, [0.25] * 4)
    assert (miss == sr.MISS).all() and (sr.MISS.view(np.int32)[[3, 11, 15]] == -1).all() and sr.MISS.sum() == 3 * 0xFFFFFFFF
    # outside the triangle everything extrapolates: no clamp
    k = by_load(s)[0]
    far = sr.lookup(s, [k], [3], [-2]).view(F)
    assert (far[0, sr.POSITION] == [12, -8, 0]).all() and (far[0, sr.UV] == np.float32([0.25 + 3 * 0.5, 0.5 - 2])).all()
    # a NaN or an infinity in (u, v): texel 0 of the texture is taken, nothing outside the pool is read (an index past a numpy
    # array would raise)
    for load in (1, 2):
        k = by_load(s)[load]
        tex = sc.m_Textures[load - 1]
        for u, v in ((np.nan, 0.5), (0.5, np.nan), (np.inf, 0.1), (0.1, -np.inf), (np.inf, np.inf), (3e38, 3e38)):
            rec = sr.lookup(s, [k], [u], [v]).view(F)
            if np.isfinite(u):
                continue                                                                     # (one component may still be finite)
            c = tex[0, 0, :3].astype(F) / F(255)
            assert (rec[0, sr.ALBEDO] == c * c).all(), (load, u, v)
    assert sr.texel_coord(F(np.nan), 7) == 0 and sr.texel_coord(F(np.inf), 7) == 0 and sr.texel_coord(F(-np.inf), 7) == 0
    assert sr.texel_coord(TINY, 7) == 7 and sr.texel_coord(F(1.0), 7) == 0 and sr.texel_coord(F(3e38), 7) == 0 and sr.texel_coord(F(-2.75), 8) == 2


@pytest.mark.parametrize("name", ["uv_texture_test", "mc_transparency"])
def test_albedo_and_alpha_are_the_oracle_s_texel_lookups(name):
    sc = drt.Scene()
    sc.loadGLTFmodel(scene_path(name))
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
    b.buildIterative(sc)
    s = sr.from_product(sc)
    rng = np.random.default_rng(4)
    n = 300
    prim = rng.integers(0, len(s.v0), n).astype(np.int32)
    u, v = rng.uniform(0, 1, n).astype(F), rng.uniform(0, 1, n).astype(F)
    flip = u + v > 1
    u[flip], v[flip] = 1 - u[flip], 1 - v[flip]
    rec = sr.lookup(s, prim, u, v).view(F)
    tex = rec.view(np.int32)[:, sr.TEXTURE]
    textures = sc.m_Textures
    assert (tex >= 0).sum() > 100
    for t in np.unique(tex[tex >= 0]):
        rows = tex == t
        assert (oracle.kat_texpixel(textures[t], rec[rows, sr.UV]) == rec[rows, sr.ALBEDO]).all()
        assert (oracle.kat_texalpha(textures[t], rec[rows, sr.UV]) == rec[rows, sr.ALPHA]).all()
    if name == "mc_transparency":
        assert (rec[:, sr.ALPHA] < 1).any() and (rec[:, sr.ALPHA] == 1).any()


def soup(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-4, 4, (n, 1, 3)) + rng.uniform(-0.5, 0.5, (n, 3, 3))).astype(F)


def test_weights_are_a_cumulative_sum_of_truncated_scaled_areas():
    p = soup(300, 2)
    s = sr.from_triangles(p)
    cdf = sr.weights(s)
    a = sr.areas(s)
    e = math.frexp(float(a.max()))[1]
    q = [int(float(x) * 2.0 ** (35 - e)) for x in a]
    assert cdf == list(np.cumsum(np.array(q, dtype=object))) and 2 ** 34 <= max(q) < 2 ** 35 and all(x < 2 ** 36 for x in q)
    # against float64 areas: every weight within one of the exactly scaled area up to fp32's rounding of a
    exact = np.linalg.norm(np.cross(s.e1.astype(np.float64), s.e2.astype(np.float64)), axis=1) * 2.0 ** (35 - e)
    assert np.abs(np.array(q, np.float64) - exact).max() <= 2 ** 35 * 2.0 ** -20


def test_degenerate_triangles_weigh_nothing():
    p = soup(40, 3)
    p[3, 2] = p[3, 1]                                    # zero area
    p[5] = p[5, 0]                                       # a point
    p[7, 1, 0] = np.nan
    p[9, 2, 2] = np.inf
    p[11] *= F(1e30)                                     # finite, and its squared cross product overflows: a = inf counts as 0
    s = sr.from_triangles(p)
    cdf = sr.weights(s)
    q = np.diff([0] + cdf)
    assert all(q[k] == 0 for k in (3, 5, 7, 9, 11)) and (np.delete(q, [3, 5, 7, 9, 11]) > 0).all()
    smp = sr.sample(s, 9, 0, 4000, cdf)
    assert not np.isin(smp.view(np.int32)[:, 1], [3, 5, 7, 9, 11]).any() and (smp.view(np.int32)[:, 1] >= 0).all()
    # an all-degenerate mesh: total 0, every sample is the miss record; and no triangles at all
    flat = sr.from_triangles(np.stack([p[:, 0]] * 3, axis=1))
    assert sr.weights(flat) == [0] * 40
    for scene in (flat, sr.from_triangles(np.zeros((0, 3, 3), F))):
        m = sr.sample(scene, 1, 0, 5)
        assert (m.view(np.int32)[:, 1] == -1).all() and not m[:, [0, 2, 3]].any()
    # areas 2^40 apart: the small one gets 0; 2^30 apart: it still counts
    big = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    for shift, counted in ((-20, False), (-15, True)):                                    # (lengths: the area is their square)
        two = sr.from_triangles(np.stack([big, big * F(2.0 ** shift)]))
        q = np.diff([0] + sr.weights(two))
        assert q[0] == 2 ** 34 and (q[1] > 0) == counted and q[1] == (2 ** (34 + 2 * shift) if counted else 0)


def test_scaling_by_powers_of_two_leaves_the_table_unchanged():
    p = soup(200, 5)
    p[4, 2] = p[4, 1]
    want = sr.weights(sr.from_triangles(p))
    for e in (-24, -7, 9, 24):
        assert sr.weights(sr.from_triangles(p * F(2.0 ** e))) == want, e
    # the smallest areas there are: the squared cross product is a subnormal, and a itself never is (a^2 >= 2^-149)
    tiny = np.float32([[[0, 0, 0], [2.0 ** -36, 0, 0], [0, 2.0 ** -36, 0]], [[0, 0, 0], [2.0 ** -37, 0, 0], [0, 2.0 ** -36, 0]]])
    assert list(sr.areas(sr.from_triangles(tiny))) == [2.0 ** -72, 2.0 ** -73]
    assert list(np.diff([0] + sr.weights(sr.from_triangles(tiny)))) == [2 ** 34, 2 ** 33]


def test_samples_are_exact_barycentrics_and_do_not_depend_on_the_split():
    s = sr.from_triangles(soup(100, 6))
    cdf = sr.weights(s)
    whole = sr.sample(s, 77, 1000, 3000, cdf)
    u, v = whole[:, 2].astype(np.float64), whole[:, 3].astype(np.float64)
    w = F(F(1) - whole[:, 2]) - whole[:, 3]
    assert (u >= 0).all() and (v >= 0).all() and (w >= 0).all() and (u + v + w.astype(np.float64) == 1).all() and not whole[:, 0].any()
    assert (np.ldexp(u, 24) == np.round(np.ldexp(u, 24))).all() and (np.ldexp(v, 24) == np.round(np.ldexp(v, 24))).all()
    parts = np.concatenate([sr.sample(s, 77, 1000, 1234, cdf), sr.sample(s, 77, 2234, 1766, cdf)])
    assert parts.tobytes() == whole.tobytes()
    assert sr.sample(s, 78, 1000, 50, cdf).tobytes() != whole[:50].tobytes()
    top = sr.sample(s, 77, 2 ** 32 - 10, 10, cdf)                                          # the last indices of a stream
    assert (top.view(np.int32)[:, 1] >= 0).all()
    assert sr.pcg(0) == 129708002 and sr.pcg(1) == 2831084092                              # the reference's pcg_hash


def test_counts_follow_the_areas():
    """Areas 1 : 2 : 4 : 0 and 2^16 samples of a fixed seed: every count within five binomial standard deviations of its share."""
    base = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    p = np.stack([base, base * np.float32([2, 1, 1]), base * np.float32([2, 2, 1]) + F(5), base * np.float32([1, 0, 1])])
    s = sr.from_triangles(p)
    assert list(sr.areas(s)) == [1, 2, 4, 0]
    n = 1 << 16
    prim = sr.sample(s, 2024, 0, n).view(np.int32)[:, 1]
    counts = np.bincount(prim, minlength=4)
    print("counts", counts.tolist())
    assert counts[3] == 0
    for k, share in enumerate((1 / 7, 2 / 7, 4 / 7)):
        assert abs(counts[k] - n * share) <= 5 * math.sqrt(n * share * (1 - share)), (k, counts[k])


def test_the_restatement_s_columns_are_the_header_s_record():
    """The columns the restatement writes are the fields of drt_surface in include/drt.h, in its order, four bytes a word."""
    import os
    import re

    from tests.scenes import ROOT
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    body = text[text.index("typedef struct drt_surface {"):text.index("} drt_surface;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    words, at = {}, 0
    for kind, name, count in re.findall(r"(float|int32_t|uint32_t)\s+(\w+)(?:\[(\d)\])?;", body):
        words[name] = (at, int(count or 1), kind)
        at += int(count or 1)
    assert at == 24
    col = lambda c: (c.start, c.stop - c.start) if isinstance(c, slice) else (c, 1)
    for name, c in (("position", sr.POSITION), ("material", sr.MATERIAL), ("normal", sr.NORMAL), ("alpha", sr.ALPHA), ("shading", sr.SHADING),
                    ("load_index", sr.LOAD_INDEX), ("albedo", sr.ALBEDO), ("texture", sr.TEXTURE), ("uv", sr.UV), ("roughness", sr.ROUGHNESS),
                    ("flags", sr.FLAGS), ("emissive", sr.EMISSIVE), ("refractive_index", sr.REFRACTIVE_INDEX)):
        assert words[name][:2] == col(c), name
        assert (words[name][2] == "float") == (col(c)[0] in sr.FLOAT_COLUMNS), name
    assert drt.SURFACE_SCAN_BLOCK == int(re.search(r"#define DRT_SURFACE_SCAN_BLOCK (\d+)", text).group(1))
