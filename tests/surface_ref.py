"""Surface lookups and area-weighted sampling restated in numpy (include/drt.h "surface lookups and area-weighted sampling"): one
operation per operation of the header, float32 throughout, the weights in Python integers.  The scene is read through the product's
getters (drt_scene_get_triangles, _materials, _texture_texels, triangleOrder); nothing here calls the device.

    lookup(s, prim, u, v, normals=None)  -> records uint32 [N, 24] (drt_surface)
    weights(s)                           -> the inclusive table as a list of Python integers
    sample(s, seed, first, n, cdf=None)  -> records float32 [N, 4] (drt_hit)
"""
import collections
import math

import numpy as np

SurfaceScene = collections.namedtuple("SurfaceScene", "v0 e1 e2 fn uv material normals order mats texs pool")
F = np.float32
MATERIAL_DTYPE = np.dtype({"names": ["albedo", "emissive", "albedo_tex", "roughness", "transmission", "refractive_index", "metallic"],      # drt_material
                           "formats": [("<f4", 3), ("<f4", 3), "<i4", "<f4", "u1", "<f4", "u1"],
                           "offsets": [0, 12, 24, 28, 32, 36, 40], "itemsize": 44})
MISS = np.zeros(24, np.uint32)
MISS[[3, 11, 15]] = 0xFFFFFFFF
# columns of a record
POSITION, MATERIAL, NORMAL, ALPHA, SHADING, LOAD_INDEX = slice(0, 3), 3, slice(4, 7), 7, slice(8, 11), 11
ALBEDO, TEXTURE, UV, ROUGHNESS, FLAGS, EMISSIVE, REFRACTIVE_INDEX = slice(12, 15), 15, slice(16, 18), 18, 19, slice(20, 23), 23
FLOAT_COLUMNS = [0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14, 16, 17, 18, 20, 21, 22, 23]


def pool_of(textures):
    """The renderer's texel pool: every texture followed by (width + 1) zero texels, then zeros up to a multiple of 16 bytes; and
    (width, height, channels, byte offset) per texture."""
    pool, texs = bytearray(), []
    for t in textures:
        h, w, c = t.shape
        texs.append((w, h, c, len(pool)))
        pool += np.ascontiguousarray(t, np.uint8).tobytes() + bytes((w + 1) * c)
        pool += bytes(-len(pool) % 16)
    return np.frombuffer(bytes(pool), np.uint8), texs


def from_product(sc, hot=None):
    """The product's host scene through its getters.  hot: TriHot records uint8 [n, 48] to use instead of the host triangles' (a
    renderer's device copy after a refit: Renderer.debugReadDeviceScene)."""
    t = sc.m_PrimitivesBuffer
    p = t["vertex"]["position"].astype(F)
    if hot is None:
        v0, e1, e2, fn = p[:, 0], p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], t["face_normal"].astype(F)
    else:
        h = np.ascontiguousarray(hot).view(F).reshape(-1, 12)
        v0, e1, e2, fn = h[:, 0:3], h[:, 3:6], h[:, 6:9], h[:, 9:12]
    pool, texs = pool_of(sc.m_Textures)
    return SurfaceScene(v0, e1, e2, fn, t["vertex"]["uv"].astype(F), t["material"].astype(np.int32), t["vertex"]["normal"].astype(F),
                        sc.triangleOrder(), sc.m_Material, texs, pool)


def from_triangles(p):
    """Triangles p [T, 3, 3] alone: one flat material, zero normals and uvs, load order = order (what the weights and samples read)."""
    p = np.ascontiguousarray(p, F).reshape(-1, 3, 3)
    n = len(p)
    mats = np.zeros(1, MATERIAL_DTYPE)
    mats["albedo_tex"] = -1
    with np.errstate(all="ignore"):
        e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    return SurfaceScene(p[:, 0], e1, e2, np.zeros((n, 3), F), np.zeros((n, 3, 2), F), np.zeros(n, np.int32), np.zeros((n, 3, 3), F),
                        np.arange(n, dtype=np.int32), mats, [], np.zeros(0, np.uint8))


def product_scene(drt, pos, nrm, uv, mat, materials, textures, leaf=2, bins=8):
    """A product scene from de-indexed geometry; materials: keyword arguments of Scene.addMaterialEx each."""
    sc = drt.Scene()
    for t in textures:
        sc.addTexture(t)
    for m in materials:
        sc.addMaterialEx(**m)
    sc.setGeometry(pos, nrm, uv, mat)
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = leaf, bins
    b.buildIterative(sc)
    return sc


def every_material(n_tris, seed):
    """(pos, nrm, uv, mat, materials, textures) for product_scene: a soup with one material of every kind -- flat, textured with 3 and
    with 4 channels, emissive, metallic, transmissive with its own index -- and uvs from -2 to 3."""
    rng = np.random.default_rng(seed)
    pos = (rng.uniform(-4, 4, (n_tris, 1, 3)) + rng.uniform(-0.5, 0.5, (n_tris, 3, 3))).astype(F)
    nrm = rng.normal(size=(n_tris, 3, 3)).astype(F)
    uv = rng.uniform(-2, 3, (n_tris, 3, 2)).astype(F)
    textures = [rng.integers(0, 256, (19, 23, 3), dtype=np.uint8), rng.integers(0, 256, (8, 5, 4), dtype=np.uint8)]
    materials = [dict(albedo=(0.9, 0.5, 0.25)), dict(albedo=(1, 1, 1), albedo_tex=0), dict(albedo=(0.7, 0.8, 0.9), albedo_tex=1, roughness=0.75),
                 dict(albedo=(0.1, 0.2, 0.3), emissive=(3, 2, 1)), dict(albedo=(0.6, 0.6, 0.6), metallic=True, roughness=0.125),
                 dict(albedo=(1, 1, 1), transmission=True, refractive_index=1.33), dict(albedo=(0.5, 0.5, 0.5), albedo_tex=1, metallic=True, transmission=True)]
    mat = (np.arange(n_tris) % len(materials)).astype(np.int32)
    return pos, nrm, uv, mat, materials, textures


def synthetic(n_tris, seed):
    """A scene made of arrays alone (no product, no tree): random triangles, seven materials of every kind -- flat, textured with 3, 4
    and 1 channels, metallic, transmissive, emissive --, odd-sized textures, uvs from -2 to 3, some zero-area, NaN and infinite
    triangles, a random load order."""
    rng = np.random.default_rng(seed)
    p = (rng.uniform(-4, 4, (n_tris, 1, 3)) + rng.uniform(-0.5, 0.5, (n_tris, 3, 3))).astype(F)
    p[3::17, 2] = p[3::17, 1]
    p[5::41, 1, 0] = np.nan
    p[7::43, 2, 1] = np.inf
    textures = [rng.integers(0, 256, (19, 23, 3), dtype=np.uint8), rng.integers(0, 256, (8, 5, 4), dtype=np.uint8),
                rng.integers(0, 256, (3, 7, 1), dtype=np.uint8)]
    pool, texs = pool_of(textures)
    mats = np.zeros(7, MATERIAL_DTYPE)
    mats["albedo"] = rng.uniform(0, 1, (7, 3))
    mats["albedo_tex"] = [-1, 0, 1, 2, -1, -7, 1]
    mats["emissive"][4] = (3, 2, 1)
    mats["roughness"] = rng.uniform(0, 1, 7)
    mats["metallic"][[4, 5]] = 1
    mats["transmission"][[5, 6]] = 1
    mats["refractive_index"] = rng.uniform(1, 2, 7)
    with np.errstate(invalid="ignore"):
        e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    return SurfaceScene(p[:, 0], e1, e2, rng.normal(size=(n_tris, 3)).astype(F), rng.uniform(-2, 3, (n_tris, 3, 2)).astype(F),
                        rng.integers(0, 7, n_tris).astype(np.int32), rng.normal(size=(n_tris, 3, 3)).astype(F),
                        rng.permutation(n_tris).astype(np.int32), mats, texs, pool)


def hostile_refs(n_tris, n, seed):
    """(prim int32 [n], u, v float32 [n]): references inside triangles, far outside them, with NaN and infinite u / v, and prim of -1,
    n_tris, INT_MIN, INT_MAX."""
    rng = np.random.default_rng(seed)
    prim = rng.integers(0, max(n_tris, 1), n).astype(np.int32)
    u, v = rng.uniform(0, 1, n).astype(F), rng.uniform(0, 1, n).astype(F)
    u[1::7], v[2::7] = rng.uniform(-50, 50, len(u[1::7])), rng.uniform(-1e6, 1e6, len(v[2::7]))
    u[3::31], v[4::31], u[5::37], v[6::37], u[8::41] = np.nan, np.nan, np.inf, -np.inf, 3e38
    prim[9::29], prim[10::53], prim[11::59], prim[12::61] = -1, n_tris, -2 ** 31, 2 ** 31 - 1
    return prim, u, v


def texel_coord(c, size):
    """(int)(f * size) with f = c - floorf(c), taken as 0 unless 0 <= f <= 1 (the departure: a NaN or infinite uv)."""
    with np.errstate(invalid="ignore"):
        f = F(c) - np.floor(F(c))
    if not (f >= 0 and f <= 1):
        f = F(0)
    return int(F(f * F(size)))


def lookup(s, prim, u, v, normals=None):
    """drt_renderer_surface_lookup.  normals: float32 [n_tris, 3, 3] in LOAD order, or None for the host scene's."""
    prim, u, v = np.asarray(prim, np.int32).reshape(-1), np.asarray(u, F).reshape(-1), np.asarray(v, F).reshape(-1)
    out = np.tile(MISS, (len(prim), 1))
    n_tris = len(s.v0)
    with np.errstate(all="ignore"):
        for i in range(len(prim)):
            k = int(prim[i])
            if not 0 <= k < n_tris:
                continue
            f = out[i].view(F)
            a, b = u[i], v[i]
            w = F(F(1.0) - a) - b
            load = int(s.order[k])
            nrm = s.normals[k] if normals is None else np.asarray(normals, F).reshape(-1, 3, 3)[load]
            f[POSITION] = (s.v0[k] + a * s.e1[k]) + b * s.e2[k]
            f[NORMAL] = s.fn[k]
            f[SHADING] = (w * nrm[0] + a * nrm[1]) + b * nrm[2]
            uv = (w * s.uv[k, 0] + a * s.uv[k, 1]) + b * s.uv[k, 2]
            f[UV] = uv
            m = s.mats[int(s.material[k])]
            alb, alpha, tex = m["albedo"].astype(F), F(1), int(m["albedo_tex"])
            if tex >= 0:
                width, height, comps, offset = s.texs[tex]
                t = texel_coord(uv[1], height) * width + texel_coord(uv[0], width)
                c = np.array([0, 0, 255], F)
                if comps in (3, 4):
                    c = s.pool[offset + t * comps:offset + t * comps + 3].astype(F)
                c = c / F(255)
                alb = c * c
                if comps >= 4:
                    alpha = F(s.pool[offset + t * 4 + 3]) / F(255)
            f[ALBEDO], f[ALPHA] = alb, alpha
            f[ROUGHNESS], f[EMISSIVE], f[REFRACTIVE_INDEX] = m["roughness"], m["emissive"], m["refractive_index"]
            out[i, MATERIAL], out[i, LOAD_INDEX] = np.uint32(int(s.material[k]) & 0xFFFFFFFF), np.uint32(load)
            out[i, TEXTURE] = np.uint32((tex if tex >= 0 else -1) & 0xFFFFFFFF)
            out[i, FLAGS] = (1 if m["metallic"] else 0) | (2 if m["transmission"] else 0)
    return out


def same(got, want):
    """Records equal word for word; in the float fields a NaN equals a NaN (which NaN is not specified)."""
    got = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 24)
    want = np.ascontiguousarray(want).view(np.uint32).reshape(-1, 24)
    if got.shape != want.shape:
        return False
    eq = got == want
    eq[:, FLOAT_COLUMNS] |= np.isnan(got.view(F)[:, FLOAT_COLUMNS]) & np.isnan(want.view(F)[:, FLOAT_COLUMNS])
    return bool(eq.all())


def areas(s):
    """a = sqrtf((c.x c.x + c.y c.y) + c.z c.z) of c = cross(e1, e2); a non-finite one counts as 0."""
    with np.errstate(all="ignore"):
        e1, e2 = s.e1.astype(F), s.e2.astype(F)
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        a = np.sqrt((cx * cx + cy * cy) + cz * cz).astype(F)
    return np.where(np.isfinite(a), a, F(0)).astype(F)


def weights(s):
    """drt_renderer_surface_weights: the inclusive sums of q_k = (uint64)ldexp((double)a_k, 35 - e) as Python integers."""
    a = areas(s)
    amax = float(a.max()) if len(a) else 0.0
    if amax == 0:
        return [0] * len(a)
    e = math.frexp(amax)[1]
    cdf, total = [], 0
    for x in a:
        total += int(math.ldexp(float(x), 35 - e))
        cdf.append(total)
    return cdf


def pcg(x):
    """The reference's pcg_hash (Random.cu:6-11) on Python integers."""
    state = (x * 747796405 + 2891336453) & 0xFFFFFFFF
    word = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & 0xFFFFFFFF
    return (word >> 22) ^ word


def sample(s, seed, first, n, cdf=None):
    """drt_renderer_sample_surface: records float32 [n, 4] = {t = 0, prim, u, v}."""
    cdf = weights(s) if cdf is None else [int(x) for x in cdf]
    total = cdf[-1] if cdf else 0
    out = np.zeros((n, 4), F)
    prims = out.view(np.int32)[:, 1]
    hs = pcg(seed)
    for k in range(n):
        if total == 0:
            prims[k] = -1
            continue
        i = first + k
        assert i < 1 << 32
        h1 = pcg(pcg(i ^ hs))
        h2 = pcg(h1)
        h3 = pcg(h2)
        h4 = pcg(h3)
        target = ((h1 << 32 | h2) * total) >> 64
        lo, hi = 0, len(cdf) - 1                         # the smallest k with cdf[k] > target
        while lo < hi:
            mid = lo + (hi - lo) // 2
            if cdf[mid] > target:
                hi = mid
            else:
                lo = mid + 1
        a, b = h3 >> 8, h4 >> 8
        if a + b > 1 << 24:
            a, b = (1 << 24) - a, (1 << 24) - b
        prims[k] = lo
        out[k, 2], out[k, 3] = F(a) * F(2.0 ** -24), F(b) * F(2.0 ** -24)
    return out
