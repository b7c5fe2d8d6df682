"""Restatement of the two batched ray queries (include/drt.h drt_renderer_trace_rays / drt_renderer_occluded) over the
oracle's scene, for the tests.  No tests of its own.

The traversals are BVH/BVHTraversal.cuh's (citations relative to the reference's src/), vectorised over rays: every step
pops one stack entry of every ray that still has one.  All arithmetic on rays, boxes and triangles is the oracle's pinned
known-answer entries (oracle.kat_slab, kat_intersect, kat_texalpha); only interp_uv (RayGen.cuh:116, AnyHit.cuh:20-22) is
restated, in float32 numpy, in the reference's order.
"""
import collections

import numpy as np

import oracle

FLT_MAX = np.float32(np.finfo(np.float32).max)
Hits = collections.namedtuple("Hits", "t prim u v")
MAX_STACK = 64


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _interp_uv(uv3, uvw):
    """uvw.x * uv0 + uvw.y * uv1 + uvw.z * uv2, float32, left to right (RayGen.cuh:116)."""
    x, y, z = uvw[:, 0:1], uvw[:, 1:2], uvw[:, 2:3]
    return ((x * uv3[:, 0] + y * uv3[:, 1]) + z * uv3[:, 2]).astype(np.float32)


def any_hit(osc, prim, uvw):
    """AnyHit.cuh:8-28 for triangles `prim` hit at barycentrics `uvw` [k, 3]: True unless an RGBA albedo texture's alpha < 1."""
    prim = np.asarray(prim, np.int64)
    ok = np.ones(len(prim), bool)
    if len(prim) == 0:
        return ok
    tex = osc.mats["albedo_tex"][osc.tris["material"][prim]]
    for ti in np.unique(tex[tex >= 0]):
        texels = osc.textures[int(ti)]
        if texels.shape[2] < 4:
            continue
        sel = np.nonzero(tex == ti)[0]
        uv = _interp_uv(osc.tris["uv"][prim[sel]], _f32(uvw[sel]))
        alpha = oracle.kat_texalpha(texels, uv)
        ok[sel] = ~(alpha < 1)
    return ok


def _tri_test(osc, rays6, prim):
    """Intersection.cu on (ray, triangle) pairs: (hit, t, uvw[k, 3])."""
    out, hit = oracle.kat_intersect(rays6, osc.tris["p"][prim].reshape(-1, 9))
    return hit != 0, out[:, 0], out[:, 1:4]


def _slab(osc, rays6, node):
    nd = osc.nodes[node]
    return oracle.kat_slab(rays6, np.concatenate([nd["bmin"], nd["bmax"]], axis=1))


def closest(osc, org, dirs, tmin, tmax):
    """traverseBVH (:14-73) started as TraceRay starts it (TraceRay.cu:15-32), with the interval changes of drt.h."""
    n = len(org)
    rays6 = _f32(np.concatenate([org, dirs], axis=1))
    tmin, tmax = _f32(np.broadcast_to(tmin, n)), _f32(np.broadcast_to(tmax, n))
    best_t, best_prim = tmax.copy(), np.full(n, -1, np.int32)                  # TraceRay.cu:18 closest.t = ray.interval.max
    best_u, best_v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    if len(osc.nodes) == 0 or n == 0:
        return Hits(best_t, best_prim, best_u, best_v)
    root = len(osc.nodes) - 1                                                  # the root is the last node (BVHBuilder.cu:85)
    st_node = np.zeros((n, MAX_STACK), np.int64)
    st_dist = np.zeros((n, MAX_STACK), np.float32)
    st_node[:, 0] = root
    st_dist[:, 0] = _slab(osc, rays6, np.full(n, root))                        # :23-24
    sp = np.ones(n, np.int64)
    while True:
        act = np.nonzero(sp > 0)[0]
        if len(act) == 0:
            break
        sp[act] -= 1                                                           # :34-35 pop
        node, dist = st_node[act, sp[act]], st_dist[act, sp[act]]
        keep = (np.float32(-1) < dist) & (dist < tmax[act])                     # :38 interval (-1, tmax).surrounds
        keep &= ~((best_prim[act] >= 0) & (best_t[act] < dist))                 # :41
        act, node = act[keep], node[keep]
        leaf = osc.nodes["is_leaf"][node] != 0
        # ---- leaves (:45-58): the triangles in order; strict <, t > tmin (drt.h), then AnyHit ----
        la, ln = act[leaf], node[leaf]
        start, count = osc.nodes["prim_start"][ln], osc.nodes["prim_count"][ln]
        for k in range(int(count.max()) if len(ln) else 0):
            sel = count > k
            r, prim = la[sel], (start[sel] + k).astype(np.int64)
            h, t, uvw = _tri_test(osc, rays6[r], prim)
            h &= (t < best_t[r]) & (t > tmin[r])                                # :51 + inner clipping
            r, prim, t, uvw = r[h], prim[h], t[h], uvw[h]
            ok = any_hit(osc, prim, uvw)                                        # :52
            r, prim, t, uvw = r[ok], prim[ok], t[ok], uvw[ok]
            best_t[r], best_prim[r], best_u[r], best_v[r] = t, prim, uvw[:, 1], uvw[:, 2]
        # ---- interior nodes (:60-71): both children's boxes, the farther one pushed first ----
        ia, inode = act[~leaf], node[~leaf]
        if len(ia):
            c1, c2 = osc.nodes["child1"][inode], osc.nodes["child2"][inode]
            d1, d2 = _slab(osc, rays6[ia], c1), _slab(osc, rays6[ia], c2)
            p1 = (d1 >= 0) & (d1 < best_t[ia])
            p2 = (d2 >= 0) & (d2 < best_t[ia])
            far1 = d1 > d2                                                      # :63
            for push, c, d in ((np.where(far1, p1, p2), np.where(far1, c1, c2), np.where(far1, d1, d2)),
                               (np.where(far1, p2, p1), np.where(far1, c2, c1), np.where(far1, d2, d1))):
                r = ia[push]
                st_node[r, sp[r]], st_dist[r, sp[r]] = c[push], d[push]
                sp[r] += 1
    return Hits(best_t, best_prim, best_u, best_v)


def occluded(osc, org, dirs, tmin, tmax):
    """traverseBVH_raytest (:76-134) with the interval changes of drt.h."""
    n = len(org)
    rays6 = _f32(np.concatenate([org, dirs], axis=1))
    tmin, tmax = _f32(np.broadcast_to(tmin, n)), _f32(np.broadcast_to(tmax, n))
    occ = np.zeros(n, bool)
    if len(osc.nodes) == 0 or n == 0:
        return occ
    root = len(osc.nodes) - 1
    d = _slab(osc, rays6, np.full(n, root))
    st = np.zeros((n, MAX_STACK), np.int64)
    st[:, 0] = root
    sp = np.where((d < 0) | (d > tmax), 0, 1)                                   # :95-103 root only, + tmax
    while True:
        act = np.nonzero((sp > 0) & ~occ)[0]
        if len(act) == 0:
            break
        sp[act] -= 1
        node = st[act, sp[act]]
        leaf = osc.nodes["is_leaf"][node] != 0
        la, ln = act[leaf], node[leaf]
        start, count = osc.nodes["prim_start"][ln], osc.nodes["prim_count"][ln]
        for k in range(int(count.max()) if len(ln) else 0):                    # :106-117, first hit returns
            sel = (count > k) & ~occ[la]
            r, prim = la[sel], (start[sel] + k).astype(np.int64)
            h, t, uvw = _tri_test(osc, rays6[r], prim)
            h &= (t > tmin[r]) & (t < tmax[r])
            r, prim, uvw = r[h], prim[h], uvw[h]
            occ[r[any_hit(osc, prim, uvw)]] = True
        ia, inode = act[~leaf], node[~leaf]
        if len(ia):
            c1, c2 = osc.nodes["child1"][inode], osc.nodes["child2"][inode]
            h1, h2 = _slab(osc, rays6[ia], c1), _slab(osc, rays6[ia], c2)
            p1 = (h1 >= 0) & ~(h1 > tmax[ia])                                   # :122-129, + tmax
            p2 = (h2 >= 0) & ~(h2 > tmax[ia])
            far1 = h1 > h2
            for push, c in ((np.where(far1, p1, p2), np.where(far1, c1, c2)), (np.where(far1, p2, p1), np.where(far1, c2, c1))):
                r = ia[push]
                st[r, sp[r]] = c[push]
                sp[r] += 1
    return occ


def brute_force(osc, org, dirs, tmin, tmax):
    """Every ray x triangle pair: (minimum accepted t or tmax, per-pair accepted mask [n, T], t [n, T]).
    A pair is accepted when Intersection.cu hits, tmin < t < tmax and AnyHit passes."""
    n, T = len(org), len(osc.tris)
    rays6 = _f32(np.repeat(np.concatenate([org, dirs], axis=1), T, axis=0))
    prim = np.tile(np.arange(T), n)
    h, t, uvw = _tri_test(osc, rays6, prim)
    tmin_r, tmax_r = np.repeat(_f32(np.broadcast_to(tmin, n)), T), np.repeat(_f32(np.broadcast_to(tmax, n)), T)
    h &= (t > tmin_r) & (t < tmax_r)
    idx = np.nonzero(h)[0]
    h[idx] = any_hit(osc, prim[idx], uvw[idx])
    acc, t = h.reshape(n, T), t.reshape(n, T)
    tbest = np.where(acc, t, np.inf).min(axis=1) if T else np.full(n, np.inf)
    return np.where(np.isfinite(tbest), tbest, _f32(np.broadcast_to(tmax, n))).astype(np.float32), acc, t


# ---------------------------------------------------------------- ray sets shared by the CPU and GPU tests

def camera_rays(cam, W, H):
    """Frame-1 camera rays of every pixel, row-major from y = 0: seed x + y*W, uv ((float)x/W)*2-1 (drt_oracle.c ray_gen)."""
    y, x = np.mgrid[0:H, 0:W]
    x, y = x.ravel().astype(np.uint32), y.ravel().astype(np.uint32)
    uv = np.stack([(x.astype(np.float32) / np.float32(W)) * np.float32(2) - np.float32(1),
                   (y.astype(np.float32) / np.float32(H)) * np.float32(2) - np.float32(1)], axis=1).astype(np.float32)
    r6, _ = oracle.kat_getray(cam, W, H, uv, x + y * np.uint32(W))
    return r6[:, :3].copy(), r6[:, 3:].copy()


def scene_bounds(osc):
    p = osc.tris["p"].reshape(-1, 3)
    return p.min(axis=0), p.max(axis=0)


def surface_rays(osc, n, rng):
    """Rays from random points on random triangles in random directions (not normalised)."""
    prim = rng.integers(0, len(osc.tris), n)
    b = rng.uniform(0, 1, (n, 2)).astype(np.float32)
    b = np.where(b.sum(axis=1, keepdims=True) > 1, 1 - b, b).astype(np.float32)
    p = osc.tris["p"][prim]
    org = (p[:, 0] + b[:, 0:1] * (p[:, 1] - p[:, 0]) + b[:, 1:2] * (p[:, 2] - p[:, 0])).astype(np.float32)
    dirs = rng.normal(size=(n, 3)).astype(np.float32) * rng.uniform(0.2, 3.0, (n, 1)).astype(np.float32)
    return org, dirs.astype(np.float32)


def interval_rays(osc, n, rng):
    """Random origins in and around the scene, random directions and random [tmin, tmax] -- tmax inside the scene, NaN,
    negative, zero, infinite -- as (org, dirs, tmin, tmax)."""
    lo, hi = scene_bounds(osc)
    ext = (hi - lo).astype(np.float32)
    org = (lo - 0.25 * ext + rng.uniform(0, 1.5, (n, 3)) * ext).astype(np.float32)
    dirs = rng.normal(size=(n, 3)).astype(np.float32)
    diag = np.float32(np.linalg.norm(ext))
    tmax = rng.uniform(0, 2 * diag, n).astype(np.float32)
    tmin = np.where(rng.uniform(size=n) < 0.5, np.float32(0), rng.uniform(0, 1, n).astype(np.float32) * tmax).astype(np.float32)
    k = rng.integers(0, 8, n)
    tmax = np.where(k == 0, np.float32(np.nan), tmax)
    tmax = np.where(k == 1, -tmax, tmax)
    tmax = np.where(k == 2, np.float32(np.inf), tmax)
    tmax = np.where(k == 3, FLT_MAX, tmax)
    tmax = np.where(k == 4, np.float32(0), tmax)
    tmin = np.where(k == 5, np.float32(np.nan), tmin)
    tmin = np.where(k == 6, -tmin - 1, tmin)
    return org, dirs, tmin.astype(np.float32), tmax.astype(np.float32)


def axis_rays(osc, n, rng):
    """Directions with one or two zero components (+0 or -0) from origins inside the scene's bounds."""
    lo, hi = scene_bounds(osc)
    org = (lo + rng.uniform(0, 1, (n, 3)) * (hi - lo)).astype(np.float32)
    dirs = rng.normal(size=(n, 3)).astype(np.float32)
    zero = rng.uniform(size=(n, 3)) < 0.5
    zero[np.arange(n), rng.integers(0, 3, n)] = False                          # keep one component
    sign = np.where(rng.uniform(size=(n, 3)) < 0.5, np.float32(0.0), np.float32(-0.0))
    dirs = np.where(zero, sign, dirs).astype(np.float32)
    # some origins exactly on a triangle vertex plane: coordinates copied from vertices
    v = osc.tris["p"].reshape(-1, 3)
    pick = rng.uniform(size=(n, 3)) < 0.2
    org = np.where(pick, v[rng.integers(0, len(v), (n, 3)), np.arange(3)[None, :]], org).astype(np.float32)
    return org, dirs


def box_rays(osc, n, rng):
    """Rays starting inside BVH boxes (random nodes)."""
    nd = osc.nodes[rng.integers(0, len(osc.nodes), n)]
    org = (nd["bmin"] + rng.uniform(0, 1, (n, 3)) * (nd["bmax"] - nd["bmin"])).astype(np.float32)
    return org, rng.normal(size=(n, 3)).astype(np.float32)


def programmatic_scene(drt, pos, nrm, uv, mat, materials, textures, leaf, bins):
    """The same de-indexed geometry given to the product (Scene.setGeometry) and to the oracle, both built with (leaf, bins)."""
    sc = drt.Scene()
    for tex in textures:
        sc.addTexture(tex)
    for alb, tex in materials:
        sc.addMaterial(alb, tex)
    sc.setGeometry(pos, nrm, uv, mat)
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = leaf, bins
    b.buildIterative(sc)
    n = len(mat)
    tris = np.zeros(n, oracle.TRI_DTYPE)
    a = [np.ascontiguousarray(x, np.float32) for x in (pos.reshape(-1, 3), nrm.reshape(-1, 3), uv.reshape(-1, 2))]
    m = np.ascontiguousarray(mat, np.int32)
    oracle.lib().o_build_triangles(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, m.ctypes.data, n, tris.ctypes.data)
    return sc, oracle.Scene(tris, materials, textures).build_bvh(leaf, bins)


def soup(n, seed, half=0.25, spread=4.0):
    """A triangle soup with RGB and RGBA (cut-out) textures: (pos, nrm, uv, mat, materials, textures)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-spread, spread, (n, 1, 3)).astype(np.float32)
    pos = (c + rng.uniform(-half, half, (n, 3, 3))).astype(np.float32)
    nrm = rng.normal(size=(n, 3, 3)).astype(np.float32)
    uv = rng.uniform(-2, 3, (n, 3, 2)).astype(np.float32)
    tex_rgb = rng.integers(0, 256, (19, 23, 3), dtype=np.uint8)
    tex_rgba = rng.integers(0, 256, (8, 8, 4), dtype=np.uint8)
    tex_rgba[..., 3] = np.where(rng.uniform(size=(8, 8)) < 0.5, 255, 40)
    materials = [((0.9, 0.9, 0.9), -1), ((1.0, 1.0, 1.0), 0), ((0.7, 0.8, 0.9), 1)]
    mat = rng.integers(0, 3, n).astype(np.int32)
    return pos, nrm, uv, mat, materials, [tex_rgb, tex_rgba]


def degenerate_chain(n=62):
    """Triangles whose centroids double in x: with leaf size 1 and two bins one peels off per level (a tree of ~n levels)."""
    cx = (2.0 ** np.arange(n)).astype(np.float32)
    pos = np.zeros((n, 3, 3), np.float32)
    pos[:, :, 0] = cx[:, None]
    pos += (np.float32([[0, -1, -1], [0, 1, -1], [0, 0, 1]]) * 0.4)[None] * cx[:, None, None]
    nrm = np.tile(np.float32([-1, 0, 0]), (n, 3, 1))
    return pos, nrm, np.zeros((n, 3, 2), np.float32), np.zeros(n, np.int32), [((0.7, 0.6, 0.5), -1)], []
