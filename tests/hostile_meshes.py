"""Meshes that are not well behaved, and the queries aimed at them, for tests/test_hostile_meshes_ref.py (CPU) and
tests/test_gpu_hostile_meshes.py.  No tests of its own.

`degenerate`: ray_query_ref.soup(300, 3, 0.25, 2.0) plus zero-area triangles of every kind include/drt.h names (v0 = v1, v0 = v2,
v1 = v2, three collinear vertices with an exactly representable midpoint, all three equal), slivers (a collinear triple whose
midpoint was rounded), needles (two vertices 2^-12 apart, the third 2^4 away), exact duplicates of soup triangles and triangles that
share an edge with a soup triangle exactly.  Their vertices are copied from soup triangles and the order is shuffled, so that they
share leaves with real triangles.  `offset` is the same mesh moved by (4096, -8192, 16384) and rounded to fp32; `scaled(k)` is it
times 2^k, which is exact.  Every scene is built as ray_query_ref.programmatic_scene builds one: leaf 4, bins 8, one material.
"""
import collections

import numpy as np

import oracle
from tests import hits_ref as hr
from tests import inside_ref as ir
from tests import near_list_ref as nl
from tests import nearest_ref as nr
from tests import overlap_ref as ov
from tests import ray_query_ref as rq
from tests import refit_ref as rf
from tests import section_ref as sr
from tests import sweep_ref as sw
from tests import tri_overlap_ref as tv

LEAF, BINS = 4, 8
ONE_MATERIAL = [((0.8, 0.8, 0.8), -1)]
OFFSET = np.float32([4096, -8192, 16384])

# kinds of triangle, in Mesh.kind
SOUP, V0_V1, V0_V2, V1_V2, COLLINEAR, POINT, SLIVER, NEEDLE, DUPLICATE, SHARED_EDGE = range(10)
KIND_NAMES = ("soup", "v0 = v1", "v0 = v2", "v1 = v2", "collinear", "point", "sliver", "needle", "duplicate", "shared edge")
ZERO_AREA = (V0_V1, V0_V2, V1_V2, COLLINEAR, POINT)         # the stored e1 x e2 is exactly zero
THIN = ZERO_AREA + (SLIVER, NEEDLE)                         # what the aimed queries aim at

Mesh = collections.namedtuple("Mesh", "pos nrm uv mat kind twin")          # load order; twin: the other triangle of a duplicate pair, or -1
Queries = collections.namedtuple("Queries", "points radius casts rays boxes tris planes")


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _exact_midpoints(pos):
    """(triangle, edge) of the soup edges whose midpoint is a float32, and of those whose midpoint is not."""
    a, b = pos, np.roll(pos, -1, axis=1)
    mid = (a.astype(np.float64) + b.astype(np.float64)) / 2
    exact = (mid.astype(np.float32).astype(np.float64) == mid).all(axis=2)
    return np.argwhere(exact), np.argwhere(~exact)


def degenerate(seed=3):
    """The degenerate mesh in load order."""
    pos, nrm, _, _, _, _ = rq.soup(300, 3, 0.25, 2.0)
    rng = np.random.default_rng(seed)
    exact, rounded = _exact_midpoints(pos)
    tris, kinds = [pos], [np.full(300, SOUP)]
    take = iter(rng.permutation(300))                            # every added triangle copies its vertices from another soup triangle

    def add(t, kind):
        tris.append(_f32(t)[None])
        kinds.append(np.array([kind]))

    for _ in range(5):
        a = pos[next(take)]
        add([a[0], a[0], a[2]], V0_V1)
        a = pos[next(take)]
        add([a[0], a[1], a[0]], V0_V2)
        a = pos[next(take)]
        add([a[0], a[1], a[1]], V1_V2)
    for t, e in exact[rng.choice(len(exact), 5, replace=False)]:
        a, b = pos[t, e], pos[t, (e + 1) % 3]
        add([a, ((a.astype(np.float64) + b) / 2).astype(np.float32), b], COLLINEAR)
    for _ in range(4):
        a = pos[next(take)]
        add([a[1], a[1], a[1]], POINT)
    for t, e in rounded[rng.choice(len(rounded), 6, replace=False)]:
        a, b = pos[t, e], pos[t, (e + 1) % 3]
        add([a, ((a.astype(np.float64) + b) / 2).astype(np.float32), b], SLIVER)
    for _ in range(6):
        a = pos[next(take)][0]
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        w = np.cross(u, rng.normal(size=3))
        w /= np.linalg.norm(w)
        add([a, (a + 2.0 ** -12 * w).astype(np.float32), (a + 2.0 ** 4 * u).astype(np.float32)], NEEDLE)
    first_dup = sum(len(t) for t in tris)
    dup_of = np.array([next(take) for _ in range(20)])
    tris.append(pos[dup_of])
    kinds.append(np.full(20, DUPLICATE))
    for _ in range(4):
        a, b = pos[next(take)], pos[next(take)]
        add([a[1], a[0], b[2]], SHARED_EDGE)                     # the edge a0 a1 of a soup triangle, exactly, and a vertex of another
    p, kind = np.concatenate(tris).astype(np.float32), np.concatenate(kinds)
    n = len(p)
    twin = np.full(n, -1)
    twin[first_dup:first_dup + 20], twin[dup_of] = dup_of, first_dup + np.arange(20)
    order = np.random.default_rng(seed + 1).permutation(n)
    inverse = np.empty(n, np.int64)
    inverse[order] = np.arange(n)
    twin = np.where(twin[order] >= 0, inverse[np.maximum(twin[order], 0)], -1)
    more = np.random.default_rng(seed + 2).normal(size=(n, 3, 3)).astype(np.float32)
    more[:300] = nrm
    return Mesh(p[order], more[order], np.zeros((n, 3, 2), np.float32), np.zeros(n, np.int32), kind[order], twin)


def without_thin(mesh):
    """The mesh without its zero-area triangles, slivers and needles, the rest in the same order (what the refit test loads)."""
    keep = ~np.isin(mesh.kind, THIN)
    renumber = np.cumsum(keep) - 1
    return Mesh(mesh.pos[keep], mesh.nrm[keep], mesh.uv[keep], mesh.mat[keep], mesh.kind[keep], np.where(mesh.twin[keep] >= 0, renumber[np.maximum(mesh.twin[keep], 0)], -1))


def collapsed(mesh, seed=5):
    """Positions for a refit of without_thin(degenerate()) into degeneracy: 20 soup triangles collapse, four of each zero-area kind,
    and 10 more move exactly onto other soup triangles.  Returns (positions, kind after the refit)."""
    rng = np.random.default_rng(seed)
    pos, kind = mesh.pos.copy(), mesh.kind.copy()
    soup = (mesh.kind == SOUP) & (mesh.twin < 0)
    exact, _ = _exact_midpoints(mesh.pos)
    exact = [t for t, e in exact if e == 0 and soup[t]][:4]      # the edge v0 v1 has a float32 midpoint
    assert len(exact) == 4
    pick = [t for t in rng.permutation(np.nonzero(soup)[0]) if t not in exact]
    for j, k in enumerate((V0_V1, V0_V2, V1_V2, POINT)):
        for t in pick[4 * j:4 * j + 4]:
            a = mesh.pos[t]
            pos[t] = {V0_V1: [a[0], a[0], a[2]], V0_V2: [a[0], a[1], a[0]], V1_V2: [a[0], a[1], a[1]], POINT: [a[1], a[1], a[1]]}[k]
            kind[t] = k
    for t in exact:
        a = mesh.pos[t]
        pos[t] = [a[0], ((a[0].astype(np.float64) + a[1]) / 2).astype(np.float32), a[1]]
        kind[t] = COLLINEAR
    for t, onto in zip(pick[16:26], pick[26:36]):
        pos[t] = mesh.pos[onto]
        kind[t] = DUPLICATE
    return pos, kind


def offset(mesh):
    """The same positions + (4096, -8192, 16384), rounded to fp32: the rounded mesh is the mesh."""
    return mesh._replace(pos=(mesh.pos + OFFSET).astype(np.float32))


def scaled(mesh, k):
    """Positions x 2^k (exact while nothing overflows or goes subnormal)."""
    return mesh._replace(pos=(mesh.pos * np.float32(2.0 ** k)).astype(np.float32))


def streams(mesh):
    return mesh.pos, mesh.nrm, mesh.uv, mesh.mat, ONE_MATERIAL, []


def oracle_scene(mesh):
    """The oracle's scene of a mesh with the (4, 8) tree -- no product library needed."""
    return oracle.Scene(rf.triangles(mesh.pos, mesh.nrm, mesh.uv, mesh.mat), ONE_MATERIAL, []).build_bvh(LEAF, BINS)


def scene_pair(drt, mesh):
    """(product scene, oracle scene), as ray_query_ref.programmatic_scene builds them."""
    return rq.programmatic_scene(drt, *streams(mesh), LEAF, BINS)


def kinds_in_tree_order(osc, mesh):
    """(kind, twin) per triangle of the built scene: the builder reorders triangles, so each is found again by its nine coordinates
    (a duplicate pair has the same nine: both are DUPLICATE-or-SOUP and each other's twin, which is all the tests ask of them)."""
    key = lambda p: [r.tobytes() for r in _f32(p).reshape(len(p), 9)]
    where = {}
    for i, k in enumerate(key(mesh.pos)):
        where.setdefault(k, []).append(i)
    tree = key(osc.tris["p"])
    load = np.array([where[k][0] for k in tree])
    kind = mesh.kind[load]
    pairs = {}
    for i, k in enumerate(tree):
        pairs.setdefault(k, []).append(i)
    twin = np.full(len(tree), -1)
    for idx in pairs.values():
        if len(idx) == 2:
            twin[idx[0]], twin[idx[1]] = idx[1], idx[0]
            kind[idx] = DUPLICATE
    return kind, twin


# ---------------------------------------------------------------- the queries aimed at the thin triangles

def segments(g, kind):
    """(prim, a, b) of the thin triangles of a Geometry: the two vertices that are farthest apart (a point: a = b)."""
    prim = np.nonzero(np.isin(kind, THIN))[0]
    v = np.stack([g.v0[prim], g.v0[prim] + g.e1[prim], g.v0[prim] + g.e2[prim]], axis=1).astype(np.float64)
    d = np.stack([np.linalg.norm(v[:, i] - v[:, j], axis=1) for i, j in ((0, 1), (0, 2), (1, 2))], axis=1)
    far = d.argmax(axis=1)
    i, j = np.array([0, 0, 1])[far], np.array([1, 2, 2])[far]
    m = np.arange(len(prim))
    return prim, v[m, i], v[m, j]


def _unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _extent(g):
    """The size of the soup the mesh is made of (the needles reach 2^4 beyond it): the median edge length times 16."""
    return 16 * float(np.median(np.linalg.norm(g.e1.astype(np.float64), axis=1)))


def _along(rng, a, b, per):
    """`per` points on and beyond each segment: t in {0, 1, 1/2} (the vertices and the midpoint) and random t in [-0.25, 1.25]."""
    t = np.concatenate([np.tile([0.0, 1.0, 0.5], (len(a), 1)), rng.uniform(-0.25, 1.25, (len(a), per - 3))], axis=1)
    return (a[:, None] + (b - a)[:, None] * t[:, :, None]).reshape(-1, 3), np.repeat(np.arange(len(a)), per)


def _twins(twin):
    return np.nonzero((twin >= 0) & (np.arange(len(twin)) < twin))[0]


def aimed_points(g, kind, twin, seed, per=10):
    """Points along and around every thin triangle's segment and exactly at its vertices: the first three of each `per` lie on
    the segment (two vertices, the midpoint), the rest up to 2 % of the extent off it.  Then two points off the centroid of each
    duplicate pair: an exact tie between the two."""
    rng = np.random.default_rng(seed)
    _, a, b = segments(g, kind)
    on, _ = _along(rng, a, b, per)
    off = _unit(rng, len(on)) * rng.uniform(0, 0.02 * _extent(g), (len(on), 1))
    off.reshape(len(a), per, 3)[:, :3] = 0
    t = np.repeat(_twins(twin), 2)
    mid = g.v0[t] + (g.e1[t] + g.e2[t]) / np.float32(3)
    return np.concatenate([on + off, mid + _unit(rng, len(t)) * rng.uniform(0, 0.01 * _extent(g), (len(t), 1))]).astype(np.float32)


def aimed_casts(g, kind, seed, per=9):
    """Sphere casts (org, dirs, radius, tmin, tmax) at the thin triangles: a third aimed at a point of the segment from up to half an
    extent away, a third running along the segment beside it, a third starting within a radius of it (the containment branches)."""
    rng = np.random.default_rng(seed)
    ext = _extent(g)
    _, a, b = segments(g, kind)
    tgt, owner = _along(rng, a, b, per)
    n = len(tgt)
    k = np.arange(n) % 3
    radius = (ext * rng.choice([0.0, 0.005, 0.02], n) * rng.uniform(0.5, 1.0, n))
    away = _unit(rng, n) * rng.uniform(0.05, 0.5, (n, 1)) * ext
    axis = (b - a)[owner]
    axis = np.where((np.abs(axis).max(axis=1) > 0)[:, None], axis, _unit(rng, n) * 0.1 * ext)           # (a point has no axis)
    beside = _unit(rng, n) * (radius * rng.uniform(0.5, 1.5, n) + 1e-4 * ext)[:, None]
    inside = _unit(rng, n) * (radius * rng.uniform(0.0, 0.95, n))[:, None]
    org = np.where((k == 0)[:, None], tgt + away, np.where((k == 1)[:, None], a[owner] - 0.5 * axis + beside, tgt + inside))
    dirs = np.where((k == 0)[:, None], -away * rng.uniform(0.5, 2.0, (n, 1)), np.where((k == 1)[:, None], axis, _unit(rng, n) * 0.2 * ext))
    tmin = np.where(rng.uniform(size=n) < 0.8, 0.0, rng.uniform(0, 0.3, n))
    tmax = np.where(rng.uniform(size=n) < 0.6, np.inf, rng.uniform(0.5, 3.0, n))
    return tuple(_f32(x) for x in (org, dirs, radius, tmin, tmax))


def aimed_rays(g, kind, seed, per=6):
    """Rays (org, dirs, tmin, tmax) through points of the thin triangles' segments and along them."""
    org, dirs, _, tmin, tmax = aimed_casts(g, kind, seed, per)
    return org, dirs, tmin, tmax


def aimed_boxes(g, kind, twin, seed, per=6):
    """Boxes [N, 16]: small ones (half up to 0.2 % of the extent, every third one a point, every other one rotated) centred on
    points of the thin triangles' segments, which touch little else; and boxes about the centroid of each duplicate pair."""
    rng = np.random.default_rng(seed)
    ext = _extent(g)
    _, a, b = segments(g, kind)
    center, _ = _along(rng, a, b, per)
    n = len(center)
    half = rng.uniform(0, 0.002 * ext, (n, 3))
    half[::3] = 0
    rot, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    rot[::2] = np.eye(3)
    t = _twins(twin)
    mid = g.v0[t] + (g.e1[t] + g.e2[t]) / np.float32(3)
    straddle = ov.pack(np.tile(mid, (2, 1)), np.concatenate([np.zeros((len(t), 3)), rng.uniform(0, 0.01 * ext, (len(t), 3))]))
    return np.concatenate([ov.pack(_f32(center), _f32(half), _f32(rot)), straddle]).astype(np.float32)


def aimed_triangle_parts(g, kind, twin, seed, per=6):
    """The three parts of aimed_triangles, each [n, 3, 3] float32: the small triangles around the segments, the thin triangles
    themselves (in the order of segments()), and the triangles through the duplicate pairs' centroids."""
    rng = np.random.default_rng(seed)
    ext = _extent(g)
    prim, a, b = segments(g, kind)
    center, _ = _along(rng, a, b, per)
    size = rng.uniform(0, 0.01 * ext, (len(center), 1, 1))
    q = center[:, None, :] + rng.uniform(-1, 1, (len(center), 3, 3)) * size
    q[::4, 2] = q[::4, 1]
    own = tv.scene_triangles(g)[prim]
    t = _twins(twin)
    mid = (g.v0[t] + (g.e1[t] + g.e2[t]) / np.float32(3)).astype(np.float64)
    across = mid[:, None, :] + rng.uniform(-1, 1, (len(t), 3, 3)) * 0.02 * ext
    across[:, 0] = mid                                             # one vertex in the pair's plane: a touch
    return q.astype(np.float32), own.astype(np.float32), across.astype(np.float32)


def aimed_triangles(g, kind, twin, seed, per=6):
    """Query triangles [N, 3, 3]: small ones (up to 1 % of the extent) around points of the thin triangles' segments, every fourth
    one itself a segment; the thin triangles themselves; and triangles through the centroid of each duplicate pair."""
    return np.concatenate(aimed_triangle_parts(g, kind, twin, seed, per))


def aimed_planes(g, kind, seed):
    """Planes [N, 4]: axis planes through the thin triangles' vertices (s = 0 exactly there), planes that contain their segments
    (n perpendicular to it, d = dot(n, a) in fp32) and planes across them."""
    rng = np.random.default_rng(seed)
    _, a, b = segments(g, kind)
    a32, b32 = _f32(a), _f32(b)
    out = []
    for v in (a32, b32):
        axis = np.eye(3, dtype=np.float32)[rng.integers(0, 3, len(v))] * np.float32(rng.choice([-1, 1], len(v)))[:, None]
        out.append(sr.pack(axis, nr.dot(axis, v)))
    n = _f32(np.cross(b - a, _unit(rng, len(a))))
    out.append(sr.pack(n, nr.dot(n, a32)))
    for _ in range(2):
        n = _f32(_unit(rng, len(a)))
        mid = _f32(a + (b - a) * rng.uniform(0, 1, (len(a), 1)))
        out.append(sr.pack(n, nr.dot(n, mid)))
    return np.concatenate(out).astype(np.float32)


def general_boxes(g, n, rng):
    """About n boxes as test_gpu_overlap.sweep_boxes makes them, without its NaN and infinite ones (every query here scales)."""
    q = max(n // 3, 1)
    lo, hi = nr.bounds(g)
    center = np.concatenate([nr.surface_points(g, q, rng), nr.tie_points(g, q, rng), nr.box_points(g, q, rng)]).astype(np.float32)
    m = len(center)
    half = (rng.uniform(0, 1, (m, 3)) ** 3 * 0.15 * _extent(g)).astype(np.float32)
    half[::7] = 0
    half[3::11, 2] = 0
    rot, _ = np.linalg.qr(rng.normal(size=(m, 3, 3)))
    axes = rot.astype(np.float32)
    axes[::2] = np.eye(3, dtype=np.float32)
    axes[5::16] = (axes[5::16] * rng.uniform(0.5, 2, (len(axes[5::16]), 3, 1)) + 0.1).astype(np.float32)
    return np.concatenate([ov.pack(center, half, axes), ov.pack([(lo + hi) / 2], [hi - lo])]).astype(np.float32)


def general_triangles(g, n, rng):
    """About n query triangles as test_gpu_tri_overlap.sweep_queries makes them, without the invalid ones."""
    k = max(n // 3, 1)
    center = np.concatenate([nr.surface_points(g, k, rng), nr.tie_points(g, k, rng), nr.box_points(g, k, rng)]).astype(np.float32)
    m = len(center)
    size = (rng.uniform(0, 1, (m, 1, 1)) ** 3 * 0.3 * _extent(g)).astype(np.float32)
    q = (center[:, None, :] + rng.uniform(-1, 1, (m, 3, 3)).astype(np.float32) * size).astype(np.float32)
    q[::9, 2] = q[::9, 1]
    q[4::13, 1] = q[4::13, 0]
    q[4::13, 2] = q[4::13, 0]
    own = tv.scene_triangles(g)[rng.choice(len(g.v0), min(max(n // 8, 1), len(g.v0)), replace=False)]
    return np.concatenate([q, own]).astype(np.float32)


def general_planes(g, n, rng):
    """About n planes as test_gpu_section.sweep_planes makes them, without the invalid ones: axis planes through vertices, the
    planes of faces, random ones through the scene (some scaled by 1e-3 and 1e3), n = 0."""
    k = max(n // 4, 2)
    v = nr.tie_points(g, k, rng)
    axis = (np.eye(3, dtype=np.float32)[rng.integers(0, 3, k)] * np.float32(rng.choice([-1, 1], k))[:, None]).astype(np.float32)
    t = rng.integers(0, len(g.v0), k)
    fn = np.cross(g.e1[t], g.e2[t]).astype(np.float32)
    fn = (fn / np.maximum(np.abs(fn).max(axis=1, keepdims=True), np.float32(1e-30))).astype(np.float32)
    nn = rng.normal(size=(2 * k, 3)).astype(np.float32)
    pts = nr.surface_points(g, 2 * k, rng)
    rand = sr.pack(nn, nr.dot(nn, pts))
    rand[::3] *= np.float32(1e-3)
    rand[1::3] *= np.float32(1e3)
    return np.concatenate([sr.pack(axis, nr.dot(axis, v)), sr.pack(fn, nr.dot(fn, g.v0[t])), rand, sr.pack([(0, 0, 0), (-0.0, 0.0, 1)], [0, 0])]).astype(np.float32)


def queries(g, osc, kind, twin, seed, general=400):
    """The aimed queries plus about `general` of each general sweep the existing GPU tests use, without their NaN and infinite
    queries (those tests cover them, and every query here has to scale)."""
    rng = np.random.default_rng(seed)
    points = np.concatenate([aimed_points(g, kind, twin, seed), nr.point_sets(g, general, rng)]).astype(np.float32)
    radius = rng.uniform(0, 0.02 * _extent(g), len(points)).astype(np.float32)
    radius[::9] = 0
    casts = tuple(np.concatenate(p) for p in zip(aimed_casts(g, kind, seed + 2), sw.cast_sets(g, general, rng)))
    o1, d1 = rq.surface_rays(osc, general // 2, rng)
    o2, d2, tmin2, tmax2 = rq.interval_rays(osc, general // 2, rng)
    ok = np.isfinite(tmin2) & np.isfinite(tmax2)
    o3, d3, tmin3, tmax3 = aimed_rays(g, kind, seed + 4)
    rays = (np.concatenate([o1, o2[ok], o3]), np.concatenate([d1, d2[ok], d3]),
            np.concatenate([np.zeros(len(o1), np.float32), tmin2[ok], tmin3]), np.concatenate([np.full(len(o1), np.inf, np.float32), tmax2[ok], tmax3]))
    boxes = np.concatenate([aimed_boxes(g, kind, twin, seed + 5), general_boxes(g, general, rng)])
    tris = np.concatenate([aimed_triangles(g, kind, twin, seed + 7), general_triangles(g, general, rng)])
    planes = np.concatenate([aimed_planes(g, kind, seed + 9), general_planes(g, general, rng)])
    return Queries(points, radius, casts, tuple(_f32(x) for x in rays), boxes, tris, planes)


def scaled_queries(q, k):
    """The queries for scaled(mesh, k): every length x 2^k -- points, radii, origins, cast directions (so every t stays), sphere
    radii, box centres and halves (the axes stay), query triangles and plane d (the normal stays)."""
    s = np.float32(2.0 ** k)
    org, dirs, radius, tmin, tmax = q.casts
    ro, rd, rtmin, rtmax = q.rays
    boxes = q.boxes.copy()
    boxes[:, 0:6] *= s
    planes = q.planes.copy()
    planes[:, 3] *= s
    with np.errstate(over="ignore", under="ignore"):
        return Queries(q.points * s, q.radius * s, (org * s, dirs * s, radius * s, tmin, tmax), (ro * s, rd * s, rtmin, rtmax), boxes, q.tris * s, planes)


# ---------------------------------------------------------------- the restatements' answers, query kind by query kind

K_NEAR = 4
POINT_KINDS = ("nearest", "nearest_r", "k_nearest", "within")
VOLUME_KINDS = ("cast", "boxes", "tris", "planes")
RAY_KINDS = ("crossings", "closest", "occluded", "hits", "votes_parity", "votes_winding")


def restate(g, osc, q, kinds=POINT_KINDS + VOLUME_KINDS + RAY_KINDS):
    """{kind: tuple of arrays}: what each restatement says of the queries, every field of every record and every count."""
    T = max(len(g.v0), 1)
    out = {}
    for kind in kinds:
        if kind == "nearest":
            out[kind] = tuple(nr.nearest(g, q.points))
        elif kind == "nearest_r":
            out[kind] = tuple(nr.nearest(g, q.points, q.radius))
        elif kind == "k_nearest":
            slots, counts = nl.near_list(g, q.points, np.inf, K_NEAR, nl.K)
            out[kind] = tuple(slots) + (counts,)
        elif kind == "within":
            _, totals = nl.near_list(g, q.points, q.radius, 0, nl.GATHER)
            slots, _ = nl.near_list(g, q.points, q.radius, totals, nl.GATHER)
            out[kind] = tuple(slots) + (totals,)
        elif kind == "cast":
            out[kind] = tuple(sw.sphere_cast(g, *q.casts))
        elif kind == "boxes":
            _, totals = ov.overlap(g, q.boxes, 0)
            out[kind] = (ov.overlap(g, q.boxes, totals)[0], totals)
        elif kind == "tris":
            _, totals = tv.overlap(g, q.tris, 0)
            out[kind] = (tv.overlap(g, q.tris, totals)[0], totals)
        elif kind == "planes":
            rec, totals = sr.whole(g, q.planes)
            out[kind] = (rec["p"].copy(), rec["prim"].copy(), rec["q"].copy(), rec["code"].copy(), totals)
        elif kind == "crossings":
            out[kind] = tuple(ir.crossings(osc, *q.rays))
        elif kind == "closest":
            out[kind] = tuple(rq.closest(osc, *q.rays))
        elif kind == "occluded":
            out[kind] = (rq.occluded(osc, *q.rays),)
        elif kind == "hits":
            rec = hr.records(osc, *q.rays)
            totals = hr.ranks(len(q.rays[0]), rec)[2]
            out[kind] = tuple(hr.list_hits(osc, *q.rays, totals, rec)[0]) + (totals,)
        else:
            out[kind] = (ir.votes(osc, q.points, kind[len("votes_"):]),)
    return out


# which power of the scale each field of restate()'s tuples carries (None: an index, a count, a parameter: unchanged)
POWERS = {"nearest": (1, 2, None, None, None, None), "nearest_r": (1, 2, None, None, None, None),
          "k_nearest": (2, None, None, None, 1, None, None), "within": (2, None, None, None, 1, None, None),
          "cast": (None, None, None, None, 1, None), "boxes": (None, None), "tris": (None, None), "planes": (1, None, 1, None, None),
          "crossings": (None, None), "closest": (None, None, None, None), "occluded": (None,), "hits": (None, None, None, None, None),
          "votes_parity": (None,), "votes_winding": (None,)}


def rescale(kind, answer, k):
    """The answer of the plain mesh as the answer of scaled(mesh, k) would read if scaling changed nothing."""
    with np.errstate(over="ignore", under="ignore"):
        return tuple(a if p is None else (a * np.float32(2.0 ** k) if p == 1 else a * np.float32(2.0 ** k) * np.float32(2.0 ** k)).astype(np.float32)
                     for a, p in zip(answer, POWERS[kind]))


def differing(a, b):
    """The number of entries (rows) in which two answers differ, bit for bit (a NaN equals any NaN; lists of different length: -1)."""
    bad = 0
    for x, y in zip(a, b):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if x.shape != y.shape:
            return -1
        if len(x) == 0:
            continue
        bits = np.uint8 if x.itemsize == 1 else np.uint32
        d = x.view(bits) != y.view(bits)
        if x.dtype == np.float32:
            d &= ~(np.isnan(x) & np.isnan(y))
        bad += int(d.reshape(len(x), -1).any(axis=1).sum())
    return bad


# ---------------------------------------------------------------- hand scenes: answers derived on paper

# A segment (v1 = v2): e1 = e2 = (2, 0, 0).  A point: e1 = e2 = 0.  A v0 = v1 triangle (e1 = 0) beside the unit right triangle.
HAND_SEGMENT = np.float32([[[0, 0, 0], [2, 0, 0], [2, 0, 0]]])
HAND_POINT = np.float32([[[1, 1, 0], [1, 1, 0], [1, 1, 0]]])
HAND_BESIDE = np.float32([[[0, 0, 1], [0, 0, 1], [2, 0, 1]], [[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
DOWN = (0, 0, -1)

# (scene, point, u, v, closest point, d2) -- side is +1 everywhere (a zero-area triangle has no normal: dot(p - c, fn) < 0 is false).
#   segment, (1, 0, 1): ap = (1, 0, 1), d1 = d2 = 2; bp = cp = (-1, 0, 1), d3 = d4 = d5 = d6 = -2; vc = vb = va = 0.  Cases 1 and 2
#     fail (d1 > 0, d3 < 0); case 3 matches (vc <= 0, d1 >= 0, d3 <= 0) with a quotient: u = 2 / (2 + 2).
#   segment, (-1, 0, 0): d1 = d2 = -2: case 1, v0.          segment, (3, 1, 0): bp = (1, 1, 0), d3 = d4 = 2: case 2, v1.
#   point: e1 = e2 = 0, d1 = d2 = 0: case 1, always.
#   beside, (0.25, 0.25, 0.875): on the v0 = v1 triangle case 3 divides 0 by 0 (tests/test_nearest_ref.py); the proper triangle below
#     wins with its face, 0.875^2.                          beside, (-1, 0, 1): e1 = 0, d1 = 0, d2 = -2: case 1 of the v0 = v1 triangle,
#     its v0 at distance 1; the proper triangle's v0 is at distance sqrt(2).
HAND_NEAREST = [("segment", (1, 0, 1), 0.5, 0, (1, 0, 0), 1), ("segment", (-1, 0, 0), 0, 0, (0, 0, 0), 1), ("segment", (3, 1, 0), 1, 0, (2, 0, 0), 2),
                ("point", (1, 1, 2), 0, 0, (1, 1, 0), 4), ("beside", (0.25, 0.25, 0.875), 0.25, 0.25, (0.25, 0.25, 0), 0.765625),
                ("beside", (-1, 0, 1), 0, 0, (0, 0, 1), 1)]
# which triangle of the scene answers: by its stored e1 (the builder may reorder the two)
HAND_NEAREST_ZERO_AREA = [True, True, True, True, False, True]

# (scene, origin, direction, radius, t, feature, u, v, point); a miss: t = inf, feature -1.
#   segment, from (1, 0, 1): no face (den = 16 - 16 = 0).  Edge 1: m = (1, 0, 1), me = 2, de = 0, Cq = 4 * 1.9375 - 4 = 3.75,
#     x = cross(d, e) = (0, -2, 0), det = 0, A = 4, B = -4, disc = 4 (4 / 16) = 1, tau = 3.75 / 5; ax = 2 in [0, 4].  Edge 2 is the same
#     edge and no strict <; edge 3 has ee = 0; both vertex spheres are passed at distance 1 > r.
#   segment, the (3, 4, 12) / 16 offsets of tests/sweep_ref.py's HAND beyond either end: the cylinder is entered first, but with
#     ax = me < 0 or > ee; the vertex sphere gives c = 2.5, b = -1.75, disc = 0.5625, tau = 2.5 / 2.5.  At the far end p1 = p2, and
#     feature 5 comes before 6.
#   segment, from (1, 0, 0.125): Cq = 4 * 0.953125 - 4 < 0, edge 1's containment branch: feature 1 + 8, t = tmin.
#   point: the three vertex spheres coincide, feature 4 is first; 0.5 beside it with r = 0.25 is a miss.
#   beside, from (1, 0, 2): the v0 = v1 triangle's e1 has ee = 0, its segment is edge 2 (tests/test_sweep_ref.py), above the proper one.
HAND_CASTS = [("segment", (1, 0, 1), DOWN, 0.25, 0.75, 1, 0.5, 0, (1, 0, 0)), ("segment", (-0.1875, -0.25, 1.75), DOWN, 0.8125, 1.0, 4, 0, 0, (0, 0, 0)),
              ("segment", (2.1875, 0.25, 1.75), DOWN, 0.8125, 1.0, 5, 1, 0, (2, 0, 0)), ("segment", (1, 0, 0.125), DOWN, 0.25, 0.0, 9, 0.5, 0, (1, 0, 0)),
              ("point", (1, 1, 1), DOWN, 0.25, 0.75, 4, 0, 0, (1, 1, 0)), ("point", (1.5, 1, 1), DOWN, 0.25, np.inf, -1, 0, 0, (0, 0, 0)),
              ("beside", (1, 0, 2), DOWN, 0.25, 0.75, 2, 0, 0.5, (1, 0, 1))]

# (scene, centre, half (all three), listed).  Axis-aligned boxes: every product is exact.
#   segment: p0 = -1, p1 = p2 = +1 about (1, 0, 0): every axis holds; the plane and the zero cross axes pass with 0 <= 0.  Half a unit
#     beside it the y axis separates (max3 = -0.5 < -0.125).  Centre (3, 0, 0), half 0.5: max3(p.x) = -1 < -0.5.  Centre (2.5, 0, 0):
#     max3 = -0.5 >= -0.5, touching counts.
#   point: a box of half 0 at the point lists it (0 <= 0 on every axis); at (1.25, 1, 0) with half 0.125, p.x = -0.25 < -0.125.
HAND_BOXES = [("segment", (1, 0, 0), 0.125, True), ("segment", (1, 0.5, 0), 0.125, False), ("segment", (3, 0, 0), 0.5, False),
              ("segment", (2.5, 0, 0), 0.5, True), ("point", (1, 1, 0), 0.0, True), ("point", (1.25, 1, 0), 0.125, False)]

# (scene, query triangle, listed).
#   segment: the triangle in the plane x = 1 around (1, 0, 0) is crossed by the segment: the predicate never misses.  The same triangle
#     at x = 3: nq = (4, 0, 0), sq = 0, st = (-12, -4, -4): max3(st) < min3(sq).
#   point: (1, 1, 0) lies on the hypotenuse of the triangle with legs 2: a touch; axis cross(nq, g) = (-8, -8, 0) has sq = (0, -16, -16) and
#     st = -16, equal ends.  With legs 1, cross(nq, g) = (-1, -1, 0): sq = (0, -1, -1), st = -2 < -1.
HAND_TRIS = [("segment", [(1, -1, -1), (1, 1, -1), (1, 0, 1)], True), ("segment", [(3, -1, -1), (3, 1, -1), (3, 0, 1)], False),
             ("point", [(0, 0, 0), (2, 0, 0), (0, 2, 0)], True), ("point", [(0, 0, 0), (1, 0, 0), (0, 1, 0)], False)]

# (scene, n, d, [(p, q, code, zero-area)] in any order).
#   segment, x = 1: s = (-1, 1, 1), the apex v0 is below: Q -> P, both cut(0, .) = v0 + (2, 0, 0) * (-1 / -2): a zero-length segment, code 0.
#   segment, x = 2: s = (-2, 0, 0), 0 is above: t = -2 / (-2 - 0) = 1, the point is v1.  x = 0 and y = 0: nothing is below, no cut.
#   point: its three vertices are always in one class.
#   beside, x = 0.5: the proper triangle has v1 alone above, P = cut(1, 2) = (0.5, 0.5, 0), Q = cut(1, 0) = (0.5, 0, 0), P -> Q, code 1 + 4;
#     the v0 = v1 triangle has v2 alone above, t = -0.5 / -2, P = Q = (0.5, 0, 1), code 2 + 4.
HAND_PLANES = [("segment", (1, 0, 0), 1, [((1, 0, 0), (1, 0, 0), 0, True)]), ("segment", (1, 0, 0), 2, [((2, 0, 0), (2, 0, 0), 0, True)]),
               ("segment", (1, 0, 0), 0, []), ("segment", (0, 1, 0), 0, []), ("point", (0, 0, 1), 0, []), ("point", (1, 0, 0), 1, []),
               ("point", (1, 0, 0), 1.5, []),
               ("beside", (1, 0, 0), 0.5, [((0.5, 0.5, 0), (0.5, 0, 0), 5, False), ((0.5, 0, 1), (0.5, 0, 1), 6, True)])]
HAND_SCENES = {"segment": HAND_SEGMENT, "point": HAND_POINT, "beside": HAND_BESIDE}


def check_hand_cases(geometry, run):
    """The paper values above against run(name, scene, Geometry, kind of query, query arrays...) -> the answer in the restatements'
    form.  geometry(name) gives (scene handle or None, Geometry) of a hand scene."""
    zero = lambda g, prim: ~(g.e1[prim] != 0).any(axis=1) | ~(g.e2[prim] != 0).any(axis=1) | (g.e1[prim] == g.e2[prim]).all(axis=1)
    for name in HAND_SCENES:
        sc, g = geometry(name)
        rows = [h for h in HAND_NEAREST if h[0] == name]
        res = run("nearest", sc, g, np.float32([h[1] for h in rows]))
        assert (res.prim >= 0).all() and res.u.tolist() == [h[2] for h in rows] and res.v.tolist() == [h[3] for h in rows], (name, res)
        assert res.point.tolist() == [list(map(float, h[4])) for h in rows] and res.d2.tolist() == [h[5] for h in rows] and (res.side == 1).all(), (name, res)
        assert zero(g, res.prim).tolist() == [z for h, z in zip(HAND_NEAREST, HAND_NEAREST_ZERO_AREA) if h[0] == name]
        rows = [h for h in HAND_CASTS if h[0] == name]
        res = run("cast", sc, g, np.float32([h[1] for h in rows]), np.float32([h[2] for h in rows]), np.float32([h[3] for h in rows]))
        assert res.t.tolist() == [h[4] for h in rows] and res.feature.tolist() == [h[5] for h in rows], (name, res)
        assert res.u.tolist() == [h[6] for h in rows] and res.v.tolist() == [h[7] for h in rows], (name, res)
        assert res.point.tolist() == [list(map(float, h[8])) for h in rows] and ((res.prim >= 0) == (res.feature >= 0)).all(), (name, res)
        assert zero(g, res.prim[res.prim >= 0]).all()
        rows = [h for h in HAND_BOXES if h[0] == name]
        if rows:
            counts = run("boxes", sc, g, ov.pack([h[1] for h in rows], [[h[2]] * 3 for h in rows]))
            assert (counts > 0).tolist() == [h[3] for h in rows], (name, counts)
        rows = [h for h in HAND_TRIS if h[0] == name]
        if rows:
            counts = run("tris", sc, g, np.float32([h[1] for h in rows]))
            assert (counts > 0).tolist() == [h[2] for h in rows], (name, counts)
        rows = [h for h in HAND_PLANES if h[0] == name]
        rec, counts = run("planes", sc, g, sr.pack([h[1] for h in rows], [h[2] for h in rows]))
        assert counts.tolist() == [len(h[3]) for h in rows], (name, counts)
        start = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
        for i, h in enumerate(rows):
            got = sorted((r["p"].tolist(), r["q"].tolist(), int(r["code"]), bool(zero(g, np.array([r["prim"]]))[0])) for r in rec[start[i]:start[i + 1]])
            assert got == sorted((list(map(float, p)), list(map(float, q)), c, z) for p, q, c, z in h[3]), (name, h, got)
