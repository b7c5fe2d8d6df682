"""The four newest mesh queries -- triangle distance, triangle casts, surface lookups with area-weighted sampling, ambient occlusion --
aimed at the meshes of tests/hostile_meshes.py, for tests/test_hostile_queries_ref.py (CPU) and tests/test_gpu_hostile_queries.py.  No
tests of its own.

A sibling of tests/hostile_meshes.py: hm.Queries and hm.queries' generator are left alone (tests/test_gpu_hostile_meshes.py compares
those arrays byte for byte); TriQueries is a second tuple, built by tri_queries with generators of its own, restate is a second
restatement table, POWERS and scaled_tri_queries are the second scaling tables.

The mesh streams: the degenerate mesh already has random vertex normals on its added triangles; with_uvs gives a VARIANT mesh random
uvs in [-2, 3] as well (positions, normals and order unchanged, so the tree, the kinds and every answer of the older queries are the
same), and the scenes of the existing tests stay byte-identical.
"""
import collections

import numpy as np

from tests import ambient_ref as ar
from tests import hostile_meshes as hm
from tests import nearest_ref as nr
from tests import surface_ref as sr
from tests import tri_cast_ref as tc
from tests import tri_distance_ref as td
from tests import tri_overlap_ref as tv

F = np.float32
N_SAMPLES = 5140
SAMPLE_SEED = 29
AO_SEED = 2024
AO_SAMPLES = (16, 7, 65)            # a packed tile, idle lanes, several tiles per point with a partial last one
BIG_BIAS = 0.0625                   # 32 ulps of a coordinate of 16384 (2^-9); 0.001 is half of one

# tris [N, 3, 3], max_dist [N]; cast_tris [C, 3, 3], dirs [C, 3], tmax [C]; mesh_dir [3]; refs = (prim, u, v) [R] (the samples are the
# mesh's own and come from restate); ao = (points [A, 3], normals [A, 3], max_dist [A], bias [A]); flat = (tris, max_dist, cast_tris,
# dirs, tmax) of the zero-area QUERY triangles, a batch of their own (zero_area_queries)
TriQueries = collections.namedtuple("TriQueries", "tris max_dist cast_tris dirs tmax mesh_dir refs ao flat")


def _f32(a):
    return np.ascontiguousarray(a, F)


def with_uvs(mesh, seed=17):
    """The same mesh with random vertex uvs in [-2, 3]."""
    rng = np.random.default_rng(seed)
    return mesh._replace(uv=rng.uniform(-2, 3, mesh.uv.shape).astype(F))


def aimed_tri_casts(g, kind, twin, seed, per=12):
    """Triangle casts (tris, dirs, tmax) at the thin triangles: small triangles (up to 1 % of the extent) held up to a quarter of an
    extent off a point of each thin triangle's segment.  Of every eight, five move at that point (it is reached at t in [0.5, 1.25]),
    one starts beside the segment and moves along it, one moves away from it and one does not move at all (d = 0).  Then the thin
    triangles themselves (opened where they have no area: see proper) held off and moving back onto their own place, and triangles
    through the centroid of each duplicate pair moving at it: the same t on both triangles of the pair."""
    rng = np.random.default_rng(seed)
    ext = hm._extent(g)
    prim, a, b = hm.segments(g, kind)
    tgt, owner = hm._along(rng, a, b, per)
    n = len(tgt)
    k = np.array([0, 0, 1, 0, 0, 2, 0, 3])[np.arange(n) % 8]
    shape = rng.uniform(-1, 1, (n, 3, 3)) * rng.uniform(0, 0.01 * ext, (n, 1, 1))
    away = hm._unit(rng, n) * rng.uniform(0.02, 0.25, (n, 1)) * ext
    axis = (b - a)[owner]
    axis = np.where((np.abs(axis).max(axis=1) > 0)[:, None], axis, hm._unit(rng, n) * 0.1 * ext)           # (a point has no axis)
    beside = hm._unit(rng, n) * (rng.uniform(0, 0.01, n) * ext)[:, None]
    start = np.where((k == 0)[:, None], tgt + away, np.where((k == 1)[:, None], a[owner] - 0.5 * axis + beside, tgt + 0.1 * away))
    dirs = np.where((k == 0)[:, None], -away * rng.uniform(0.8, 2.0, (n, 1)), np.where((k == 1)[:, None], axis, np.where((k == 2)[:, None], away, 0.0)))
    tris = start[:, None, :] + shape
    own = tv.scene_triangles(g)[prim].astype(np.float64)
    off = hm._unit(rng, len(own)) * rng.uniform(0.05, 0.3, (len(own), 1)) * ext
    t = hm._twins(twin)
    mid = (g.v0[t] + (g.e1[t] + g.e2[t]) / F(3)).astype(np.float64)
    across = rng.uniform(-1, 1, (len(t), 3, 3)) * 0.02 * ext
    across[:, 0] = 0                                                # one vertex arrives at the centroid itself
    back = hm._unit(rng, len(t)) * 0.2 * ext
    tris = np.concatenate([tris, own + off[:, None, :], mid[:, None, :] + across + back[:, None, :]])
    dirs = np.concatenate([dirs, -off * rng.uniform(0.5, 2.0, (len(off), 1)), -back * rng.uniform(0.5, 2.0, (len(t), 1))])
    tmax = np.where(rng.uniform(size=len(tris)) < 0.5, 1.0, rng.uniform(0.3, 2.5, len(tris)))
    return proper(tris, rng, 0.005 * ext), _f32(dirs), _f32(tmax)


def proper(tris, rng, size):
    """The triangles with every zero-area one (equal vertices, or collinear to the last bit) opened: its vertices 1 and 2 move by up
    to `size`.  The overlap predicate passes a segment or point query against a POINT of the scene wherever it is (include/drt.h), so
    such a query's answer over all triangles is d2 = 0 or t = 0 whatever the tree culls: tests/test_hostile_queries_ref.py pins that
    on queries of its own, and the four features' own GPU tests send zero-area queries."""
    tris = np.array(tris, np.float64)
    flat = ~(np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]) != 0).any(axis=1)       # (exact in float64 for these collinear ones)
    move = rng.uniform(-1, 1, (len(tris), 2, 3)) * size
    tris[flat, 1:] += move[flat]
    return tris.astype(F)


def is_flat(tris):
    """Which triangles [N, 3, 3] have exactly zero area: cross(e1, e2) = 0 in float64 (exact for float32 vertices of these sizes)."""
    t = np.asarray(tris, np.float64)
    return ~(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]) != 0).any(axis=1)


def zero_area_queries(g, kind, twin, seed, general=120):
    """(tris, max_dist, cast_tris, dirs, tmax): the zero-area query triangles that tri_queries opens or leaves out, unopened -- every
    fourth of hm.aimed_triangles' small triangles (a segment through a point of a thin triangle's segment), the segments and points
    of hm.general_triangles, and the mesh's own zero-area triangles, in place and up to 2 % of the extent off it.  Here the pair rule
    meets a = 0 and e = 0 together, 0 / 0 and NaNs on both sides.  The casts: the aimed segments and the mesh's zero-area triangles held
    off and moving back at their place (t in [0.5, 1.25]), the general ones moving at random; every ninth does not move."""
    rng = np.random.default_rng(seed)
    ext = hm._extent(g)
    around, own, _ = hm.aimed_triangle_parts(g, kind, twin, seed - 5)          # (tri_queries' own aimed triangles: seed + 101)
    segs = around[::4]
    gen = hm.general_triangles(g, general, rng)
    gen = gen[is_flat(gen)]
    own = own[is_flat(own)]
    assert is_flat(segs).all() and len(gen) >= 10 and len(own) >= 15
    near = (own.astype(np.float64) + (hm._unit(rng, len(own)) * rng.uniform(0, 0.02, (len(own), 1)) * ext)[:, None, :]).astype(F)
    tris = np.concatenate([segs, gen, near, own]).astype(F)
    max_dist = (rng.uniform(0, 1, len(tris)) ** 2 * 0.05 * ext).astype(F)
    max_dist[::7] = 0
    max_dist[5::11] = np.inf
    held = np.concatenate([segs, own]).astype(np.float64)
    away = hm._unit(rng, len(held)) * rng.uniform(0.02, 0.25, (len(held), 1)) * ext
    cast_tris = np.concatenate([(held + away[:, None, :]).astype(F), gen])
    dirs = np.concatenate([-away * rng.uniform(0.8, 2.0, (len(held), 1)), hm._unit(rng, len(gen)) * rng.uniform(0, 1, (len(gen), 1)) * ext]).astype(F)
    dirs[::9] = 0
    tmax = np.where(rng.uniform(size=len(cast_tris)) < 0.5, 1.0, rng.uniform(0.3, 2.5, len(cast_tris))).astype(F)
    # (moved and rounded, a collinear triple is a sliver: all the others still have exactly zero area)
    return tris, max_dist, cast_tris, dirs, tmax


def thin_refs(kind):
    """(prim, u, v): two references on every thin triangle, (1/4, 1/4) and (1/2, 0)."""
    prim = np.repeat(np.nonzero(np.isin(kind, hm.THIN))[0], 2).astype(np.int32)
    u = np.tile(F([0.25, 0.5]), len(prim) // 2)
    v = np.tile(F([0.25, 0.0]), len(prim) // 2)
    return prim, u, v


def tri_queries(g, s, kind, twin, seed, general=200):
    """The queries of the four families for a mesh (g: nearest_ref.Geometry, s: surface_ref.SurfaceScene of the same scene): the
    triangles of hm.aimed_triangles and about `general` general ones with a max_dist each (every seventh 0, some infinite); the aimed
    casts and about `general` general ones with a tmax each (every thirteenth general one with d = 0) and one direction for the mesh
    cast; the references of the nearest answers of hm.aimed_points and sr.hostile_refs; and ambient points -- the lookup's position and
    stored face normal at 60 samples of the mesh and at two references on every thin triangle, with bias 0, 0.001 and BIG_BIAS in turn
    and a finite max_dist on every third."""
    rng = np.random.default_rng(seed + 100)
    ext = hm._extent(g)
    around, own, across = hm.aimed_triangle_parts(g, kind, twin, seed + 101)      # (the thin triangles themselves stay as they are)
    tris = np.concatenate([proper(around, rng, 0.005 * ext), own, across, proper(hm.general_triangles(g, general, rng), rng, 0.005 * ext)]).astype(F)
    max_dist = (rng.uniform(0, 1, len(tris)) ** 2 * 0.05 * ext).astype(F)
    max_dist[::7] = 0
    max_dist[5::11] = np.inf
    at, ad, atmax = aimed_tri_casts(g, kind, twin, seed + 102)
    gt = proper(hm.general_triangles(g, general, rng), rng, 0.005 * ext)
    gd = (hm._unit(rng, len(gt)) * rng.uniform(0, 1, (len(gt), 1)) * ext).astype(F)
    gtmax = np.where(rng.uniform(size=len(gt)) < 0.5, 1.0, rng.uniform(0.1, 2.0, len(gt))).astype(F)
    gd[::13] = 0
    mesh_dir = _f32(hm._unit(rng, 1)[0] * 0.25 * ext)
    near = nr.nearest(g, hm.aimed_points(g, kind, twin, seed + 103))
    hp, hu, hv = sr.hostile_refs(len(g.v0), 300, seed + 104)
    refs = (np.concatenate([near.prim.astype(np.int32), hp]), np.concatenate([near.u, hu]).astype(F), np.concatenate([near.v, hv]).astype(F))
    # ambient points: the lookup's position and stored face normal at samples of the mesh and on every thin triangle
    smp = sr.sample(s, seed + 105, 0, 60)
    tp, tu, tw = thin_refs(kind)
    ap, au, av = np.concatenate([smp.view(np.int32)[:, 1], tp]), np.concatenate([smp[:, 2], tu]), np.concatenate([smp[:, 3], tw])
    rec = sr.lookup(s, ap, au, av).view(F)
    m = len(ap)
    bias = np.tile(F([0, 0.001, BIG_BIAS]), m // 3 + 1)[:m]
    reach = np.where(np.arange(m) % 3 == 1, rng.uniform(0.02, 0.3, m) * ext, np.inf).astype(F)
    ao = (_f32(rec[:, sr.POSITION]), _f32(rec[:, sr.NORMAL]), reach, bias)
    return TriQueries(tris, max_dist, np.concatenate([at, gt]), np.concatenate([ad, gd]).astype(F), np.concatenate([atmax, gtmax]), mesh_dir, refs, ao,
                      zero_area_queries(g, kind, twin, seed + 106))


def scaled_tri_queries(q, k):
    """The queries for hm.scaled(mesh, k).  The power of each field is the header's: query triangles, max_dist, the cast's d (so that
    every t and tmax stay) and the ambient point, max_dist and bias are lengths; (prim, u, v), tmax and the ambient normal stay."""
    s = F(2.0 ** k)
    p, n, reach, bias = q.ao
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        ft, fm, fc, fd, ftmax = q.flat
        return TriQueries(q.tris * s, q.max_dist * s, q.cast_tris * s, q.dirs * s, q.tmax, q.mesh_dir * s, q.refs, (p * s, n, reach * s, bias * s),
                          (ft * s, fm * s, fc * s, fd * s, ftmax))


# ---------------------------------------------------------------- the restatements' answers

DISTANCE_KINDS = ("distance", "distance_md", "within", "mesh_distance")
CAST_KINDS = ("tcast", "casts_any", "mesh_cast")
SURFACE_KINDS = ("weights", "samples", "samples_top", "lookup")
AMBIENT_KINDS = tuple("ambient_%d" % n for n in AO_SAMPLES)
FLAT_KINDS = tuple("flat_" + kind for kind in DISTANCE_KINDS + CAST_KINDS)           # the same queries on TriQueries.flat
KINDS = DISTANCE_KINDS + CAST_KINDS + SURFACE_KINDS + AMBIENT_KINDS + FLAT_KINDS


def flat_view(q):
    """The queries with the zero-area batch in the place of the proper triangles and casts."""
    ft, fm, fc, fd, ftmax = q.flat
    return q._replace(tris=ft, max_dist=fm, cast_tris=fc, dirs=fd, tmax=ftmax)


def mesh_reduce(key, hit, fields, miss):
    """Renderer.meshDistance / meshCast: of the hits the smallest key, of equal keys the smallest query index; (key, query, fields...)."""
    least = hit & (key == np.where(hit, key, np.inf).min(initial=np.inf))
    if not least.any():
        return (np.array(np.inf, F), np.array(-1, np.int32)) + miss
    i = int(np.nonzero(least)[0][0])
    return (np.array(key[i], F), np.array(i, np.int32)) + tuple(np.array(f[i]) for f in fields)


def surface_fields(rec):
    """Records uint32 [N, 24] as a tuple: position, normal, shading, uv, albedo, emissive, (alpha, roughness, refractive index) and the
    integer words (material, load index, texture, flags)."""
    rec = np.ascontiguousarray(rec).view(np.uint32).reshape(-1, 24)
    f = rec.view(F)
    return (_f32(f[:, sr.POSITION]), _f32(f[:, sr.NORMAL]), _f32(f[:, sr.SHADING]), _f32(f[:, sr.UV]), _f32(f[:, sr.ALBEDO]), _f32(f[:, sr.EMISSIVE]),
            _f32(f[:, [sr.ALPHA, sr.ROUGHNESS, sr.REFRACTIVE_INDEX]]), np.ascontiguousarray(rec[:, [sr.MATERIAL, sr.LOAD_INDEX, sr.TEXTURE, sr.FLAGS]]))


def sample_refs(smp):
    """(prim, u, v) of sample records float32 [n, 4]."""
    return smp.view(np.int32)[:, 1].copy(), smp[:, 2].copy(), smp[:, 3].copy()


def all_refs(q, smp):
    """The three kinds of references in one batch: the nearest answers and the hostile ones of the queries, then the samples."""
    return tuple(np.concatenate([a, b]) for a, b in zip(q.refs, sample_refs(smp)))


def restate(g, osc, s, q, kinds=KINDS):
    """{kind: tuple of arrays}: what each restatement says of the queries, every field of every record."""
    out = {}
    cdf = None
    for kind in kinds:
        if kind.startswith("flat_"):
            out[kind] = restate(g, osc, s, flat_view(q), (kind[len("flat_"):],))[kind[len("flat_"):]]
        elif kind == "distance":
            out[kind] = tuple(td.distance(g, q.tris))
        elif kind == "distance_md":
            out[kind] = tuple(td.distance(g, q.tris, q.max_dist))
        elif kind == "within":
            out[kind] = (td.distance(g, q.tris, q.max_dist, td.ANY).prim >= 0,)
        elif kind == "mesh_distance":
            r = out["distance"] if "distance" in out else tuple(td.distance(g, q.tris))
            r = td.TriNear(*r)
            out[kind] = mesh_reduce(r.d2, r.prim >= 0, (r.prim, r.point_q, r.point_t, r.feature), (np.array(-1, np.int32), np.zeros(3, F), np.zeros(3, F), np.array(0, np.int32)))
        elif kind == "tcast":
            out[kind] = tuple(tc.cast(g, q.cast_tris, q.dirs, q.tmax))
        elif kind == "casts_any":
            out[kind] = (tc.cast(g, q.cast_tris, q.dirs, q.tmax, tc.ANY).prim >= 0,)
        elif kind == "mesh_cast":
            r = tc.cast(g, q.cast_tris, q.mesh_dir, q.tmax)
            out[kind] = mesh_reduce(r.t, r.prim >= 0, (r.prim, r.point, r.normal, r.feature), (np.array(-1, np.int32), np.zeros(3, F), np.zeros(3, F), np.array(-1, np.int32)))
        elif kind in SURFACE_KINDS:
            cdf = sr.weights(s) if cdf is None else cdf
            if kind == "weights":
                out[kind] = (np.array(cdf, np.uint64).view(np.uint32).reshape(-1, 2),)
            elif kind == "samples":
                out[kind] = sample_refs(sr.sample(s, SAMPLE_SEED, 0, N_SAMPLES, cdf))
            elif kind == "samples_top":
                out[kind] = sample_refs(sr.sample(s, SAMPLE_SEED, 2 ** 32 - N_SAMPLES, N_SAMPLES, cdf))
            else:
                out[kind] = surface_fields(sr.lookup(s, *all_refs(q, sr.sample(s, SAMPLE_SEED, 0, N_SAMPLES, cdf))))
        else:
            out[kind] = (ar.ambient(osc, *q.ao, int(kind[len("ambient_"):]), AO_SEED),)
    return out


# which power of the scale each field of restate()'s tuples carries (None: an index, a count, a parameter, t, u, v: unchanged).  The
# cast's normal is a cross product of two edges, not normalised: a second power.  Weights are relative to the largest area; the ambient
# record counts samples and sums unit directions.
POWERS = {"distance": (1, 2, 1, None, None, None, None), "distance_md": (1, 2, 1, None, None, None, None), "within": (None,),
          "mesh_distance": (2, None, None, 1, 1, None), "tcast": (1, None, 2, None, None, None, None), "casts_any": (None,),
          "mesh_cast": (None, None, None, 1, 2, None), "weights": (None,), "samples": (None, None, None), "samples_top": (None, None, None),
          "lookup": (1, None, None, None, None, None, None, None)}
POWERS.update({kind: (None,) for kind in AMBIENT_KINDS})
POWERS.update({kind: POWERS[kind[len("flat_"):]] for kind in FLAT_KINDS})


def rescale(kind, answer, k):
    """The answer of the plain mesh as the answer of hm.scaled(mesh, k) would read if scaling changed nothing."""
    s = F(2.0 ** k)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return tuple(a if p is None else (a * s if p == 1 else a * s * s).astype(F) for a, p in zip(answer, POWERS[kind]))


def differing(a, b):
    """hm.differing, for tuples that also hold 0-dimensional arrays and booleans."""
    prep = lambda x: np.atleast_1d(np.asarray(x).astype(np.uint8) if np.asarray(x).dtype == bool else np.asarray(x))
    return hm.differing([prep(x) for x in a], [prep(y) for y in b])


# ---------------------------------------------------------------- hand scenes: answers derived on paper (hm.HAND_SCENES)

DOWN2, DOWN4, UP2 = (0, 0, -2), (0, 0, -4), (0, 0, 2)
Q_X1 = [(1, -1, 1), (1, 1, 1), (1, 0, 2)]                 # in the plane x = 1, its lowest edge q0 q1 at z = 1 crosses above y = 0
Q_Z2 = [(0, 0, 2), (4, 0, 2), (0, 4, 2)]                  # in the plane z = 2, legs 4: (1, 1, 2) is inside
Q_X05 = [(0.5, -1, 2), (0.5, 1, 2), (0.5, 0, 3)]          # in the plane x = 0.5, its lowest edge at z = 2
Q_UNDER = [(0.25, 0.25, -1), (0.5, 0.25, -1), (0.25, 0.5, -1)]

# (scene, query triangle, d2, feature, u, v, point_q, point_t, the winner has zero area).  Candidates relative to q0, in the header's order.
#   segment, Q_X1: the query's vertices are sqrt(2), sqrt(2), 2 from the segment (or a NaN, 0 / 0 in a case of the point-triangle rule,
#     which never wins); the scene's vertices see (1, 0, 1) of the query at sqrt(2).  Edge pair 6 (query edge q0 q1, scene edge v0 + e1 t):
#     r = P1 - P2 = (1, -1, 1), a = e = 4, b = 0, f = 2, c = -2, den = 16 > 0, s = (0 + 8) / 16 = 0.5, t = (0 + 2) / 4 = 0.5, the points
#     (1, 0, 1) and (1, 0, 0), dist2 = 1 < 2.  Pairs 7 (h = e2 - e1 = 0) and 8 (the same edge backwards) give 1 as well and are later.
#     No touch: the axis cross(e1, a1) = (0, 0, 4) has the query at z in [1, 2] and the segment at 0.
#   point, Q_Z2: case 1 of the point-triangle rule gives the query's vertices 6, 14, 14.  Candidate 3, the scene's v0 against the
#     query's face: (1, 1, -2) relative to q0, inside, va + vb + vc = |cross(a1, a2)|^2 = 256 and every product an integer: the point
#     (1, 1, 2), dist2 = 4.  4 and 5 are the same vertex; an edge of the query is sqrt(5) away.
#   beside, Q_X05: the v0 = v1 triangle is the segment (0, 0, 1) - (2, 0, 1).  Pair 6 meets its edge 0, the point v0 (e = 0, t = 0):
#     the query's (0.5, 0, 2) is 0.25 + 1 from it.  Pair 7, edge 1 = v1 + (e2 - e1) t = (0, 0, 1) + (2, 0, 0) t: t = 0.25, s = 0.5, dist2 = 1,
#     u = 1 - t, v = t.  The proper triangle below is 2 away.
#   beside, Q_UNDER: q0 is straight below (0.25, 0.25, 0) of the proper triangle: candidate 0, its face, dist2 = 1; the segment is 2 above.
HAND_DISTANCE = [("segment", Q_X1, 1, 6, 0.5, 0, (1, 0, 1), (1, 0, 0), True), ("point", Q_Z2, 4, 3, 0, 0, (1, 1, 2), (1, 1, 0), True),
                 ("beside", Q_X05, 1, 7, 0.75, 0.25, (0.5, 0, 2), (0.5, 0, 1), True), ("beside", Q_UNDER, 1, 0, 0.25, 0.25, (0.25, 0.25, -1), (0.25, 0.25, 0), False)]

# (scene, query triangle, d, t, feature, u, v, point, normal, prim >= 0); tmax = 1.
#   segment, Q_X1 moving by (0, 0, -2): a zero-area triangle has e1 parallel to e2, so det = dot(e1, cross(d, e2)) = 0 in 0..2.  In 3..5
#     the ray -d = (0, 0, 2) is parallel to the query's plane x = 1 (a1 = (0, 2, 0), a2 = (0, 1, 1)): cross(-d, a2) = (-2, 0, 0) and
#     det = dot(a1, (-2, 0, 0)) = 0 too.  Pair 6: (0, 2 s, -2 tau) = (-1 + 2 w, 1, -1):
#     s = w = tau = 0.5, det = dot(a1, cross(d, -e1)) = dot((0, 2, 0), (0, 4, 0)) = 8.  Pair 7 has h = 0, det = 0; pair 8 gives 0.5 again,
#     later.  normal = cross(a1, e1) = (0, 0, -4), dot with d = 8 > 0: turned.
#   segment, moving by (0, 0, 2), away: nothing, t = tmax.
#   point, Q_Z2 moving by (0, 0, -4): only 3..5 have a determinant: the ray (0, 0, 4) tau from (1, 1, -2) meets the query's face at
#     tau = 0.5, inside; normal = cross(a1, a2) = (0, 0, 16), dot with d < 0: kept.  4 and 5 are the same vertex, later.
#   beside, Q_X05 moving by (0, 0, -2): pair 6 has the edge e1 = 0, det = 0; pair 7: w = 0.25, tau = 0.5, u = 1 - w, v = w; the proper
#     triangle would be reached at t = 1 = tmax, which is not before it.
HAND_TRI_CASTS = [("segment", Q_X1, DOWN2, 0.5, 6, 0.5, 0, (1, 0, 0), (0, 0, 4), True), ("segment", Q_X1, UP2, 1.0, -1, 0, 0, (0, 0, 0), (0, 0, 0), False),
                  ("point", Q_Z2, DOWN4, 0.5, 3, 0, 0, (1, 1, 0), (0, 0, 16), True), ("beside", Q_X05, DOWN2, 0.5, 7, 0.75, 0.25, (0.5, 0, 1), (0, 0, 4), True)]

# Weights: cross(e1, e2) = 0 on the segment, the point and the v0 = v1 triangle: weight 0, and where that is the whole mesh every sample
# is the miss record.  The proper triangle of `beside` has a = |(0, 0, 1)| = 1 = 0.5 * 2^1: q = ldexp(1, 35 - 1) = 2^34, the total.
# Lookup on the segment at (u, v) = (0.25, 0.5): (v0 + 0.25 (2, 0, 0)) + 0.5 (2, 0, 0) = (1.5, 0, 0); w = (1 - 0.25) - 0.5 = 0.25 and the
# three vertex normals are (0, 0, 1): shading (0, 0, 1).
# Ambient occlusion from (0.25, 0.25, 0) under `beside`, normal (0, 0, 1): the only triangle above is the v0 = v1 one, det = 0 < 1e-6:
# every sample is open, as it is over the proper triangle alone.
HAND_AO_POINT, HAND_AO_SAMPLES = (0.25, 0.25, 0.0), 64


def hand_zero(g, prim):
    return ~(g.e1[prim] != 0).any(axis=1) | ~(g.e2[prim] != 0).any(axis=1) | (g.e1[prim] == g.e2[prim]).all(axis=1)


def check_hand_cases(geometry, run):
    """The paper values above against run(kind of query, scene, arrays...) -> the answer in the restatements' form.  geometry(name,
    triangles) gives (scene handle, Geometry, SurfaceScene, oracle scene)."""
    for name, pos in hm.HAND_SCENES.items():
        sc, g, s, osc = geometry(name, pos)
        rows = [h for h in HAND_DISTANCE if h[0] == name]
        res = run("distance", sc, g, s, osc, F([h[1] for h in rows]))
        assert res.d2.tolist() == [h[2] for h in rows] and res.feature.tolist() == [h[3] for h in rows] and (res.prim >= 0).all(), (name, res)
        assert res.u.tolist() == [h[4] for h in rows] and res.v.tolist() == [h[5] for h in rows], (name, res)
        assert res.point_q.tolist() == [list(map(float, h[6])) for h in rows] and res.point_t.tolist() == [list(map(float, h[7])) for h in rows], (name, res)
        assert hand_zero(g, res.prim).tolist() == [h[8] for h in rows], (name, res)
        rows = [h for h in HAND_TRI_CASTS if h[0] == name]
        res = run("tcast", sc, g, s, osc, F([h[1] for h in rows]), F([h[2] for h in rows]), F(1.0))
        assert res.t.tolist() == [h[3] for h in rows] and res.feature.tolist() == [h[4] for h in rows], (name, res)
        assert res.u.tolist() == [h[5] for h in rows] and res.v.tolist() == [h[6] for h in rows], (name, res)
        assert res.point.tolist() == [list(map(float, h[7])) for h in rows] and res.normal.tolist() == [list(map(float, h[8])) for h in rows], (name, res)
        assert (res.prim >= 0).tolist() == [h[9] for h in rows] and hand_zero(g, res.prim[res.prim >= 0]).all(), (name, res)
        cdf, (prim, u, v) = run("weights", sc, g, s, osc)
        zero = hand_zero(g, np.arange(len(g.v0)))
        if name == "beside":
            assert zero.sum() == 1 and np.diff([0] + cdf).tolist() == [0 if z else 2 ** 34 for z in zero], cdf
            assert (prim == np.nonzero(~zero)[0][0]).all() and (u >= 0).all() and (v >= 0).all() and (u + v <= 1).all()
            ao = run("ambient", sc, g, s, osc, F([HAND_AO_POINT]), F([[0, 0, 1]]), F([np.inf]), F([0.001]))
            alone = ar.ambient(hm.oracle_scene(hm.Mesh(pos[~zero], np.tile(F([0, 0, 1]), (1, 3, 1)), np.zeros((1, 3, 2), F), np.zeros(1, np.int32), None, None)),
                               F([HAND_AO_POINT]), F([[0, 0, 1]]), F([np.inf]), F([0.001]), HAND_AO_SAMPLES, AO_SEED)
            assert ao[0, 0] == HAND_AO_SAMPLES and (ao == alone).all(), (ao, alone)
        else:
            assert cdf == [0] and (prim == -1).all() and not u.any() and not v.any(), (name, cdf, prim)
        if name == "segment":
            rec = run("lookup", sc, g, s, osc, np.int32([0]), F([0.25]), F([0.5])).view(F)
            assert rec[0, sr.POSITION].tolist() == [1.5, 0, 0] and rec[0, sr.SHADING].tolist() == [0, 0, 1] and rec[0, sr.UV].tolist() == [0, 0], rec
            assert rec.view(np.int32)[0, sr.MATERIAL] == 0 and rec.view(np.int32)[0, sr.LOAD_INDEX] == 0
