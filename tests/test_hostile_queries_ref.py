"""Triangle distance, triangle casts, surface lookups with area-weighted sampling and ambient occlusion (include/drt.h) on the meshes
of tests/hostile_meshes.py, on the restatements alone (CPU only; the product's host scene is read, no device is touched): hand cases on
a segment, a point and a v0 = v1 triangle; on the degenerate and the offset mesh each restatement against its own all-triangles answer
and against float64; the conditions under which tests/test_gpu_hostile_queries.py meets the hard cases; and the range of scales in
which the rules work -- what the "working range" paragraph of include/drt.h states of these four queries."""
import math

import numpy as np
import pytest

from tests import ambient_ref as ar
from tests import hostile_meshes as hm
from tests import hostile_queries as hq
from tests import nearest_ref as nr
from tests import ray_query_ref as rq
from tests import surface_ref as sr
from tests import tri_cast_ref as tc
from tests import tri_distance_ref as td
from tests.test_hostile_meshes_ref import OUT_OF_RANGE, SEED

F = np.float32


def product():
    """The product's library (its host scene is what surface_ref reads); the tests that need it skip where it is not built."""
    return pytest.importorskip("dustraytracer_amd")


def hand_geometry(name, pos):
    """A hand scene from arrays alone, without the product: one leaf, load order, vertex normals (0, 0, 1)."""
    n = len(pos)
    up = np.tile(F([0, 0, 1]), (n, 3, 1))
    osc = hm.oracle_scene(hm.Mesh(pos, up, np.zeros((n, 3, 2), F), np.zeros(n, np.int32), None, None))
    return None, nr.from_triangles(pos), sr.from_triangles(pos)._replace(normals=up), osc


def product_hand_geometry(name, pos):
    """The same hand scene as the product builds it (what tests/test_gpu_hostile_queries.py loads)."""
    n = len(pos)
    sc, osc = rq.programmatic_scene(product(), pos, np.tile(F([0, 0, 1]), (n, 3, 1)), np.zeros((n, 3, 2), F), np.zeros(n, np.int32), hm.ONE_MATERIAL, [], hm.LEAF, hm.BINS)
    return sc, nr.from_oracle(osc), sr.from_product(sc), osc


def _run(kind, sc, g, s, osc, *a):
    if kind == "distance":
        return td.distance(g, *a)
    if kind == "tcast":
        return tc.cast(g, *a)
    if kind == "weights":
        cdf = sr.weights(s)
        return cdf, hq.sample_refs(sr.sample(s, hq.SAMPLE_SEED, 0, 200, cdf))
    if kind == "lookup":
        return sr.lookup(s, *a)
    return ar.ambient(osc, *a, hq.HAND_AO_SAMPLES, hq.AO_SEED)


def test_hand_cases_on_a_segment_a_point_and_a_triangle_beside_a_zero_area_one():
    """Every value is derived in the comments of tests/hostile_queries.py from the header's text.  This one needs no product library."""
    hq.check_hand_cases(hand_geometry, _run)


def test_hand_cases_on_the_product_s_host_scenes():
    hq.check_hand_cases(product_hand_geometry, _run)


class Case:
    def __init__(self, name):
        self.name = name
        drt = product()
        base = hq.with_uvs(hm.degenerate())
        self.mesh = base if name == "degenerate" else hm.offset(base)
        self.sc, self.osc = hm.scene_pair(drt, self.mesh)
        self.g = nr.from_oracle(self.osc)
        self.s = sr.from_product(self.sc)
        self.kind, self.twin = hm.kinds_in_tree_order(self.osc, self.mesh)
        self.q = hq.tri_queries(self.g, self.s, self.kind, self.twin, SEED)
        self.answers = hq.restate(self.g, self.osc, self.s, self.q)
        # (moved and rounded, a collinear triple is a sliver: on the offset mesh it has a normal and a side)
        self.zero_area = np.isin(self.kind, hm.ZERO_AREA) & ((self.kind != hm.COLLINEAR) | (name == "degenerate"))


_cases = {}


def _case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


@pytest.fixture(scope="module", params=["degenerate", "offset"])
def case(request):
    return _case(request.param)


def test_the_variant_mesh_is_the_same_mesh_with_uvs(case):
    """Positions, normals, kinds and the tree are those of tests/test_hostile_meshes_ref.py's mesh; only the uvs are new, and they
    reach the lookup's records."""
    plain = hm.degenerate() if case.name == "degenerate" else hm.offset(hm.degenerate())
    assert case.mesh.pos.tobytes() == plain.pos.tobytes() and case.mesh.nrm.tobytes() == plain.nrm.tobytes() and not plain.uv.any()
    posc = hm.oracle_scene(plain)
    assert all((posc.nodes[f] == case.osc.nodes[f]).all() for f in ("is_leaf", "child1", "child2", "prim_start", "prim_count"))
    assert posc.tris["p"].tobytes() == case.osc.tris["p"].tobytes()
    assert (case.s.v0 == case.g.v0).all() and (case.s.e1 == case.g.e1).all() and (case.s.e2 == case.g.e2).all()
    assert (np.abs(case.s.uv).max(axis=(1, 2)) > 0).all() and (np.abs(case.answers["lookup"][3]).max(axis=1) > 0).sum() > 5000


# Queries whose tree answer differs from the float32 answer over all triangles (seed 11), capped at the shares
# tests/test_hostile_meshes_ref.py took from tests/test_nearest_ref.py (the distance family, 0.5 %) and tests/test_sweep_ref.py (casts,
# 1 %): (distance, distance with max_dist, cast).  The six casts on the offset mesh are of one kind: over all triangles the overlap
# predicate, whose sums cancel at coordinates of 16384, does not separate the query from a zero-area triangle somewhere else (t = 0,
# feature 15 + 16), and the tree never comes near that triangle.
TREE_DIFFERS = {"degenerate": (0, 0, 0), "offset": (0, 0, 6)}


def test_each_tree_answer_is_its_float32_all_triangles_answer(case):
    g, q, A = case.g, case.q, case.answers
    bits = lambda x: np.ascontiguousarray(x, F).view(np.uint32)
    best, _, _ = td.brute_force(g, q.tris)
    best_md, _, _ = td.brute_force(g, q.tris, q.max_dist)
    t, prim, feature = tc.brute_force(g, q.cast_tris, q.dirs, q.tmax)
    cast = tc.TriHits(*A["tcast"])
    d = (int((bits(A["distance"][1]) != bits(best)).sum()), int((bits(A["distance_md"][1]) != bits(best_md)).sum()),
         int(((bits(cast.t) != bits(t)) | (cast.prim != prim) | (cast.feature != feature)).sum()))
    print("%s: queries that differ from the float32 all-triangles answer: distance %d and with max_dist %d of %d, cast %d of %d" % ((case.name,) + d[:2] + (len(q.tris), d[2], len(q.cast_tris))))
    assert d == TREE_DIFFERS[case.name]
    assert max(d[0], d[1]) <= 0.005 * len(q.tris) and d[2] <= 0.01 * len(q.cast_tris)


# (segment queries, of them with d2 = 0 over all triangles, with d2 = 0 from the tree, with t = 0 over all triangles, from the tree)
ZERO_AREA_QUERIES = (54, 54, 12, 54, 11)


def test_a_zero_area_query_touches_every_point_of_the_scene(case):
    """Why the query triangles above are proper ones (hq.proper).  The overlap predicate passes a segment or point QUERY against a
    POINT of the scene wherever it is -- every axis of the pair is a zero vector or sees a zero-length interval inside the other -- so
    over all triangles every such query has d2 = 0 and t = 0 (feature bit 16) while the mesh holds one point triangle; the tree
    reports it only where the query's own neighbourhood holds one.  The header says so of drt_renderer_overlap_triangles; the
    distance and the cast inherit it.  The answer over all triangles is not the yardstick for such queries: they travel in a batch
    of their own (TriQueries.flat), which tests/test_gpu_hostile_queries.py compares with the restatement's tree answer bit for bit."""
    g = case.g
    segs = hm.aimed_triangle_parts(g, case.kind, case.twin, SEED + 101)[0][::4]      # the segments among the batch hq.zero_area_queries sends
    assert (segs[:, 1] == segs[:, 2]).all() and segs.tobytes() == case.q.flat[0][:len(segs)].tobytes()
    best, prim, feature = td.brute_force(g, segs)
    tree = td.distance(g, segs)
    d = F([0.1, 0.2, 0.3])
    t, _, _ = tc.brute_force(g, segs, d, 1.0)
    found = (len(segs), int((best == 0).sum()), int((tree.d2 == 0).sum()), int((t == 0).sum()), int((tc.cast(g, segs, d, 1.0).t == 0).sum()))
    print("%s: %d segment queries: d2 = 0 for %d over all triangles and %d from the tree, t = 0 for %d and %d; the triangle over all triangles is a point for %d"
          % ((case.name,) + found + (int((case.kind[prim] == hm.POINT).sum()),)))
    assert found == ZERO_AREA_QUERIES and (feature >= 16).all() and (case.kind[prim] == hm.POINT).sum() >= 50


# The measured largest figures of the restatements on exactly these inputs (seed 11), in units of 2^-23 M, M = the largest absolute
# coordinate of the query (for a cast: of its path up to the contact) and the scene.  Each bound is four times the figure.
#   distance         |sqrt(d2) - d64| against the float64 rule over all triangles, the winner no sliver or needle
#   distance_sliver  the same where a sliver or a needle wins.  (The predicate decides d2 = 0 in float32 and in float64 on its own
#                    roundings: where they disagree the figure is the whole float64 distance.)
#   contact          the float64 distance between the query triangle moved by d t and triangle prim, over the entering contacts
#                    (feature < 16) of proper query triangles with scene triangles that are no slivers or needles
#   contact_sliver   the same on the scene's slivers and needles, the query a proper triangle
#   contact_thin_query   the same where the QUERY is a sliver or a needle: the thin triangles' own copies, held off and cast back at their
#                    place.  A finding: every determinant and numerator of such a pair is a rounding error, as in the sphere cast's
#                    face test, and a candidate can pass with tau = 0: a thin triangle's own copy, tenths of a scene unit from it,
#                    is reported in contact at t = 0 (extent 4, M 17); the bound of this row constrains nothing and only records that.
#                    On the offset mesh every coordinate is a multiple of 2^-9 and the sums are nearly exact: the figures there are tiny.
#   weights          |q_k - 2^(35 - e) a64_k|, in units of 2^35 2^-23 (one ulp of the largest weight): a is a square root of a sum of
#                    squares of differences of products, each rounded
MEASURED = {"degenerate": {"distance": 0.544479, "distance_sliver": 0.437940, "contact": 0.399221, "contact_sliver": 0.210365, "contact_thin_query": 87817.187408, "weights": 0.144807},
            "offset": {"distance": 0.000069, "distance_sliver": 0.000302, "contact": 0.000213, "contact_sliver": 0.000109, "contact_thin_query": 0.000123, "weights": 0.106457}}
BOUND = {name: {k: 4 * v for k, v in row.items()} for name, row in MEASURED.items()}


def _check(case, what, err):
    err = np.asarray(err, np.float64)
    worst = float(err.max(initial=0))
    print("%s: largest %s figure %.6f over %d (pinned %.6f, bound %.6f)" % (case.name, what, worst, len(err), MEASURED[case.name][what], BOUND[case.name][what]))
    return bool((err <= BOUND[case.name][what]).all()) and abs(worst - MEASURED[case.name][what]) <= 1e-6 + 1e-4 * worst


def test_distances_against_float64_over_all_triangles(case):
    g, q = case.g, case.q
    res = td.TriNear(*case.answers["distance"])
    assert (res.prim >= 0).all()
    best, _, _ = td.brute_force(g, q.tris, dtype=np.float64)
    err = np.abs(np.sqrt(res.d2.astype(np.float64)) - np.sqrt(best)) / (2.0 ** -23 * td.scale_of(g, q.tris))
    sliver = np.isin(case.kind[res.prim], (hm.SLIVER, hm.NEEDLE))
    assert all([_check(case, "distance", err[~sliver]), _check(case, "distance_sliver", err[sliver])])


def test_cast_contacts_against_float64(case):
    g, q = case.g, case.q
    res = tc.TriHits(*case.answers["tcast"])
    sel = np.nonzero((res.prim >= 0) & (res.feature < 16))[0]
    assert len(sel) > 100
    k = res.prim[sel]
    moved = q.cast_tris[sel].astype(np.float64) + (q.dirs[sel].astype(np.float64) * res.t[sel].astype(np.float64)[:, None])[:, None, :]
    v0, e1, e2 = (x[k].astype(np.float64) for x in (g.v0, g.e1, g.e2))
    d2 = td.pair(moved[:, 0], moved[:, 1], moved[:, 2], v0, e1, e2).candidates_d2
    assert np.isfinite(d2).all()
    M = np.maximum(tc.scale_of(g, q.cast_tris[sel]), np.abs(moved).max(axis=(1, 2)))
    err = np.sqrt(d2) / (2.0 ** -23 * M)
    e1q, e2q = (q.cast_tris[sel, j].astype(np.float64) - q.cast_tris[sel, 0] for j in (1, 2))
    longest = np.maximum(np.linalg.norm(e1q, axis=1), np.linalg.norm(e2q, axis=1))
    thin_query = np.linalg.norm(np.cross(e1q, e2q), axis=1) < 2.0 ** -10 * longest * longest           # a thin triangle's own copy, cast back onto it
    sliver = np.isin(case.kind[k], (hm.SLIVER, hm.NEEDLE))
    assert all([_check(case, "contact", err[~sliver & ~thin_query]), _check(case, "contact_sliver", err[sliver & ~thin_query]),
                _check(case, "contact_thin_query", err[thin_query])])


# (triangles whose fp32 area is exactly 0, of those of a zero-area kind): on the degenerate mesh two slivers have it too; on the offset
# mesh the five collinear triples are slivers with an area, and four needles, whose short edge of 2^-12 is below the ulp there, have none
ZERO_WEIGHTS = {"degenerate": (26, 24), "offset": (23, 19)}
N_FREQUENCY = 20000


def test_weights_against_a_float64_cumulative_sum_and_the_samples_frequencies(case):
    s = case.s
    cdf = sr.weights(s)
    w = np.diff(np.array([0] + cdf, dtype=object)).astype(np.float64)
    a = sr.areas(s)
    e = math.frexp(float(a.max()))[1]
    a64 = np.linalg.norm(np.cross(s.e1.astype(np.float64), s.e2.astype(np.float64)), axis=1)
    assert _check(case, "weights", np.abs(w - a64 * 2.0 ** (35 - e)) / (2.0 ** 35 * 2.0 ** -23))
    assert abs(cdf[-1] - (a64 * 2.0 ** (35 - e)).sum()) <= 360 * BOUND[case.name]["weights"] * 2.0 ** 12
    zero = w == 0
    print("%s: %d triangles weigh 0, %d of them of a zero-area kind; kinds %r" % (case.name, zero.sum(), (zero & case.zero_area).sum(),
                                                                               [hm.KIND_NAMES[k] for k in sorted(set(case.kind[zero].tolist()))]))
    assert (int(zero.sum()), int((zero & case.zero_area).sum())) == ZERO_WEIGHTS[case.name] and zero[case.zero_area].all() and ((a == 0) == zero).all()
    prim, u, v = hq.sample_refs(sr.sample(s, 5, 0, N_FREQUENCY, cdf))
    counts = np.bincount(prim, minlength=len(w))
    share = w / w.sum()
    sd = np.sqrt(N_FREQUENCY * share * (1 - share))
    z = np.abs(counts - N_FREQUENCY * share) / np.maximum(sd, 1e-9)
    print("%s: %d samples: largest |count - n share| = %.2f standard deviations; %d samples on triangles of weight 0" % (case.name, N_FREQUENCY, z[~zero].max(), counts[zero].sum()))
    assert (prim >= 0).all() and counts[zero].sum() == 0 and (z[~zero] <= 5).all()
    # the 5140 samples the GPU test draws, at either end of the stream
    for which in ("samples", "samples_top"):
        p = case.answers[which][0]
        assert (p >= 0).all() and not zero[p].any() and len(set(p.tolist())) > 150


# ---------------------------------------------------------------- what the GPU test relies on: the hard cases are met

def test_coverage_conditions(case):
    """Stated on the restatement's output for exactly the queries tests/test_gpu_hostile_queries.py sends, so that it cannot pass by
    avoiding the hard cases.  The minima are below the counts measured here (printed)."""
    A, kind, twin, za, q = case.answers, case.kind, case.twin, case.zero_area, case.q
    seen = np.zeros(10, np.int64)
    dist, md = td.TriNear(*A["distance"]), td.TriNear(*A["distance_md"])
    won = za[dist.prim]
    touching = dist.d2 == 0
    deciding = set((dist.feature & 15).tolist())
    np.add.at(seen, kind[dist.prim], 1)
    tied = twin[dist.prim] >= 0
    to_smaller = int((dist.prim[tied] < twin[dist.prim[tied]]).sum())
    tied_apart = int((tied & (dist.d2 > 0)).sum())
    within = A["within"][0]
    print("%s distance: %d queries, zero-area triangles win %d, %d answers have d2 = 0, %d deciding candidates, %d answers on a duplicate pair (%d to the smaller prim, "
          "%d of them apart), with max_dist %d found and %d not, %d within; mesh distance from query %d"
          % (case.name, len(won), won.sum(), touching.sum(), len(deciding), tied.sum(), to_smaller, tied_apart, (md.prim >= 0).sum(), (md.prim < 0).sum(), within.sum(),
             A["mesh_distance"][1]))
    assert won.sum() >= 40 and touching.sum() >= 100 and len(deciding) == 15 and tied.sum() >= 20 and to_smaller == tied.sum() and tied_apart >= 5
    assert (md.prim >= 0).sum() >= 50 and (md.prim < 0).sum() >= 50 and 50 <= within.sum() and (~within).sum() >= 50 and (q.max_dist == 0).sum() >= 50
    assert (md.prim[q.max_dist == 0] == -1).all() and A["mesh_distance"][0] == 0 and A["mesh_distance"][1] == np.nonzero(touching)[0][0] and touching[1:].any()
    cast = tc.TriHits(*A["tcast"])
    hit = cast.prim >= 0
    on = hit & za[np.maximum(cast.prim, 0)]
    features = sorted(set(cast.feature[on].tolist()))
    np.add.at(seen, kind[cast.prim[hit]], 1)
    ctied = hit & (twin[np.maximum(cast.prim, 0)] >= 0)
    still = ~(q.dirs != 0).any(axis=1)
    any_ = A["casts_any"][0]
    print("%s cast: %d casts, %d hits, %d first contacts on zero-area triangles with features %r, %d start overlaps, %d hits on a duplicate pair (%d to the smaller prim), "
          "%d casts with d = 0 (%d of them hit); mesh cast t = %r from query %d"
          % (case.name, len(hit), hit.sum(), on.sum(), features, (cast.feature[hit] >= 16).sum(), ctied.sum(), (cast.prim[ctied] < twin[cast.prim[ctied]]).sum(),
             still.sum(), (hit & still).sum(), float(A["mesh_cast"][0]), A["mesh_cast"][1]))
    assert on.sum() >= 15 and len(features) >= 8 and ctied.sum() >= 20 and (cast.prim[ctied] < twin[cast.prim[ctied]]).all()
    assert hit.sum() >= 150 and (~hit).sum() >= 100 and (cast.feature[hit] >= 16).sum() >= 10 and still.sum() >= 50 and (any_ == hit).all() and A["mesh_cast"][1] >= 0
    assert (seen > 0).all(), dict(zip(hm.KIND_NAMES, seen.tolist()))
    # the zero-area QUERY triangles, a batch of their own: the pair rule with a = 0 and e = 0 together
    ft, fm, fc, fd, ftmax = q.flat
    fdist, fmd, fcast = td.TriNear(*A["flat_distance"]), td.TriNear(*A["flat_distance_md"]), tc.TriHits(*A["flat_tcast"])
    fhit = fcast.prim >= 0
    enter = fhit & (fcast.feature < 16)
    both = za[fdist.prim] & hq.is_flat(ft)
    print("%s zero-area queries: %d distance queries (%d of exactly zero area), %d apart, %d won by a zero-area triangle (%d of them apart), deciding candidates %r, "
          "with max_dist %d found and %d not; %d casts (%d of exactly zero area, %d with d = 0), %d hits, %d entering contacts with features %r, %d hits on zero-area "
          "triangles, %d start overlaps; mesh forms: d2 = %r from query %d, t = %r from query %d"
          % (case.name, len(ft), hq.is_flat(ft).sum(), (fdist.d2 > 0).sum(), both.sum(), (both & (fdist.d2 > 0)).sum(), sorted(set((fdist.feature & 15).tolist())),
             (fmd.prim >= 0).sum(), (fmd.prim < 0).sum(), len(fc), hq.is_flat(fc).sum(), (~(fd != 0).any(axis=1)).sum(), fhit.sum(), enter.sum(),
             sorted(set(fcast.feature[enter].tolist())), (fhit & za[np.maximum(fcast.prim, 0)]).sum(), (fcast.feature[fhit] >= 16).sum(),
             float(A["flat_mesh_distance"][0]), A["flat_mesh_distance"][1], float(A["flat_mesh_cast"][0]), A["flat_mesh_cast"][1]))
    assert hq.is_flat(ft).sum() >= 120 and (fdist.prim >= 0).all() and (fdist.d2 > 0).sum() >= 50 and both.sum() >= 30 and (both & (fdist.d2 > 0)).sum() >= 5
    assert len(set((fdist.feature & 15).tolist())) >= 12 and (fmd.prim >= 0).sum() >= 40 and (fmd.prim < 0).sum() >= 20
    assert hq.is_flat(fc).sum() >= 90 and fhit.sum() >= 40 and (~fhit).sum() >= 30 and enter.sum() >= 20 and len(set(fcast.feature[enter].tolist())) >= 6
    assert (fhit & za[np.maximum(fcast.prim, 0)]).sum() >= 15 and (A["flat_casts_any"][0] == fhit).all() and A["flat_mesh_cast"][1] >= 0
    # ... among them the mesh's own zero-area triangles, in place (distance) and held off and cast back (casts)
    own = hm.aimed_triangle_parts(case.g, kind, twin, SEED + 101)[1]
    own = own[hq.is_flat(own)]
    assert len(own) >= 15 and ft[-len(own):].tobytes() == own.tobytes() and hq.is_flat(fc[54:54 + len(own)]).sum() >= 15
    # references: on zero-area triangles, from the nearest answers and the hostile ones; the records of all three kinds
    prim = q.refs[0]
    ok = (prim >= 0) & (prim < len(za))
    on_zero = ok & za[np.where(ok, prim, 0)]
    with np.errstate(invalid="ignore"):
        wild = ~(np.abs(q.refs[1]) <= 1) | ~(np.abs(q.refs[2]) <= 1)
    position, normal = A["lookup"][0], A["lookup"][1]
    print("%s surface: %d references and %d samples, %d references on zero-area triangles, %d outside the mesh, %d with u or v beyond [-1, 1], infinite or a NaN; %d records "
          "with a NaN normal, %d with a NaN position" % (case.name, len(prim), hq.N_SAMPLES, on_zero.sum(), (~ok).sum(), wild.sum(), np.isnan(normal).any(axis=1).sum(),
                                                         np.isnan(position).any(axis=1).sum()))
    assert on_zero.sum() >= 50 and (~ok).sum() >= 15 and wild.sum() >= 50 and np.isnan(position).any(axis=1).sum() >= 5
    assert np.isnan(normal).any(axis=1).sum() >= (50 if case.name == "degenerate" else 30)
    # ambient points
    p, n, reach, bias = q.ao
    with np.errstate(invalid="ignore"):
        no_normal = np.isnan(n).any(axis=1) | ~(n != 0).any(axis=1)
    rec = {s_: A["ambient_%d" % s_][0] for s_ in hq.AO_SAMPLES}
    mixed = {s_: int(((r[:, 0] > 0) & (r[:, 0] < s_)).sum()) for s_, r in rec.items()}
    with np.errstate(invalid="ignore"):
        step = (n * bias[:, None]).astype(F)
        lost = int((~no_normal & ((step != 0) & ((p + step).astype(F) == p)).any(axis=1)).sum())       # a coordinate of o = p + n * bias stays at p's
    print("%s ambient: %d points, %d with a zero or NaN normal, %d with a finite max_dist, biases %r, %d points whose bias is rounded away in a coordinate; points with "
          "blocked and open samples per sample count %r" % (case.name, len(p), no_normal.sum(), np.isfinite(reach).sum(), sorted(set(bias.tolist())), lost, mixed))
    assert no_normal.sum() >= (20 if case.name == "degenerate" else 10) and np.isfinite(reach).sum() >= 40 and len(set(bias.tolist())) == 3
    assert all(v >= 20 for v in mixed.values()) and (lost >= 10 or case.name != "offset")
    assert all((r[no_normal, 0] == s_).all() for s_, r in rec.items())          # no normal: a NaN direction hits nothing


# ---------------------------------------------------------------- the range of scales in which the rules work

def _scaled_case(case, k, kinds, q=None):
    mesh = hm.scaled(case.mesh, k)
    sc, osc = hm.scene_pair(product(), mesh)
    for f in ("is_leaf", "child1", "child2", "prim_start", "prim_count"):       # the same tree: the builder's choices are scale-free here
        assert (osc.nodes[f] == case.osc.nodes[f]).all(), (k, f)
    g = nr.from_oracle(osc)
    s = sr.from_product(sc)
    return s, hq.restate(g, osc, s, hq.scaled_tri_queries(case.q if q is None else q, k), kinds)


# Entries of the degenerate mesh's answers that differ after scaling by 2^20 and 2^-20, for the kinds that are not unchanged there.
# Ambient occlusion inherits the ray family's absolute 1e-6: at 2^-20 every triangle is dropped and every sample of every live point
# is open; at 2^20 grazing triangles come back.
DIFFERS_AT = {20: {"ambient_16": 14, "ambient_7": 14, "ambient_65": 17}, -20: {"ambient_16": 56, "ambient_7": 41, "ambient_65": 70}}


@pytest.mark.parametrize("k", [20, -20])
def test_scaling_by_2_to_the_20_changes_nothing_where_the_rule_allows(k):
    case = _case("degenerate")
    _, B = _scaled_case(case, k, hq.KINDS)
    d = {kind: hq.differing(hq.rescale(kind, case.answers[kind], k), B[kind]) for kind in hq.KINDS}
    print("2^%d: entries that differ from the plain answer scaled: %r" % (k, d))
    assert {kind: v for kind, v in d.items() if v != 0} == DIFFERS_AT[k]
    assert all(d[kind] == 0 for kind in hq.DISTANCE_KINDS + hq.SURFACE_KINDS)
    if k == -20:
        for n in hq.AO_SAMPLES:
            assert (B["ambient_%d" % n][0][:, 0] == n).all()


# The range of k, in steps of 2, over which scaled(k) with scaled queries gives the plain answer scaled on EVERY query of the aimed
# queries plus about 60 general ones.  Distance: the fourth powers of drt_renderer_nearest and of den = a e - b b.  Cast: third powers
# with the direction scaled too, and the predicate's fourth.  Weights and samples: a is a second power and a^2, under the square root, a
# fourth; the table is relative to the largest area, so it is unchanged until the first area^2 overflows or the first one underflows.
RANGE = {"distance": (-22, 28), "tcast": (-32, 32), "weights": (-22, 32)}
# The two "mixed" scales of the weights: some areas have overflowed to infinity (weight 0), or their squares have underflowed to 0,
# while the rest still sample.  (triangles of weight 0 of 360)
MIXED = {-36: 331, 34: 220}


def _weightless(answer):
    cdf = answer["weights"][0].copy().view(np.uint64).reshape(-1)
    return int((np.diff(np.concatenate([[0], cdf.astype(object)])) == 0).sum()), int(cdf[-1])


def test_the_range_of_scales_of_distance_cast_and_weights():
    case = _case("degenerate")
    q = hq.tri_queries(case.g, case.s, case.kind, case.twin, SEED, general=60)
    groups = {"distance": ("distance",), "tcast": ("tcast",), "weights": ("weights", "samples")}
    plain = hq.restate(case.g, case.osc, case.s, q, sum(groups.values(), ()))
    found = {}
    for name, kinds in groups.items():
        ends = []
        for step in (-2, 2):
            k = 0
            while abs(k) < 70:
                _, B = _scaled_case(case, k + step, kinds, q)
                if any(hq.differing(hq.rescale(kind, plain[kind], k + step), B[kind]) != 0 for kind in kinds):
                    break
                k += step
            ends.append(k)
        found[name] = tuple(ends)
        print("%s: scaling by 2^k changes nothing for k in [%d, %d]" % (name, *found[name]))
    assert found == RANGE
    for k in (20, -20):
        assert (RANGE["tcast"][0] <= k <= RANGE["tcast"][1]) == ("tcast" not in DIFFERS_AT[k])
    zero0, total0 = _weightless(plain)
    for k, zeros in MIXED.items():
        s, B = _scaled_case(case, k, ("weights", "samples"), q)
        zero, total = _weightless(B)
        w = np.diff(np.array([0] + sr.weights(s), dtype=object))
        print("2^%d: %d of 360 triangles weigh 0 (%d on the plain mesh), the total is %d, %d distinct triangles sampled" % (k, zero, zero0, total, len(set(B["samples"][0].tolist()))))
        assert zero == zeros and total > 0 and (B["samples"][0] >= 0).all() and (w[B["samples"][0]] > 0).all()
    for k in OUT_OF_RANGE:
        s, B = _scaled_case(case, k, ("distance", "tcast", "weights", "samples", "lookup"), q)
        zero, total = _weightless(B)
        print("2^%d: %d of 360 triangles weigh 0, the total is %d" % (k, zero, total))
        assert (zero, total) == (360, 0) and (B["samples"][0] == -1).all() and not B["samples"][1].any() and not B["samples"][2].any()
        assert hq.differing(hq.rescale("distance", plain["distance"], k), B["distance"]) != 0 and hq.differing(hq.rescale("tcast", plain["tcast"], k), B["tcast"]) != 0
        assert (B["lookup"][7][len(q.refs[0]):, 0].view(np.int32) == -1).all()                 # the lookup of a miss is the miss record


def test_the_subnormal_branch_of_the_weights_exponent_cannot_be_reached():
    """surface_exponent (csrc/surface.hpp) has a branch for a subnormal amax.  amax = sqrtf(x) of a float32 x; the smallest positive x
    is 2^-149 and its root, 2^-74.5, is a normal number: whatever the mesh, amax is 0 or at least 2^-75, never subnormal.  (The code
    stays: the branch is dead, not wrong.)"""
    tiny = np.float32(2.0 ** -149)
    assert tiny > 0 and np.sqrt(tiny) >= np.float32(2.0 ** -75) and np.sqrt(tiny) > np.finfo(np.float32).tiny
    a = sr.areas(sr.from_triangles(F([[[0, 0, 0], [2.0 ** -37, 0, 0], [0, 2.0 ** -37, 0]], [[0, 0, 0], [2.0 ** -38, 0, 0], [0, 2.0 ** -37, 0]]])))
    assert a.tolist() == [2.0 ** -74, 0.0]                                  # 2^-148 is a float32, 2^-150 is not
