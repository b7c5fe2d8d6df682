"""Triangle distance, triangle casts, surface lookups with area-weighted sampling and ambient occlusion on the GPU against meshes that
are not well behaved (tests/hostile_meshes.py, with the uvs of tests/hostile_queries.py): zero-area triangles of every kind, slivers,
needles, duplicates; the same mesh far from the origin; scaled by 2^20 and 2^-20; scaled beyond the range in which the rules keep their
digits, where both sides go wrong in the same way; and, for the weights, the two scales at which part of the table has overflowed or
underflowed.  Every field of every record is bit-equal to the restatement.  tests/test_hostile_queries_ref.py shows, on the
restatements alone, that these queries meet the hard cases and where the working range ends."""
import numpy as np
import pytest

import oracle
from tests import hostile_meshes as hm
from tests import hostile_queries as hq
from tests import nearest_ref as nr
from tests import refit_ref as rf
from tests import surface_ref as sr
from tests import tri_distance_ref as td
from tests.test_hostile_queries_ref import MIXED, OUT_OF_RANGE, SEED

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
MESHES = ["degenerate", "offset", "scaled(20)", "scaled(-20)", "scaled(%d)" % OUT_OF_RANGE[0], "scaled(%d)" % OUT_OF_RANGE[1]]
MIXED_MESHES = ["scaled(%d)" % k for k in sorted(MIXED)]
_cache = {}


@pytest.fixture(scope="module")
def renderer():
    return drt.Renderer(0)


class Pair:
    """A mesh as the product's scene and the oracle's, the queries for it and what the restatements say of them (each kind computed
    once, when a test first asks for it)."""

    def __init__(self, name):
        base = hq.with_uvs(hm.degenerate())
        if name.startswith("scaled"):
            k = int(name[len("scaled("):-1])
            self.mesh, self.q = hm.scaled(base, k), hq.scaled_tri_queries(pair("degenerate").q, k)
        else:
            self.mesh = base if name == "degenerate" else hm.offset(base)
        self.sc, self.osc = hm.scene_pair(drt, self.mesh)
        self.g = nr.from_oracle(self.osc)
        self.s = sr.from_product(self.sc)
        self.kind, self.twin = hm.kinds_in_tree_order(self.osc, self.mesh)
        if not name.startswith("scaled"):
            self.q = hq.tri_queries(self.g, self.s, self.kind, self.twin, SEED)
        self._answers = {}

    def answer(self, kind):
        if kind not in self._answers:
            self._answers[kind] = hq.restate(self.g, self.osc, self.s, self.q, (kind,))[kind]
        return self._answers[kind]


def pair(name):
    if name not in _cache:
        _cache[name] = Pair(name)
    return _cache[name]


def equal(got, ref, what):
    """Bit for bit on every array of two tuples, of the same shape and dtype (a NaN equals any NaN: a NaN's payload is not
    arithmetic; a 0-dimensional array is an array of one)."""
    assert len(got) == len(ref), what
    for i, (g, r) in enumerate(zip(got, ref)):
        g, r = np.ascontiguousarray(g), np.ascontiguousarray(r)
        assert g.shape == r.shape and g.dtype == r.dtype, (what, i, g.shape, r.shape, g.dtype, r.dtype)
        g, r = np.atleast_1d(g), np.atleast_1d(r)
        g, r = (g.astype(np.uint8) if g.dtype == bool else g), (r.astype(np.uint8) if r.dtype == bool else r)
        if g.size == 0:
            continue
        bits = {1: np.uint8, 4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
        diff = g.view(bits) != r.view(bits)
        if g.dtype == np.float32:
            diff &= ~(np.isnan(g) & np.isnan(r))
        bad = np.nonzero(diff.reshape(len(g), -1).any(axis=1))[0]
        assert len(bad) == 0, "%s: field %d differs in %d of %d records, first %d: %r vs %r" % (what, i, len(bad), len(g), bad[0], g[bad[0]], r[bad[0]])


def tri_near(res):
    """A TriNearest of the Python interface in the restatement's order."""
    return (res.point_q, res.d2, res.point_t, res.prim, res.u, res.v, res.feature)


def tri_hits(res):
    return (res.point, res.t, res.normal, res.prim, res.u, res.v, res.feature)


def surface_records(res):
    from tests.test_gpu_surface import records
    return hq.surface_fields(records(res))


def ambient_records(res):
    return (np.concatenate([res.open.reshape(-1, 1), res.sums.reshape(-1, 3)], axis=1).astype(np.int32),)


def run_ambient(rend, sc, ao, samples):
    p, n, reach, bias = ao
    return ambient_records(rend.ambientOcclusion(sc, points=p, normals=n, samples=samples, max_dist=reach, bias=bias, seed=hq.AO_SEED))


def check_distances(renderer, name, flat):
    """triangleDistance with and without max_dist, withinDistance and meshDistance on the proper query triangles, or (flat = "flat_") on
    the zero-area ones."""
    p = pair(name)
    sc, q = p.sc, hq.flat_view(p.q) if flat else p.q
    name = name + " " + flat
    equal(tri_near(renderer.triangleDistance(sc, q.tris)), p.answer(flat + "distance"), name + " triangleDistance")
    equal(tri_near(renderer.triangleDistance(sc, q.tris, q.max_dist)), p.answer(flat + "distance_md"), name + " triangleDistance, max_dist per query")
    equal((renderer.withinDistance(sc, q.tris, q.max_dist),), p.answer(flat + "within"), name + " withinDistance")
    got = renderer.meshDistance(sc, q.tris)
    equal((got.d2, got.query, got.prim, got.point_q, got.point_t, got.feature), p.answer(flat + "mesh_distance"), name + " meshDistance")
    # every query that is found and does not touch, twice: every d2 is tied with its copy, and the smaller query index wins
    ref = td.TriNear(*p.answer(flat + "distance"))
    apart = np.nonzero((ref.prim >= 0) & (ref.d2 > 0))[0]
    twice = np.concatenate([apart, apart])
    want = hq.mesh_reduce(ref.d2[twice], np.ones(len(twice), bool), (ref.prim[twice], ref.point_q[twice], ref.point_t[twice], ref.feature[twice]),
                          (np.array(-1, np.int32), np.zeros(3, F), np.zeros(3, F), np.array(0, np.int32)))
    got = renderer.meshDistance(sc, q.tris[twice])
    equal((got.d2, got.query, got.prim, got.point_q, got.point_t, got.feature), want, name + " meshDistance of a batch with every query twice")
    assert len(apart) == 0 or want[1] < len(apart)


def check_casts(renderer, name, flat):
    p = pair(name)
    sc, q = p.sc, hq.flat_view(p.q) if flat else p.q
    name = name + " " + flat
    equal(tri_hits(renderer.triangleCast(sc, q.cast_tris, q.dirs, q.tmax)), p.answer(flat + "tcast"), name + " triangleCast")
    equal((renderer.castsAny(sc, q.cast_tris, q.dirs, q.tmax),), p.answer(flat + "casts_any"), name + " castsAny")
    got = renderer.meshCast(sc, q.cast_tris, q.mesh_dir, q.tmax)
    equal((got.t, got.query, got.prim, got.point, got.normal, got.feature), p.answer(flat + "mesh_cast"), name + " meshCast")


@pytest.mark.parametrize("name", MESHES)
def test_triangle_distances_are_bit_equal_to_the_restatement(renderer, name):
    check_distances(renderer, name, "")


@pytest.mark.parametrize("name", MESHES)
def test_triangle_casts_are_bit_equal_to_the_restatement(renderer, name):
    check_casts(renderer, name, "")


@pytest.mark.parametrize("name", MESHES)
def test_zero_area_query_triangles_are_bit_equal_to_the_restatement(renderer, name):
    """The batch of zero-area QUERY triangles (hq.zero_area_queries) against the hostile scene triangles: the pair rule with a = 0
    and e = 0 together, 0 / 0 and NaNs on both sides, and the predicate that passes a segment against every point of the scene."""
    assert hq.is_flat(pair("degenerate").q.flat[0]).sum() >= 120
    check_distances(renderer, name, "flat_")
    check_casts(renderer, name, "flat_")


@pytest.mark.parametrize("name", MESHES + MIXED_MESHES)
def test_weights_samples_and_lookups_are_bit_equal_to_the_restatement(renderer, name):
    p = pair(name)
    sc, q, n = p.sc, p.q, hq.N_SAMPLES
    got = renderer.surfaceWeights(sc)
    assert got.dtype == np.uint64
    equal((got.view(np.uint32).reshape(-1, 2),), p.answer("weights"), name + " surfaceWeights")
    smp = renderer.sampleSurface(sc, n, seed=hq.SAMPLE_SEED)
    equal(tuple(smp), p.answer("samples"), name + " sampleSurface")
    equal(tuple(renderer.sampleSurface(sc, n, seed=hq.SAMPLE_SEED, first=2 ** 32 - n)), p.answer("samples_top"), name + " sampleSurface at the end of the stream")
    if name in MIXED_MESHES:
        zero = np.diff(np.concatenate([[0], got.astype(object)])) == 0
        assert zero.sum() == MIXED[int(name[len("scaled("):-1])] and (smp.prim >= 0).all() and not zero[smp.prim].any()
    prim, u, v = (np.concatenate([a, b]) for a, b in zip(q.refs, smp))                # the nearest answers, the hostile references, the samples
    equal(surface_records(renderer.surface(sc, prim, u, v)), p.answer("lookup"), name + " surface")
    equal(surface_records(renderer.surface(sc, smp)), tuple(a[len(q.refs[0]):] for a in p.answer("lookup")), name + " surface of the samples as they stand")


@pytest.mark.parametrize("name", MESHES)
def test_ambient_occlusion_is_bit_equal_to_the_restatement(renderer, name):
    p = pair(name)
    for samples in hq.AO_SAMPLES:
        equal(run_ambient(renderer, p.sc, p.q.ao, samples), p.answer("ambient_%d" % samples), "%s ambientOcclusion, %d samples" % (name, samples))


def test_the_hard_cases_are_in_these_answers():
    """The conditions of tests/test_hostile_queries_ref.py, on the answers compared above: the same seed gives the same queries."""
    from tests import test_hostile_queries_ref as ref
    for name in ("degenerate", "offset"):
        p, c = pair(name), ref._case(name)
        for f in hq.TriQueries._fields:
            a, b = getattr(p.q, f), getattr(c.q, f)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) if isinstance(a, tuple) else a.tobytes() == b.tobytes(), (name, f)
        ref.test_coverage_conditions(c)


def test_hand_cases_on_a_segment_a_point_and_a_triangle_beside_a_zero_area_one(renderer):
    """The values derived on paper in tests/hostile_queries.py, through the GPU."""
    from tests.test_hostile_queries_ref import _run, product_hand_geometry

    def run(kind, sc, g, s, osc, *a):
        want = _run(kind, sc, g, s, osc, *a)
        if kind == "distance":
            got = renderer.triangleDistance(sc, *a)
            equal(tri_near(got), tuple(want), "hand distance")
        elif kind == "tcast":
            got = renderer.triangleCast(sc, a[0], a[1], float(a[2]))
            equal(tri_hits(got), tuple(want), "hand cast")
        elif kind == "weights":
            got = [int(x) for x in renderer.surfaceWeights(sc)], tuple(renderer.sampleSurface(sc, 200, seed=hq.SAMPLE_SEED))
            assert got[0] == want[0]
            equal(got[1], want[1], "hand samples")
        elif kind == "lookup":
            from tests.test_gpu_surface import records
            got = records(renderer.surface(sc, *a))
            assert sr.same(got, want)
        else:
            got = ambient_records(renderer.ambientOcclusion(sc, points=a[0], normals=a[1], samples=hq.HAND_AO_SAMPLES, max_dist=a[2], bias=a[3], seed=hq.AO_SEED))[0]
            assert (got == want).all()
        return got
    hq.check_hand_cases(product_hand_geometry, run)


def test_refit_into_degeneracy_for_the_four_queries(renderer):
    """tests/test_gpu_hostile_meshes.py's refit, for these queries: the mesh is loaded without its thin triangles and a refit collapses
    20 triangles and moves 10 onto others.  The refitted renderer answers for the host scene refitted with the same positions -- the
    collapsed triangles weigh nothing and are never sampled --, a renderer that was not refitted for the mesh as loaded."""
    mesh = hq.with_uvs(hm.without_thin(hm.degenerate()))
    moved, kind = hm.collapsed(mesh)
    assert (np.bincount(kind, minlength=10)[1:6] == 4).all()
    sc, loaded = hm.scene_pair(drt, mesh)
    host, _ = hm.scene_pair(drt, mesh)
    host.refit(moved)
    order = sc.triangleOrder()
    refitted = oracle.Scene(rf.triangles(moved, mesh.nrm, mesh.uv, mesh.mat, order=order), hm.ONE_MATERIAL, [])      # as tests/test_gpu_ambient.py refits one
    refitted.nodes = rf.oracle_tree(rf.nodes(sc.m_BVHNodes, moved[order]))
    r = drt.Renderer(0)
    r.nearest(sc, np.zeros((1, 3), F))                                          # the scene is on the device before the refit
    r.refit(sc, torch.from_numpy(moved).to(DEV))
    q = pair("degenerate").q
    kinds = ("distance", "tcast", "weights", "samples", "ambient_16")
    answers = {}
    for which, scene, osc, rend in (("old", sc, loaded, renderer), ("new", host, refitted, r)):
        g, s = nr.from_product(scene), sr.from_product(scene)
        A = answers[which] = hq.restate(g, osc, s, q, kinds)
        equal(tri_near(rend.triangleDistance(sc, q.tris)), A["distance"], which + " triangleDistance")
        equal(tri_hits(rend.triangleCast(sc, q.cast_tris, q.dirs, q.tmax)), A["tcast"], which + " triangleCast")
        equal((rend.surfaceWeights(sc).view(np.uint32).reshape(-1, 2),), A["weights"], which + " surfaceWeights")
        equal(tuple(rend.sampleSurface(sc, hq.N_SAMPLES, seed=hq.SAMPLE_SEED)), A["samples"], which + " sampleSurface")
        equal(run_ambient(rend, sc, q.ao, 16), A["ambient_16"], which + " ambientOcclusion")
    old, new = answers["old"], answers["new"]
    assert hq.differing(old["distance"][1:2], new["distance"][1:2]) >= 20 and hq.differing(old["tcast"][1:2], new["tcast"][1:2]) >= 5
    assert hq.differing(old["ambient_16"], new["ambient_16"]) >= 1
    # the collapsed triangles are segments and points now: weight 0, never sampled, and they still answer distance queries
    g = nr.from_product(host)
    flat = ~(np.cross(g.e1.astype(np.float64), g.e2.astype(np.float64)) != 0).any(axis=1)
    weight = lambda A: np.diff(np.concatenate([[0], A["weights"][0].copy().view(np.uint64).reshape(-1).astype(object)]))
    assert flat.sum() == 20 and (weight(new)[flat] == 0).all() and (weight(new)[~flat] > 0).all() and (weight(old) > 0).all()
    assert not flat[new["samples"][0]].any() and flat[old["samples"][0]].any() and flat[new["distance"][3]].any()
