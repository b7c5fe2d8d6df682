"""Cuts, curves, contours and topology on the GPU against surfaces that are not well behaved (tests/hostile_surfaces.py): a closed
sphere whose split edges are closed by zero-area and sliver caps, the same sphere with so many caps that they collide into
non-manifold edges and with holes whose rotations run into them, a band with exact coordinates whose caps all have exactly zero area,
and the unconnected degenerate soup -- each plain, moved to (4096, -8192, 16384), scaled by 2^20 and 2^-20, at the fringe scales where
the intersection records are lost one by one to subnormals and infinities, and beyond the range.  Every record, slot, label, count and
term is bit-equal to the restatement (a NaN equals a NaN); the float64 sums built on them are checked against math.fsum of the same
terms.  tests/test_hostile_surfaces_ref.py shows, on the restatements alone, that these cases contain the hard ones."""
import math
import time

import numpy as np
import pytest

from tests import contour_ref as cr
from tests import contour_scenes as cs
from tests import curve_ref as cu
from tests import hostile_meshes as hm
from tests import hostile_surfaces as hs
from tests import intersect_ref as ix
from tests import nearest_ref as nr
from tests import section_ref as sr
from tests import topology_ref as tr
from tests.test_gpu_hostile_meshes import equal

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

from tests import test_gpu_contour as tcont  # noqa: E402  (these import the product themselves)
from tests import test_gpu_curve as tcurve  # noqa: E402
from tests import test_gpu_intersect as tcut  # noqa: E402
from tests import test_gpu_topology as ttopo  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = [(name, variant) for name in hs.MESHES for variant in hs.VARIANTS]
_scenes = {}
_began = time.time()


@pytest.fixture(scope="module")
def renderer():
    return drt.Renderer(0)


def product_scene(c):
    """The product's scene of a case, built once; its tree is the oracle's, triangle for triangle."""
    key = (c.name, c.variant)
    if key not in _scenes:
        sc = hm.scene_pair(drt, c.mesh)[0] if c.name == "soup" else cs.flat_scene(drt, c.pos)[0]
        assert cs.tree_positions(sc).tobytes() == c.tree.tobytes(), key
        _scenes[key] = sc
    return _scenes[key]


def csr(totals):
    return np.concatenate([[0], np.cumsum(np.asarray(totals).astype(np.int64))])


def same_words(got, want, what):
    """Records as int32 words [M, 8]: the integers exactly, the floats bit for bit but for a NaN's payload."""
    got, want = np.ascontiguousarray(got).view(np.int32).reshape(-1, 8), np.ascontiguousarray(want).view(np.int32).reshape(-1, 8)
    flt = [0, 1, 2, 4, 5, 6]
    equal((got[:, flt].copy().view(np.float32), got[:, [3, 7]].copy()), (want[:, flt].copy().view(np.float32), want[:, [3, 7]].copy()), what)


def same_lists(got, want, what):
    got = tuple(x.cpu().numpy() if torch.is_tensor(x) else x for x in got)
    assert all(a.dtype == b.dtype for a, b in zip(got, want)), what
    equal(tuple(x.view(np.uint8) if x.dtype == bool else x for x in got), tuple(x.view(np.uint8) if x.dtype == bool else x for x in want), what)


def check_sums(what, got, want, mass):
    """A float64 sum of the product against math.fsum of the same terms -- the exact sum, rounded once -- by the project's criterion
    (tests/test_gpu_contour.py check_areas, tests/test_gpu_topology.py check_measures), with mass = the sum of the absolute terms:
      everywhere               |got - want| <= 1e-12 * mass
      where mass <= 20 |want|  |got - want| <= 1e-12 * |want|
      mass == 0                got == 0 exactly
    check_areas argues its bound from chains of at most 64 records; the ranges here hold thousands.  What is owed does not grow with the
    length: dustraytracer_amd._segment_sums keeps, beside the running sum over ALL terms, the running sum of every step's rounding error
    (Knuth's two-sum: exact), so the two differences at a range's ends add up to the range's own sum but for the roundings of those
    two subtractions and their sum -- three units of 2^-53 of the range's mass -- and for the roundings of the error sum itself, which
    are 2^-53 of 2^-53 of the running total per term: second order.  The terms agree to two units of 2^-53 of their own mass (a
    three-term dot product in another order; every product of two float32 values is exact in float64, so a fused multiply-add changes
    nothing).  About 6e-16 of the mass is owed; 1e-12 is the project's figure.  The numpy path of CurveList.lengths sums a chain left to
    right: m * 2^-53 of the sum for m records, 1e-13 at a thousand.  Returns the largest |got - want| / mass."""
    got, want, mass = (np.asarray(x, np.float64).reshape(-1) for x in (got, want, mass))
    assert got.shape == want.shape, what
    fine = np.isfinite(want)
    assert (np.isnan(got) == np.isnan(want)).all() and (got[~fine & ~np.isnan(want)] == want[~fine & ~np.isnan(want)]).all(), what
    diff = np.abs(got[fine] - want[fine])
    w, m = np.abs(want[fine]), mass[fine]
    some, owed = m > 0, (m > 0) & (m <= 20 * w)
    ratio = float((diff[some] / m[some]).max(initial=0))
    print("%s: %d sums, %d well conditioned; largest |got - want| / mass %.3e, / |want| where well conditioned %.3e"
          % (what, len(got), owed.sum(), ratio, (diff[owed] / w[owed]).max(initial=0)))
    assert (diff[some] <= 1e-12 * m[some]).all(), what
    assert (diff[owed] <= 1e-12 * w[owed]).all(), what
    assert (got[fine][~some] == 0).all(), what
    return ratio


def fsums(term, at):
    """math.fsum of term[at[i]:at[i + 1]] and of its absolute values."""
    term = np.asarray(term, np.float64)
    return (np.array([math.fsum(term[a:b]) for a, b in zip(at[:-1], at[1:])], np.float64),
            np.array([math.fsum(np.abs(term[a:b])) for a, b in zip(at[:-1], at[1:])], np.float64))


def area_terms(planes, p, q, owner):
    """The terms of sectionAreas / ContourList.areas from the records the device returned: (dot(n / |n|, cross(p, q)) per record,
    the sum of the three absolute products per record), float64."""
    nn = np.asarray(planes, np.float32)[:, 0:3].astype(np.float64)
    length = np.sqrt((nn * nn).sum(axis=1, keepdims=True))
    unit = np.where(length > 0, nn / np.where(length > 0, length, 1), 0)
    three = unit[owner] * np.cross(np.asarray(p, np.float32).astype(np.float64), np.asarray(q, np.float32).astype(np.float64))
    return three.sum(axis=1), np.abs(three).sum(axis=1)


@pytest.mark.parametrize("name,variant", CASES)
def test_intersection_records_are_bit_equal_to_the_restatement(renderer, name, variant):
    c = hs.case(name, variant)
    sc, q = product_scene(c), c.q.tris
    splits, rec = hs.restate(c, ("cut",))["cut"]
    totals = np.diff(splits).astype(np.uint32)
    n = len(q)
    print("%s %s: %d triangles, %d queries, %d records over %d queries" % (name, variant, len(c.tree), n, len(rec), (totals > 0).sum()))
    got = renderer.intersectTriangles(sc, q)
    assert (got.splits == splits).all(), (name, variant)
    same_words(tcut.as_words(got), rec, "%s %s intersectTriangles" % (name, variant))
    # the entry point itself: ragged capacities, zeros included, on sentinel-filled buffers; the miss record behind a short list
    rng = np.random.default_rng(5)
    caps = rng.integers(0, 7, n)
    caps[rng.integers(0, n, n // 8)] = 0
    assert (caps == 0).sum() >= n // 16 and ((caps > totals).any() or len(rec) == 0)
    out, counts = tcut.run_raw(renderer, sc, q, csr(caps), int(caps.sum()), int(caps.sum()))
    same_words(out, tcut.cut(tcut.words(rec), totals, caps), "%s %s ragged capacities" % (name, variant))
    assert (counts.view(np.uint32) == totals).all()
    # a pure count
    _, counts = tcut.run_raw(renderer, sc, q, np.zeros(n + 1), 0, 0, with_out=False)
    assert (counts.view(np.uint32) == totals).all()
    if name in ("soup", "capped_dense"):
        pairs, p, e, code = hs.restate(c, ("self",))["self"]
        cuts = renderer.selfIntersectionSegments(sc)
        print("%s %s: %d self-intersection segments" % (name, variant, len(pairs)))
        equal((cuts.pairs, cuts.p, cuts.q, cuts.code), (pairs, p, e, code), "%s %s selfIntersectionSegments" % (name, variant))


def length_terms(p, q):
    d = np.asarray(q, np.float32).astype(np.float64) - np.asarray(p, np.float32).astype(np.float64)
    return np.sqrt((d * d).sum(axis=1))


@pytest.mark.parametrize("name,variant", CASES)
def test_curves_are_bit_equal_to_the_restatement(renderer, name, variant):
    c = hs.case(name, variant)
    sc, q = product_scene(c), c.q.tris
    A = hs.restate(c, ("curve",))
    (splits, rec), (want, want_counts), query_adj = A["cut"], A["curve"], A["query_adj"]
    total = len(rec)
    print("%s %s: %d records, counts %s, statuses %s" % (name, variant, total, want_counts.tolist(), hs.curve_status(c).tolist()))
    assert (sc.edgeAdjacency().reshape(-1) == A["adj"]).all()
    if total:                                                                  # (beyond the range there may be no record left)
        slots, counts = tcurve.run_raw(renderer, sc, rec, splits, query_adj)
        assert slots.tobytes() == tcurve.padded(want, total + 8).tobytes() and counts.tobytes() == want_counts.tobytes(), (name, variant)
    lists = tcurve.expected_lists(rec, splits, want)
    got = renderer.intersectionCurves(sc, q)
    assert isinstance(got, drt.CurveList)
    same_lists(got, lists, "%s %s intersectionCurves" % (name, variant))
    dev = renderer.intersectionCurves(sc, torch.from_numpy(q).to(DEV))
    same_lists(dev, lists, "%s %s intersectionCurves on the device" % (name, variant))
    # lengths: every term is positive, so the mass is the sum
    at = lists[0].astype(np.int64)
    sums, mass = fsums(length_terms(got.p, got.q), at)
    check_sums("%s %s CurveList.lengths (numpy)" % (name, variant), got.lengths(), sums, mass)
    check_sums("%s %s CurveList.lengths (device)" % (name, variant), dev.lengths().cpu().numpy(), sums, mass)


@pytest.mark.parametrize("name,variant", CASES)
def test_sections_and_contours_are_bit_equal_to_the_restatement(renderer, name, variant):
    c = hs.case(name, variant)
    sc, planes = product_scene(c), c.q.planes
    A = hs.restate(c, ("contour",))
    (rec, totals), (want, want_chains) = A["section"], A["contour"]
    splits = csr(totals)
    print("%s %s: %d planes, %d records, %d chains (%d closed), statuses %s"
          % (name, variant, len(planes), len(rec), want_chains[:, 0].sum(), want_chains[:, 1].sum(), hs.contour_status(c).tolist()))
    sec = renderer.planeSections(sc, planes)
    if name != "soup":                                                         # (tests/test_gpu_hostile_meshes.py compares the soup's)
        assert (sec.splits == splits).all(), (name, variant)
        equal((sec.p, sec.prim, sec.q, sec.code), (rec["p"], rec["prim"], rec["q"], rec["code"]), "%s %s planeSections" % (name, variant))
    slots, chains = tcont.run_raw(renderer, sc, rec, splits)
    assert slots.tobytes() == want.tobytes() and (chains == want_chains).all(), (name, variant)
    lists = tcont.expected_lists(rec, want, want_chains)
    got = renderer.contours(sc, planes)
    assert isinstance(got, drt.ContourList)
    same_lists(got, lists, "%s %s contours" % (name, variant))
    same_lists(renderer.chainSections(sc, sec), lists, "%s %s chainSections" % (name, variant))
    # the float64 sums, from the records the device returned
    owner = np.repeat(np.arange(len(planes)), np.diff(sec.splits))
    term, absolute = area_terms(planes, sec.p, sec.q, owner)
    sums, _ = fsums(term, sec.splits.astype(np.int64))
    _, mass = fsums(absolute, sec.splits.astype(np.int64))
    check_sums("%s %s sectionAreas" % (name, variant), renderer.sectionAreas(sc, planes), 0.5 * sums, 0.5 * mass)
    chain_plane = np.repeat(np.arange(len(planes)), np.diff(got.splits))
    owner = np.repeat(chain_plane, np.diff(got.chain_splits))
    term, absolute = area_terms(planes, got.p, got.q, owner)
    at = got.chain_splits.astype(np.int64)
    sums, _ = fsums(term, at)
    _, mass = fsums(absolute, at)
    areas = got.areas()
    assert np.isnan(areas[~got.closed]).all() and np.isfinite(areas[got.closed]).all()
    check_sums("%s %s ContourList.areas" % (name, variant), areas, np.where(got.closed, 0.5 * sums, np.nan), 0.5 * mass)


@pytest.mark.parametrize("name,variant", CASES)
def test_topology_is_bit_equal_to_the_restatement(renderer, name, variant):
    c = hs.case(name, variant)
    sc = product_scene(c)
    A = hs.restate(c, ("topology",))
    adj, label, counts, (want, want_counts) = A["adj"], A["labels"], A["counts"], A["loops"]
    n, m = len(label), len(want)
    print("%s %s: %d triangles, %s shells / open / bad, %s records / loops / closed" % (name, variant, n, counts.tolist(), want_counts.tolist()))
    assert (sc.edgeAdjacency().reshape(-1) == adj).all()
    fresh = drt.Renderer(0)                                                     # (nothing is cached: the labelling runs here)
    got, got_counts = ttopo.run_labels(fresh, sc, n)
    assert got.tobytes() == label.tobytes() and (got_counts == counts).all(), (name, variant)
    steps = fresh.topologySteps()
    assert steps[0] >= steps[1] >= steps[2] >= 1 and steps[0] > steps[1], steps
    again, none = ttopo.run_labels(fresh, sc, n, with_counts=False)             # the second call is served from the cache
    assert none is None and again.tobytes() == label.tobytes() and fresh.topologySteps() == steps
    nothing, only_counts = ttopo.run_loops(fresh, sc, None)
    assert len(nothing) == 0 and (only_counts == want_counts).all(), (name, variant)
    if m:
        slots, loop_counts = ttopo.run_loops(fresh, sc, m)
        assert slots.tobytes() == want.tobytes() and (loop_counts == want_counts).all(), (name, variant)
    term, want_term = ttopo.device_terms(fresh, sc)
    equal((term["c"], term["w"]), (want_term["c"], want_term["w"]), "%s %s terms of the device's records" % (name, variant))
    equal((term["c"], term["w"]), (A["terms"]["c"], A["terms"]["w"]), "%s %s terms of the positions" % (name, variant))
    shells = ttopo.expected_shells(adj, label)
    assert ttopo.same(fresh.shells(sc), shells) and ttopo.same(fresh.boundaryLoops(sc), ttopo.expected_loops(want, shells[1])), (name, variant)
    # shellMeasures against math.fsum of the same terms (topology_ref.measures)
    ms = fresh.shellMeasures(sc)
    area, volume, vector, m_area, m_volume, m_vector = tr.measures(term, shells[1], shells[2])
    for what, g, w, mass in (("area", ms.area, area, m_area), ("volume", ms.volume, volume, m_volume), ("area_vector", ms.area_vector, vector, m_vector)):
        check_sums("%s %s shellMeasures %s" % (name, variant, what), g, w, mass)


@pytest.mark.parametrize("name", ["capped_sparse", "capped_band"])
def test_the_measures_of_a_manifold_mesh_scale_exactly(renderer, name):
    """A power of two commutes with every float64 operation of the terms and of the sums (nothing leaves float64's range), and the
    tree, the shells and so the order of the sums are the same: c and the area vector carry 2^(2k), w and the volume 2^(3k), and the
    area -- half the sum of |c| -- 2^(2k) like the area vector, bit for bit."""
    plain = renderer.shellMeasures(product_scene(hs.case(name, "plain")))
    assert len(plain.area) == 1 and plain.area[0] > 0
    for k in (20, -20):
        got = renderer.shellMeasures(product_scene(hs.case(name, "scaled(%d)" % k)))
        assert got.area.tobytes() == (plain.area * 2.0 ** (2 * k)).tobytes(), (name, k)
        assert got.area_vector.tobytes() == (plain.area_vector * 2.0 ** (2 * k)).tobytes(), (name, k)
        assert got.volume.tobytes() == (plain.volume * 2.0 ** (3 * k)).tobytes(), (name, k)


def _restate_refit(c, host, adj):
    """The contours and curves of the case's queries on the refitted host scene, chained with the table `adj`."""
    g = nr.from_product(host)
    rec, totals = sr.whole(g, c.q.planes)
    contour = tcont.expected_lists(rec, *cr.chain(adj, rec, csr(totals)))
    splits, cut = ix.whole(g, c.q.tris)
    w = cut.view(np.int32)
    slots, _ = cu.chain(adj, cu.tri_adjacency(c.q.tris), w[:, 3], w[:, 7], splits, len(c.tree))
    return contour, tcurve.expected_lists(cut, splits, slots)


def test_a_refit_into_degeneracy_with_and_without_a_new_table(renderer):
    """A host refit collapses 20 further triangles of capped_sparse and moves ten vertices onto neighbours (hostile_surfaces.collapsed):
    the re-upload brings the refitted scene's own adjacency.  A device-only refit with the same positions keeps the old table, as
    drt.h says: its records are the new ones, chained by the old adjacency."""
    c = hs.case("capped_sparse", "plain")
    A = hs.restate(c, ("curve", "contour", "topology"))
    new = hs.collapsed(c)
    sc = cs.flat_scene(drt, c.pos)[0]
    r = drt.Renderer(0)
    before = (r.contours(sc, c.q.planes), r.intersectionCurves(sc, c.q.tris), r.shells(sc), r.boundaryLoops(sc))
    same_lists(before[0], tcont.expected_lists(A["section"][0], *A["contour"]), "before the refit")
    sc.refit(new)
    tree = cs.tree_positions(sc)
    adj = cr.adjacency(tree)
    label = tr.labels(adj)
    want, want_counts = tr.loops(adj)
    assert (sc.edgeAdjacency().reshape(-1) == adj).all() and (adj != A["adj"]).sum() >= 60
    assert label.tobytes() != A["labels"].tobytes() and len(want) > 0 and ((want["flags"] >> 1) == cr.NON_MANIFOLD).any()
    shells = ttopo.expected_shells(adj, label)
    assert ttopo.same(r.shells(sc), shells) and ttopo.same(r.boundaryLoops(sc), ttopo.expected_loops(want, shells[1]))
    contour, curve = _restate_refit(c, sc, adj)
    after = (r.contours(sc, c.q.planes), r.intersectionCurves(sc, c.q.tris))
    same_lists(after[0], contour, "contours after the host refit")
    same_lists(after[1], curve, "curves after the host refit")
    assert any(a.tobytes() != b.tobytes() for a, b in zip(after[0], before[0])) and any(a.tobytes() != b.tobytes() for a, b in zip(after[1], before[1]))
    # device only: the scene as loaded, on the device before the refit
    old = cs.flat_scene(drt, c.pos)[0]
    r2 = drt.Renderer(0)
    same_lists(r2.contours(old, c.q.planes), tcont.expected_lists(A["section"][0], *A["contour"]), "before the device refit")
    r2.refit(old, torch.from_numpy(new).to(DEV))
    contour_old, curve_old = _restate_refit(c, sc, A["adj"])                   # the NEW records by the OLD table
    same_lists(r2.contours(old, c.q.planes), contour_old, "contours after the device refit")
    same_lists(r2.intersectionCurves(old, c.q.tris), curve_old, "curves after the device refit")
    assert ttopo.same(r2.shells(old), ttopo.expected_shells(A["adj"], A["labels"]))
    assert any(a.tobytes() != b.tobytes() for a, b in zip(contour_old, contour))


def test_the_hard_cases_are_in_these_answers():
    """The conditions of tests/test_hostile_surfaces_ref.py on the very answers compared above: hostile_surfaces keeps one Case per
    mesh and variant, so these are the same arrays."""
    from tests import test_hostile_surfaces_ref as ref
    for variant in ref.FULL:
        ref.test_capped_sparse_is_one_watertight_shell(variant)
    ref.test_capped_dense_falls_apart_and_its_holes_rotate_into_bad_edges()
    ref.test_every_exit_status_comes_from_geometry()
    ref.test_the_tool_curve_on_capped_sparse()
    for variant in ("plain", "offset"):
        ref.test_the_band_s_sections_close_through_zero_length_records(variant)
        for name in hs.CAPPED_MESHES:
            ref.test_the_aimed_triangles_meet_ties(name, variant)
    for name in hs.MESHES:
        ref.test_the_fringe_scales_lose_some_records_and_the_far_ones_nearly_all(name)
    print("tests/test_gpu_hostile_surfaces.py: %.1f s since its import" % (time.time() - _began))
