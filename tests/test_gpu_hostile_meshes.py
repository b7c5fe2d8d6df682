"""The mesh queries on the GPU against meshes that are not well behaved (tests/hostile_meshes.py): zero-area triangles of every kind,
slivers, needles, duplicates; the same mesh far from the origin; scaled by 2^20 and 2^-20; and scaled beyond the range in which the
rules keep their digits, where both sides go wrong in the same way (infinities, NaNs, subnormals).  Every field of every record and
every count is bit-equal to the restatement.  tests/test_hostile_meshes_ref.py shows, on the restatements alone, that these queries
meet the hard cases and where the working range ends."""
import numpy as np
import pytest

from tests import hostile_meshes as hm
from tests import hits_ref as hr
from tests import inside_ref as ir
from tests import nearest_ref as nr
from tests import overlap_ref as ov
from tests import ray_query_ref as rq
from tests import section_ref as sr
from tests import sweep_ref as sw
from tests import tri_overlap_ref as tv
from tests.test_hostile_meshes_ref import OUT_OF_RANGE, SEED

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MESHES = ["degenerate", "offset", "scaled(20)", "scaled(-20)", "scaled(%d)" % OUT_OF_RANGE[0], "scaled(%d)" % OUT_OF_RANGE[1]]
_cache = {}


@pytest.fixture(scope="module")
def renderer():
    return drt.Renderer(0)


class Pair:
    """A mesh as the product's scene and the oracle's, the queries for it and what the restatements say of them (computed once)."""

    def __init__(self, name):
        base = hm.degenerate()
        if name.startswith("scaled"):
            k = int(name[len("scaled("):-1])
            plain = pair("degenerate")
            self.mesh, self.q = hm.scaled(base, k), hm.scaled_queries(plain.q, k)
        else:
            self.mesh = base if name == "degenerate" else hm.offset(base)
        self.sc, self.osc = hm.scene_pair(drt, self.mesh)
        self.g = nr.from_oracle(self.osc)
        self.kind, self.twin = hm.kinds_in_tree_order(self.osc, self.mesh)
        if not name.startswith("scaled"):
            self.q = hm.queries(self.g, self.osc, self.kind, self.twin, SEED)
        self.answers = hm.restate(self.g, self.osc, self.q)


def pair(name):
    if name not in _cache:
        _cache[name] = Pair(name)
    return _cache[name]


def equal(got, ref, what):
    """Bit for bit on every array of two tuples (a NaN equals any NaN: a NaN's payload is not arithmetic)."""
    assert len(got) == len(ref), what
    for i, (g, r) in enumerate(zip(got, ref)):
        g, r = np.ascontiguousarray(g), np.ascontiguousarray(r)
        g = g.reshape(r.shape) if g.size == r.size else g
        assert g.shape == r.shape and g.dtype.itemsize == r.dtype.itemsize and g.dtype.kind == r.dtype.kind, (what, i, g.shape, r.shape, g.dtype, r.dtype)
        if g.size == 0:
            continue
        bits = np.uint8 if g.dtype.itemsize == 1 else np.uint32
        diff = g.view(bits) != r.view(bits)
        if g.dtype == np.float32:
            diff &= ~(np.isnan(g) & np.isnan(r))
        bad = np.nonzero(diff.reshape(len(g), -1).any(axis=1))[0]
        assert len(bad) == 0, "%s: field %d differs in %d of %d records, first %d: %r vs %r" % (what, i, len(bad), len(g), bad[0], g[bad[0]], r[bad[0]])


def fields(got, kind):
    return tuple(getattr(got, f) for f in kind._fields)


def csr(totals):
    return np.concatenate([[0], np.cumsum(totals.astype(np.int64))])


@pytest.mark.parametrize("name", MESHES)
def test_point_queries_are_bit_equal_to_the_restatement(renderer, name):
    p = pair(name)
    sc, q, A = p.sc, p.q, p.answers
    for kind, radius in (("nearest", np.inf), ("nearest_r", q.radius)):
        got = renderer.nearest(sc, q.points, radius)
        equal(fields(got, nr.Nearest), A[kind], "%s %s" % (name, kind))
        for rule in ("parity", "winding"):
            votes = A["votes_" + rule][0]
            side = np.where(votes >= 2, np.float32(-1), np.float32(1)).astype(np.float32)
            equal(fields(renderer.signedDistance(sc, q.points, radius, rule=rule), nr.Nearest), A[kind][:5] + (side,), "%s signedDistance %s %s" % (name, kind, rule))
    for rule in ("parity", "winding"):
        votes = A["votes_" + rule][0]
        got = renderer.inside(sc, q.points, rule=rule, votes=True)
        assert got.dtype == votes.dtype and (got == votes).all(), "%s %s: %d votes differ" % (name, rule, (got != votes).sum())
        assert (renderer.inside(sc, q.points, rule=rule) == (votes >= 2)).all()
    got = renderer.kNearest(sc, q.points, k=hm.K_NEAR)
    equal((got.d2, got.prim, got.u, got.v, got.point.reshape(-1, 3), got.side, got.count.view(np.uint32)), A["k_nearest"], name + " kNearest")
    got = renderer.withinRadius(sc, q.points, q.radius)
    totals = A["within"][6]
    assert (got.splits == csr(totals)).all(), name
    equal((got.d2, got.prim, got.u, got.v, got.point.reshape(-1, 3), got.side), A["within"][:6], name + " withinRadius")


@pytest.mark.parametrize("name", MESHES)
def test_ray_queries_are_bit_equal_to_the_restatement(renderer, name):
    p = pair(name)
    sc, A = p.sc, p.answers
    org, dirs, tmin, tmax = p.q.rays
    got = renderer.crossings(sc, org, dirs, tmin, tmax)
    equal((got.count, got.winding), A["crossings"], name + " crossings")
    totals = A["hits"][4]
    got = renderer.listHits(sc, org, dirs, tmin, tmax)
    assert (got.splits == csr(totals)).all(), name
    equal((got.t, got.prim, got.u, got.v), A["hits"][:4], name + " listHits")
    got = renderer.firstHits(sc, org, dirs, tmin, tmax, k=3)
    equal((got.t, got.prim, got.u, got.v), tuple(hr.list_hits(p.osc, org, dirs, tmin, tmax, 3)[0]), name + " firstHits")
    assert (got.count == totals).all()
    got = renderer.traceRays(sc, org, dirs, tmin, tmax)
    equal((got.t, got.prim, got.u, got.v), A["closest"], name + " traceRays")
    got = renderer.occluded(sc, org, dirs, tmin, tmax)
    assert got.dtype == bool and (got == A["occluded"][0]).all(), name


@pytest.mark.parametrize("name", MESHES)
def test_sphere_casts_are_bit_equal_to_the_restatement(renderer, name):
    p = pair(name)
    equal(fields(renderer.sphereCast(p.sc, *p.q.casts), sw.SweepHits), p.answers["cast"], name + " sphereCast")


@pytest.mark.parametrize("name", MESHES)
def test_overlap_queries_are_bit_equal_to_the_restatement(renderer, name):
    p = pair(name)
    sc, q, A = p.sc, p.q, p.answers
    for kind, queries, lists, any_ in (("boxes", q.boxes, renderer.overlapBoxes, renderer.overlapsAny), ("tris", q.tris, renderer.overlapTriangles, renderer.intersectsAny)):
        prims, totals = A[kind]
        got = lists(sc, queries)
        assert (got.splits == csr(totals)).all() and got.prim.dtype == np.int32 and (got.prim == prims).all(), (name, kind)
        hit = any_(sc, queries)
        assert hit.dtype == np.bool_ and (hit == (totals > 0)).all(), (name, kind)
        table = lists(sc, queries, k=2)
        assert (table.count.view(np.uint32) == totals).all(), (name, kind)
        rows = np.full((len(totals), 2), -1, np.int32)
        start = csr(totals)
        for j in range(2):
            has = totals > j
            rows[has, j] = prims[start[:-1][has] + j]
        assert (table.prim == rows).all(), (name, kind)


@pytest.mark.parametrize("name", MESHES)
def test_plane_sections_are_bit_equal_to_the_restatement(renderer, name):
    p = pair(name)
    planes = p.q.planes
    rp, rprim, rq_, rcode, totals = p.answers["planes"]
    got = renderer.planeSections(p.sc, planes)
    assert (got.splits == csr(totals)).all(), name
    equal((got.p, got.prim, got.q, got.code), (rp, rprim, rq_, rcode), name + " planeSections")
    hit = renderer.cutsAny(p.sc, planes)
    assert hit.dtype == np.bool_ and (hit == (totals > 0)).all(), name


def test_the_hard_cases_are_in_these_answers():
    """The conditions of tests/test_hostile_meshes_ref.py, on the answers compared above: the same seed gives the same queries."""
    from tests import test_hostile_meshes_ref as ref
    for name in ("degenerate", "offset"):
        p, c = pair(name), ref._case(name)
        for f in hm.Queries._fields:
            a, b = getattr(p.q, f), getattr(c.q, f)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) if isinstance(a, tuple) else a.tobytes() == b.tobytes(), (name, f)
        ref.test_coverage_conditions(c)


def _run_hand(renderer):
    def run(kind, sc, g, *a):
        if kind == "nearest":
            got = renderer.nearest(sc, *a)
            equal(fields(got, nr.Nearest), tuple(nr.nearest(g, *a)), "hand nearest")
            return got
        if kind == "cast":
            got = renderer.sphereCast(sc, *a)
            equal(fields(got, sw.SweepHits), tuple(sw.sphere_cast(g, *a)), "hand cast")
            return got
        if kind == "boxes":
            return renderer.overlapBoxes(sc, a[0], k=1).count
        if kind == "tris":
            return renderer.overlapTriangles(sc, a[0], k=1).count
        got = renderer.planeSections(sc, a[0])
        rec = np.zeros(len(got.prim), sr.SECTION)
        rec["p"], rec["q"], rec["prim"], rec["code"] = got.p, got.q, got.prim, got.code
        return rec, np.diff(got.splits).astype(np.uint32)
    return run


def test_hand_cases_on_a_segment_a_point_and_a_triangle_beside_a_zero_area_one(renderer):
    """The values derived on paper in tests/hostile_meshes.py, through the GPU."""
    def geometry(name):
        pos = hm.HAND_SCENES[name]
        n = len(pos)
        sc, osc = rq.programmatic_scene(drt, pos, np.tile(np.float32([0, 0, 1]), (n, 3, 1)), np.zeros((n, 3, 2), np.float32), np.zeros(n, np.int32), hm.ONE_MATERIAL, [],
                                        hm.LEAF, hm.BINS)
        return sc, nr.from_oracle(osc)
    hm.check_hand_cases(geometry, _run_hand(renderer))


def test_self_intersections_of_the_degenerate_mesh(renderer):
    """Duplicates share every vertex position and are not pairs; a zero-area triangle is one where it touches another."""
    p = pair("degenerate")
    want = tv.self_pairs(p.g, p.osc.tris["p"])
    got = renderer.selfIntersections(p.sc)
    assert got.dtype == np.int32 and got.shape == want.shape and (got == want).all()
    assert len(want) >= 10 and np.isin(p.kind[want], hm.ZERO_AREA).any()
    assert not (p.twin[want[:, 0]] == want[:, 1]).any()


def test_refit_into_degeneracy(renderer):
    """The mesh is loaded without its zero-area triangles, slivers and needles; a refit then collapses 20 triangles (four of each
    kind) and moves 10 onto others.  The refitted renderer answers for the host scene refitted with the same positions, a renderer
    that was not refitted for the mesh as loaded."""
    mesh = hm.without_thin(hm.degenerate())
    moved, kind = hm.collapsed(mesh)
    assert (np.bincount(kind, minlength=10)[1:6] == 4).all() and (kind == hm.DUPLICATE).sum() == 30 and not np.isin(mesh.kind, hm.THIN).any()
    sc, _ = hm.scene_pair(drt, mesh)
    host, _ = hm.scene_pair(drt, mesh)
    host.refit(moved)
    r = drt.Renderer(0)
    r.nearest(sc, np.zeros((1, 3), np.float32))                                 # the scene is on the device before the refit
    r.refit(sc, torch.from_numpy(moved).to(DEV))
    base = pair("degenerate")
    q = base.q
    answers = {}
    for which, scene, rend in (("old", sc, renderer), ("new", host, r)):
        g, osc = nr.from_product(scene), ir.product_scene(scene)
        answers[which] = (tuple(nr.nearest(g, q.points)), tuple(sw.sphere_cast(g, *q.casts)))
        _, totals = ov.overlap(g, q.boxes, 0)
        prims, _ = ov.overlap(g, q.boxes, totals)
        rec, ptotals = sr.whole(g, q.planes)
        votes = ir.votes(osc, q.points)
        equal(fields(rend.nearest(sc, q.points), nr.Nearest), answers[which][0], which + " nearest")
        equal(fields(rend.sphereCast(sc, *q.casts), sw.SweepHits), answers[which][1], which + " sphereCast")
        got = rend.overlapBoxes(sc, q.boxes)
        assert (got.splits == csr(totals)).all() and (got.prim == prims).all(), which
        got = rend.planeSections(sc, q.planes)
        assert (got.splits == csr(ptotals)).all(), which
        equal((got.p, got.prim, got.q, got.code), (rec["p"], rec["prim"], rec["q"], rec["code"]), which + " planeSections")
        got = rend.inside(sc, q.points, votes=True)
        assert (got == votes).all(), "%s: %d votes differ" % (which, (got != votes).sum())
        answers[which] += (votes,)
    old, new = answers["old"], answers["new"]
    assert (old[0][1].view(np.uint32) != new[0][1].view(np.uint32)).sum() >= 20 and (old[1][1] != new[1][1]).sum() >= 5
    # the collapsed triangles answer as the segments and points they now are
    g = nr.from_product(host)
    flat = ~(np.cross(g.e1.astype(np.float64), g.e2.astype(np.float64)) != 0).any(axis=1)
    assert flat.sum() == 20 and flat[new[0][2][new[0][2] >= 0]].any()


@pytest.mark.parametrize("name", ["degenerate", "offset"])
def test_a_small_frame_is_the_oracle_s_image(renderer, name):
    """96 x 64, 2 frames, bounce limit 4: the path tracer's leaf loop meets the same triangles."""
    import oracle
    from tests.test_gpu_parity import compare, settings_pair
    p = pair(name)
    pos = np.float32([0.0, 0.5, 9.0]) + (hm.OFFSET if name == "offset" else np.float32(0))
    fwd = (0.0, -0.05, -1.0)
    cam = drt.Camera(tuple(float(x) for x in pos))
    cam.m_Forward_dir = np.array(fwd, np.float32)
    s, o = settings_pair(ray_bounce_limit=4)
    r = drt.Renderer(0)
    r.m_RendererSettings = s
    r.ResizeBuffer(96, 64)
    r.resetAccumulationBuffer()
    r.RenderBatch(cam, p.sc, 2)
    ref, _, _ = oracle.render(p.osc, oracle.default_camera(position=tuple(float(x) for x in pos), forward=fwd), o, 96, 64, 1, 2)
    img = r.GetRenderTargetImage()
    compare(img, ref, name)
    assert (np.abs(ref[..., :3] - ref[0, 0, :3]).max(axis=-1) > 0.02).mean() > 0.05        # the mesh is in the picture
