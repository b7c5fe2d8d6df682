"""Crossing counts, inside votes and signed distance on the GPU (drt_renderer_crossings / _inside / _signed_distance,
kernel_crossings.hip): every field of every result bit-equal to the restatement in tests/inside_ref.py -- over scenes, rules,
radii, a tree deeper than the LDS stack, batch shapes, a refitted device copy and the torch path -- and the renderer's state
untouched, and the error codes of include/drt.h."""
import numpy as np
import pytest

import oracle
from tests import inside_ref as ir
from tests import nearest_ref as nr
from tests import ray_query_ref as rq
from tests.scenes import SCENES, scene_path

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RULE_NAMES = ["parity", "winding"]
SCENE_NAMES = ["cube", "torus", "cornell_box", "chain"]
_cache = {}


@pytest.fixture(scope="module")
def renderer():
    return drt.Renderer(0)


def scene_pair(name):
    """(product scene, oracle scene) with the same tree: the cube with leaf size 2, the torus with 4, cornell_box with the editor's
    tree, ray_query_ref.degenerate_chain(62) with one triangle per leaf (a tree deeper than the 16 LDS levels)."""
    if name not in _cache:
        if name == "cornell_box":
            sc = drt.Scene()
            sc.loadGLTFmodel(scene_path(name))
            b = drt.BVHBuilder()
            b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
            b.buildIterative(sc)
            _cache[name] = (sc, oracle.Scene.load_glb(scene_path(name)).build_bvh(20, 8))
        elif name == "chain":
            _cache[name] = rq.programmatic_scene(drt, *rq.degenerate_chain(62), 1, 2)
        else:
            pos, leaf = {"cube": (ir.cube(), 2), "torus": (ir.torus(), 4), "wedge": (ir.wedge(), 4)}[name]
            _cache[name] = rq.programmatic_scene(drt, *ir.streams(pos), leaf, 8)
    return _cache[name]


def assert_fields_equal(got, ref, what):
    """Bit for bit on every field of two namedtuples of arrays."""
    for field in ref._fields:
        g, r = np.ascontiguousarray(getattr(got, field)), np.ascontiguousarray(getattr(ref, field))
        assert g.shape == r.shape and g.dtype == r.dtype, (what, field, g.shape, r.shape, g.dtype, r.dtype)
        bad = np.nonzero((g.view(np.uint32) != r.view(np.uint32)).reshape(len(g), -1).any(axis=1))[0]
        assert len(bad) == 0, "%s: %s differs on %d of %d, first %d: %r vs %r" % (what, field, len(bad), len(g), bad[0], g[bad[0]], r[bad[0]])


def assert_votes_equal(got, ref, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, got.shape)
    bad = np.nonzero(got != ref)[0]
    assert len(bad) == 0, "%s: %d of %d votes differ, first %d: %r vs %r" % (what, len(bad), len(ref), bad[0], got[bad[0]], ref[bad[0]])


def ray_set(name, osc, seed):
    """(org, dirs, tmin, tmax): rays from the surfaces, random intervals (NaN, negative, zero and infinite bounds among them), the
    vote's own directions, and rays with a NaN origin, a NaN direction and a NaN interval."""
    rng = np.random.default_rng(seed)
    o1, d1 = rq.surface_rays(osc, 500, rng)
    o2, d2, tmin2, tmax2 = rq.interval_rays(osc, 700, rng)
    o3 = nr.box_points(nr.from_oracle(osc), 300, rng, 1.3)
    d3 = ir.DIRS[rng.integers(0, 3, 300)]
    o4, d4 = o1[:6].copy(), d1[:6].copy()
    o4[0, 0] = o4[1, 2] = d4[2, 1] = d4[3, 0] = np.nan
    tmin4, tmax4 = np.float32([0, 0, 0, 0, np.nan, 0]), np.float32([np.inf, np.inf, np.inf, np.inf, np.inf, np.nan])
    org, dirs = np.concatenate([o1, o2, o3, o4]), np.concatenate([d1, d2, d3, d4])
    tmin = np.concatenate([np.zeros(500, np.float32), tmin2, np.zeros(300, np.float32), tmin4])
    tmax = np.concatenate([np.full(500, np.inf, np.float32), tmax2, np.full(300, np.inf, np.float32), tmax4])
    if name == "chain":
        # along the chain in both directions: towards -x the near leaves are the farther children, so they wait on the stack
        k = 200
        oo = np.concatenate([np.tile(np.float32([-3, 0, 0]), (k, 1)), np.tile(np.float32([2.0 ** 62, 0, 0]), (k, 1))])
        dd = np.concatenate([np.ones((2 * k, 1), np.float32), rng.normal(scale=0.02, size=(2 * k, 2)).astype(np.float32)], axis=1)
        dd[k:, 0] = -1
        org, dirs = np.concatenate([org, oo]), np.concatenate([dirs, dd.astype(np.float32)])
        tmin, tmax = np.concatenate([tmin, np.zeros(2 * k, np.float32)]), np.concatenate([tmax, np.full(2 * k, np.inf, np.float32)])
    return org.astype(np.float32), dirs.astype(np.float32), tmin.astype(np.float32), tmax.astype(np.float32)


def point_set(g, n, seed):
    """About n points for a nearest_ref.Geometry: near and on surfaces, at vertices and edge midpoints (no defined answer, but one
    answer), in the scene's box, in a larger box, and three with a NaN coordinate."""
    rng = np.random.default_rng(seed)
    pts = np.concatenate([nr.point_sets(g, n, rng), nr.box_points(g, n // 2, rng, 1.2)])
    bad = np.repeat(pts[:1], 3, axis=0)
    bad[np.arange(3), np.arange(3)] = np.nan
    return np.concatenate([pts, bad]).astype(np.float32)


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_crossings_bit_equal_to_the_restatement(renderer, name):
    sc, osc = scene_pair(name)
    org, dirs, tmin, tmax = ray_set(name, osc, 7)
    depth = np.zeros(len(org), np.int64)
    ref = ir.crossings(osc, org, dirs, tmin, tmax, depth=depth)
    assert ref.count.max() >= 2 and (ref.winding > 0).any() and (ref.winding < 0).any()
    if name == "chain":
        assert sc.bvh_depth > 16 and depth.max() > 16 and ref.count.max() > 16   # the levels beyond the 16 in LDS run through the HBM stack
    got = renderer.crossings(sc, org, dirs, tmin, tmax)
    assert isinstance(got, drt.Crossings)
    assert_fields_equal(got, ref, name)
    bad = np.isnan(org).any(axis=1) | np.isnan(dirs).any(axis=1) | np.isnan(tmin) | np.isnan(tmax)
    assert bad.sum() >= 6 and not got.count[bad].any() and not got.winding[bad].any()
    # packed rays, and the default interval (0, +inf)
    packed = np.concatenate([org, tmin[:, None], dirs, tmax[:, None]], axis=1).astype(np.float32)
    assert_fields_equal(renderer.crossings(sc, packed), ref, name + " packed")
    assert_fields_equal(renderer.crossings(sc, org[:500], dirs[:500]), ir.Crossings(ref.count[:500], ref.winding[:500]), name + " default interval")


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_inside_and_signed_distance_bit_equal_to_the_restatement(renderer, name):
    sc, osc = scene_pair(name)
    g = nr.from_oracle(osc)
    pts = point_set(g, 800, 13)
    near = nr.nearest(g, pts)
    radius = (np.sqrt(near.d2) * np.random.default_rng(5).uniform(0.25, 2.0, len(pts)).astype(np.float32)).astype(np.float32)
    near_r, near_0 = nr.nearest(g, pts, radius), nr.nearest(g, pts, 0.0)
    assert (near_r.prim >= 0).any() and (near_r.prim < 0).any() and (near_0.prim == -1).all()
    raw = renderer.nearest(sc, pts)
    for rule in RULE_NAMES:
        v = ir.votes(osc, pts, rule)
        if name in ("cube", "torus"):
            assert (v == 3).any() and (v == 0).any()
        assert_votes_equal(renderer.inside(sc, pts, rule=rule, votes=True), v, "%s %s votes" % (name, rule))
        assert_votes_equal(renderer.inside(sc, pts, rule=rule), v >= 2, "%s %s" % (name, rule))
        side = np.where(v >= 2, np.float32(-1), np.float32(1)).astype(np.float32)
        for what, md, ref in (("inf", np.inf, near), ("per point", radius, near_r), ("0", 0.0, near_0)):
            got = renderer.signedDistance(sc, pts, md, rule=rule)
            assert_fields_equal(got, ref._replace(side=side), "%s %s max_dist %s" % (name, rule, what))
        # the first seven words are nearest's own output
        got = renderer.signedDistance(sc, pts, rule=rule)
        for f in ("point", "d2", "prim", "u", "v"):
            assert getattr(got, f).tobytes() == getattr(raw, f).tobytes(), (name, rule, f)
    assert_votes_equal(renderer.inside(sc, pts), ir.votes(osc, pts) >= 2, name + " default rule")
    # packed points: max_dist is ignored by inside
    packed = np.concatenate([pts, np.zeros((len(pts), 1), np.float32)], axis=1)
    assert_votes_equal(renderer.inside(sc, packed, votes=True), ir.votes(osc, pts), name + " packed")


def test_the_wedge_points_come_out_as_derived(renderer):
    sc, osc = scene_pair("wedge")
    near = renderer.nearest(sc, ir.WEDGE_POINTS)
    assert sorted(near.side.tolist()) == [-1.0, 1.0] and near.prim[0] == near.prim[1]      # nearest: one outside point is "behind"
    assert_fields_equal(near, nr.nearest(nr.from_oracle(osc), ir.WEDGE_POINTS), "wedge nearest")
    for rule in RULE_NAMES:
        assert renderer.inside(sc, ir.WEDGE_POINTS, rule=rule, votes=True).tolist() == [0, 0]
        sd = renderer.signedDistance(sc, ir.WEDGE_POINTS, rule=rule)
        assert sd.side.tolist() == [1.0, 1.0] and sd.d2.tolist() == [np.float32(1 / 256 + 1 / 4096)] * 2
        assert_fields_equal(sd, ir.signed_distance(osc, ir.WEDGE_POINTS, rule=rule), "wedge " + rule)
    assert renderer.signedDistance(sc, np.float32([[0.5, 0, 0.5]])).side.tolist() == [-1.0]


def test_an_empty_scene_has_no_crossings_and_no_inside(renderer):
    sc = drt.Scene()
    sc.addMaterial((0.8, 0.8, 0.8), -1)
    sc.setGeometry(np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 2), np.float32), np.zeros(0, np.int32))
    drt.BVHBuilder().buildIterative(sc)
    pts = np.random.default_rng(0).normal(size=(500, 3)).astype(np.float32)
    pts[7, 1] = np.nan
    c = renderer.crossings(sc, pts, np.tile(ir.DIRS[0], (500, 1)))
    assert c.count.dtype == np.uint32 and c.winding.dtype == np.int32 and not c.count.any() and not c.winding.any()
    for rule in RULE_NAMES:
        assert not renderer.inside(sc, pts, rule=rule, votes=True).any()
        sd = renderer.signedDistance(sc, pts, 2.5, rule=rule)
        assert_fields_equal(sd, nr.nearest(nr.from_product(sc), pts, 2.5)._replace(side=np.ones(500, np.float32)), "empty " + rule)


@pytest.fixture(scope="module")
def batch():
    sc, osc = scene_pair("torus")
    pts = point_set(nr.from_oracle(osc), 1400, 21)[:2000]
    assert len(pts) == 2000
    rays = np.concatenate([pts, np.zeros((2000, 1), np.float32), np.tile(ir.DIRS, (667, 1))[:2000], np.full((2000, 1), np.inf, np.float32)], axis=1)
    ref = {"rays": rays.astype(np.float32), "crossings": ir.crossings(osc, pts, rays[:, 4:7])}
    for rule in RULE_NAMES:
        ref[rule] = ir.votes(osc, pts, rule)
    ref["nearest"] = nr.nearest(nr.from_oracle(osc), pts, 0.5)
    return sc, pts, ref


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2000])
def test_batch_sizes(renderer, batch, n):
    sc, pts, ref = batch
    for sl in (slice(0, n), slice(2000 - n, 2000)):
        assert_fields_equal(renderer.crossings(sc, ref["rays"][sl]), ir.Crossings(*[f[sl] for f in ref["crossings"]]), "crossings %r" % (sl,))
        for rule in RULE_NAMES:
            assert_votes_equal(renderer.inside(sc, pts[sl], rule=rule, votes=True), ref[rule][sl], "%s %r" % (rule, sl))
            side = np.where(ref[rule][sl] >= 2, np.float32(-1), np.float32(1)).astype(np.float32)
            want = nr.Nearest(*[f[sl] for f in ref["nearest"]])._replace(side=side)
            assert_fields_equal(renderer.signedDistance(sc, pts[sl], 0.5, rule=rule), want, "signed %s %r" % (rule, sl))


def _packed(res):
    return torch.cat([res.point, res.d2[:, None], res.prim.view(torch.float32)[:, None], res.u[:, None], res.v[:, None], res.side[:, None]],
                     dim=1).view(torch.int32)


def test_a_batch_beyond_the_grid_a_permutation_and_a_second_run(renderer, batch):
    sc, pts, ref = batch
    tiles = 300                                 # 600 000 queries: more than the persistent grid has threads, so lanes are refilled
    assert tiles * len(pts) > torch.cuda.get_device_properties(0).multi_processor_count * 2048
    dev_pts = torch.from_numpy(pts).to(DEV).repeat(tiles, 1)
    perm = torch.from_numpy(np.random.default_rng(2).permutation(len(dev_pts))).to(DEV)
    for rule in RULE_NAMES:
        got = renderer.inside(sc, dev_pts, rule=rule, votes=True)
        want = torch.from_numpy(ref[rule]).to(DEV).repeat(tiles)
        assert got.dtype == torch.uint8 and torch.equal(got, want), "%s: %d of %d votes differ from the tiled reference" % (rule, (got != want).sum(), len(want))
        assert torch.equal(renderer.inside(sc, dev_pts, rule=rule, votes=True), got)                      # two runs: identical bytes
        assert torch.equal(renderer.inside(sc, dev_pts[perm], rule=rule, votes=True), got[perm])
        assert torch.equal(renderer.inside(sc, dev_pts, rule=rule), want >= 2)
    side = np.where(ref["parity"] >= 2, np.float32(-1), np.float32(1)).astype(np.float32)
    near = ref["nearest"]
    want = np.concatenate([near.point, near.d2[:, None], near.prim.view(np.float32)[:, None], near.u[:, None], near.v[:, None], side[:, None]], axis=1)
    want = torch.from_numpy(np.ascontiguousarray(want).view(np.int32)).to(DEV).repeat(tiles, 1)
    got = _packed(renderer.signedDistance(sc, dev_pts, 0.5))
    bad = (got != want).any(dim=1)
    assert not bad.any(), "%d of %d records differ from the tiled reference, first %d" % (bad.sum(), len(bad), bad.nonzero()[0])
    assert torch.equal(_packed(renderer.signedDistance(sc, dev_pts, 0.5)), got)
    assert torch.equal(_packed(renderer.signedDistance(sc, dev_pts[perm], 0.5)), got[perm])
    dev_rays = torch.from_numpy(ref["rays"]).to(DEV).repeat(tiles, 1)
    c = renderer.crossings(sc, dev_rays)
    got = torch.stack([c.count, c.winding], dim=1)
    want = torch.from_numpy(np.stack([ref["crossings"].count.view(np.int32), ref["crossings"].winding], axis=1)).to(DEV).repeat(tiles, 1)
    assert got.dtype == torch.int32 and torch.equal(got, want)
    c = renderer.crossings(sc, dev_rays[perm])
    assert torch.equal(torch.stack([c.count, c.winding], dim=1), got[perm])


def test_after_a_refit_the_moved_mesh_answers(renderer):
    def load():
        return rq.programmatic_scene(drt, *ir.streams(ir.torus()), 4, 8)[0]

    sc, host = load(), load()
    moved = (ir.torus() * np.float32([1.25, 0.75, 1.5]) + np.float32([0.125, 0, -0.25])).astype(np.float32)
    host.refit(moved)                                          # the host scene refitted with the same positions
    old, new = ir.product_scene(sc), ir.product_scene(host)
    g_old, g_new = nr.from_product(sc), nr.from_product(host)
    pts = np.concatenate([point_set(g_old, 500, 4), point_set(g_new, 500, 5)])
    org, dirs = pts, np.tile(ir.DIRS, (len(pts) // 3 + 1, 1))[:len(pts)]
    v_old, v_new = ir.votes(old, pts), ir.votes(new, pts)
    assert ((v_old >= 2) != (v_new >= 2)).mean() > 0.05
    r = drt.Renderer(0)
    assert_votes_equal(r.inside(sc, pts, votes=True), v_old, "before the refit")
    r.refit(sc, torch.from_numpy(moved).to(DEV))
    assert_votes_equal(r.inside(sc, pts, votes=True), v_new, "after the refit")
    assert_votes_equal(r.inside(sc, pts, rule="winding", votes=True), ir.votes(new, pts, "winding"), "after the refit, winding")
    assert_fields_equal(r.crossings(sc, org, dirs), ir.crossings(new, org, dirs), "crossings after the refit")
    assert_fields_equal(r.signedDistance(sc, pts), ir.signed_distance(new, pts, g=g_new), "signed distance after the refit")
    assert_votes_equal(renderer.inside(sc, pts, votes=True), v_old, "a renderer that was not refitted")
    assert_fields_equal(renderer.signedDistance(sc, pts), ir.signed_distance(old, pts, g=g_old), "a renderer that was not refitted")
    assert_votes_equal(r.inside(sc, pts, votes=True), v_new, "after the other renderer's query")


def test_torch_path_stays_on_the_device_and_orders_with_the_stream(renderer):
    sc, osc = scene_pair("torus")
    dev = torch.device(DEV)
    pts = point_set(nr.from_oracle(osc), 2400, 12)
    v = ir.votes(osc, pts)
    ref = ir.signed_distance(osc, pts)
    dirs = np.tile(ir.DIRS, (len(pts) // 3 + 1, 1))[:len(pts)]
    cref = ir.crossings(osc, pts, dirs)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        p = torch.from_numpy(pts).to(dev)
        d = torch.from_numpy(dirs).to(dev)
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(2000000)                  # the inputs' producer is still busy when the queries are enqueued
        votes = renderer.inside(sc, p * 1.0, votes=True)
        flags = renderer.inside(sc, p * 1.0)
        sd = renderer.signedDistance(sc, p * 1.0)
        c = renderer.crossings(sc, p * 1.0, d * 1.0)
        side_copy = sd.side.clone()
        grid = renderer.sdfGrid(sc, (5, 4, 3))
    assert votes.device == dev and votes.dtype == torch.uint8 and flags.dtype == torch.bool and all(x.device == dev for x in sd)
    assert c.count.dtype == torch.int32 and c.winding.dtype == torch.int32 and c.count.device == dev
    s.synchronize()
    assert_votes_equal(votes.cpu().numpy(), v, "device tensors")
    assert_votes_equal(flags.cpu().numpy(), v >= 2, "device tensors")
    assert_fields_equal(nr.Nearest(*[x.cpu().numpy() for x in sd]), ref, "device tensors")
    assert (side_copy.cpu().numpy() == ref.side).all()
    assert_fields_equal(ir.Crossings(c.count.cpu().numpy().view(np.uint32), c.winding.cpu().numpy()), cref, "device tensors")
    # the grid: cell centres of the scene's bounds, [Z, Y, X], side * sqrt(d2)
    assert grid.device == dev and grid.dtype == torch.float32 and tuple(grid.shape) == (3, 4, 5)
    lo, hi = np.float32(sc.m_BVHNodes[-1]["bmin"]), np.float32(sc.m_BVHNodes[-1]["bmax"])
    res = (5, 4, 3)
    axes = [float(lo[k]) + (torch.arange(res[k], dtype=torch.float32) + 0.5) * (float(hi[k] - lo[k]) / res[k]) for k in range(3)]
    z, y, x = torch.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    cells = torch.stack([x, y, z], dim=-1).reshape(-1, 3).numpy()
    want = ir.signed_distance(osc, cells)
    # (the square root is torch's: within an ulp of the correctly rounded one, 2^-23 relative, whichever way it rounds)
    assert np.allclose(grid.cpu().numpy().ravel(), want.side * np.sqrt(want.d2), rtol=2.0 ** -22, atol=0) and (want.side < 0).any()
    boxed = renderer.sdfGrid(sc, 2, lo=(-0.5, -0.5, -0.5), hi=(1.5, 0.5, 0.5), rule="winding").cpu().numpy()
    cells = np.float32([[x, y, z] for z in (-0.25, 0.25) for y in (-0.25, 0.25) for x in (0.0, 1.0)])
    want = ir.signed_distance(osc, cells, rule="winding")
    assert boxed.shape == (2, 2, 2) and np.allclose(boxed.ravel(), want.side * np.sqrt(want.d2), rtol=2.0 ** -22, atol=0)
    assert (boxed[..., 1] < 0).all() and (boxed[..., 0] > 0).all()                 # x = 1: in the tube; x = 0: in the hole


def test_queries_leave_the_renderer_alone_and_work_on_a_sharded_one(renderer):
    sc, osc = scene_pair("cornell_box")
    _, pos, fwd, depth = SCENES["cornell_box"]
    cam = drt.Camera(pos)
    cam.m_Forward_dir = np.array(fwd, np.float32)
    pts = point_set(nr.from_oracle(osc), 1200, 6)
    v, sd = ir.votes(osc, pts), ir.signed_distance(osc, pts)
    dirs = np.tile(ir.DIRS, (len(pts) // 3 + 1, 1))[:len(pts)]
    cref = ir.crossings(osc, pts, dirs)
    images = []
    for with_queries in (False, True):
        r = drt.Renderer(0)
        r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=depth)
        r.ResizeBuffer(96, 64)
        r.Render(cam, sc)
        if with_queries:
            info, frame, accum, n, span = r.kernelInfo(), r.GetRenderTargetImage(), r.GetAccumulationBuffer(), r.getSampleCount(), r.kernelSpanMs()
            assert_votes_equal(r.inside(sc, pts, votes=True), v, "between two renders")
            assert_fields_equal(r.signedDistance(sc, pts), sd, "between two renders")
            assert_fields_equal(r.crossings(sc, pts, dirs), cref, "between two renders")
            assert r.kernelInfo() == info and r.getSampleCount() == n and r.kernelSpanMs() == span
            assert r.GetRenderTargetImage().tobytes() == frame.tobytes() and r.GetAccumulationBuffer().tobytes() == accum.tobytes()
        r.Render(cam, sc)
        images.append((r.GetRenderTargetImage(), r.getSampleCount()))
    assert images[0][0].tobytes() == images[1][0].tobytes() and images[0][1] == images[1][1]
    r = drt.Renderer(0)
    r.setShard(8, 1, 2)
    r.ResizeBuffer(96, 64)
    assert_votes_equal(r.inside(sc, pts, votes=True), v, "sharded renderer")
    assert_fields_equal(r.signedDistance(sc, pts), sd, "sharded renderer")
    assert_fields_equal(r.crossings(sc, pts, dirs), cref, "sharded renderer")


def test_error_paths(renderer):
    sc, osc = scene_pair("cornell_box")
    dev = torch.device(DEV)
    pts = torch.zeros((65, 4), dtype=torch.float32, device=dev)
    rays = torch.zeros((65, 8), dtype=torch.float32, device=dev)
    rays[:, 4] = 1
    out = torch.zeros((66, 8), dtype=torch.float32, device=dev)
    L, h = drt._lib, renderer._h
    INV = drt.ERR_INVALID
    host_in, host_out = np.zeros((64, 8), np.float32), np.zeros((64, 8), np.float32)
    calls = {"crossings": (lambda *a: L.drt_renderer_crossings(*a[:5], a[6]), rays, 8),
             "inside": (lambda *a: L.drt_renderer_inside(*a), pts, 0),
             "signed_distance": (lambda *a: L.drt_renderer_signed_distance(*a), pts, 16)}
    for what, (fn, src, align) in calls.items():
        assert fn(h, sc._h, None, out.data_ptr(), 64, 0, None) == INV, what
        assert fn(h, sc._h, src.data_ptr(), None, 64, 0, None) == INV, what
        assert fn(None, sc._h, src.data_ptr(), out.data_ptr(), 64, 0, None) == INV, what
        assert fn(h, None, src.data_ptr(), out.data_ptr(), 64, 0, None) == INV, what
        assert fn(h, sc._h, src.data_ptr() + 4, out.data_ptr(), 64, 0, None) == INV, what                 # misaligned queries
        if align:
            assert fn(h, sc._h, src.data_ptr(), out.data_ptr() + align // 2, 64, 0, None) == INV, what    # misaligned results
        assert fn(h, sc._h, host_in.ctypes.data, out.data_ptr(), 64, 0, None) == INV, what                # host memory
        assert fn(h, sc._h, src.data_ptr(), host_out.ctypes.data, 64, 0, None) == INV, what
        assert fn(h, sc._h, None, None, 0, 0, None) == drt.OK, what                                       # n == 0: nothing to do
        if what != "crossings":
            for rule in (2, -1):
                assert fn(h, sc._h, src.data_ptr(), out.data_ptr(), 64, rule, None) == INV, what
                assert b"rule" in L.drt_last_error()
    torch.cuda.synchronize()
    assert (out == 0).all()                                                                               # nothing was launched
    assert L.drt_renderer_inside(h, sc._h, pts.data_ptr(), out.data_ptr() + 1, 64, 1, None) == drt.OK     # votes need no alignment
    torch.cuda.synchronize()
    flat = out.view(torch.uint8).view(-1)
    assert flat[0] == 0 and (flat[65:] == 0).all() and (flat[1:65] == flat[1]).all() and flat[1] <= 3     # 64 bytes, one vote each
    assert len(renderer.inside(sc, np.zeros((0, 3), np.float32))) == 0 and len(renderer.signedDistance(sc, np.zeros((0, 3), np.float32)).d2) == 0
    assert len(renderer.crossings(sc, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)).count) == 0
    for bad in (lambda: renderer.inside(sc, pts.cpu()),                                                  # wrong device
                lambda: renderer.inside(sc, pts.double()),                                               # wrong dtype
                lambda: renderer.inside(sc, pts[:, :2]),                                                 # wrong shape
                lambda: renderer.inside(sc, pts, rule="odd"),
                lambda: renderer.signedDistance(sc, pts[:, :3], pts[:10, 3]),                            # mismatched counts
                lambda: renderer.signedDistance(sc, pts[:, :3].cpu().numpy(), pts[:, 3]),                # numpy mixed with device tensors
                lambda: renderer.signedDistance(sc, pts, 1.0),                                           # packed points carry max_dist
                lambda: renderer.signedDistance(sc, pts, rule="even"),
                lambda: renderer.crossings(sc, rays[:, :3], rays[:10, 4:7]),
                lambda: renderer.crossings(sc, rays, tmax=1.0),                                          # packed rays carry their interval
                lambda: renderer.sdfGrid(sc, 0),
                lambda: renderer.crossings(sc, host_in.astype(np.float64))):
        with pytest.raises(drt.DrtError) as e:
            bad()
        assert e.value.code == INV
    # a pending asynchronous batch
    r = drt.Renderer(0)
    r.ResizeBuffer(64, 32)
    r.RenderBatchAsync(drt.Camera(SCENES["cornell_box"][1]), sc, 1)
    for call in (lambda: r.inside(sc, pts), lambda: r.signedDistance(sc, pts), lambda: r.crossings(sc, rays)):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == INV
    r.Wait()
    r.inside(sc, pts), r.signedDistance(sc, pts), r.crossings(sc, rays)
    # a 67-level tree: the chain's centroids double per triangle (scaled down so that no area overflows)
    chain = list(rq.degenerate_chain(110))
    chain[0] = (chain[0] * np.float32(2.0 ** -55)).astype(np.float32)
    deep, _ = rq.programmatic_scene(drt, *chain, 1, 2)
    assert deep.bvh_depth == 67
    for call in (lambda: renderer.inside(deep, pts), lambda: renderer.signedDistance(deep, pts), lambda: renderer.crossings(deep, rays)):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == drt.ERR_UNSUPPORTED
    p = pts[:, :3].cpu().numpy()
    assert_votes_equal(renderer.inside(sc, p, votes=True), ir.votes(osc, p), "after the errors")
