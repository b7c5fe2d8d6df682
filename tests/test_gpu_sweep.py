"""Sphere casts on the GPU (drt_renderer_sphere_cast, kernel_sphere_cast.hip): every field of every record bit-equal to the
restatement in tests/sweep_ref.py -- over scenes, radii, intervals, a tree deeper than the LDS stack, batch shapes, a refitted device
copy and the torch path -- and the renderer's state untouched, and the error codes of include/drt.h."""
import numpy as np
import pytest

import oracle
from tests import nearest_ref as nr
from tests import ray_query_ref as rq
from tests import refit_ref as rf
from tests import sweep_ref as sw
from tests.scenes import SCENES, scene_path

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ONE_MATERIAL = [((0.8, 0.8, 0.8), -1)]
_cache = {}


@pytest.fixture(scope="module")
def renderer():
    return drt.Renderer(0)


def flat_scene(pos):
    n = len(pos)
    nrm = np.tile(np.float32([0, 0, 1]), (n, 3, 1))
    return rq.programmatic_scene(drt, pos, nrm, np.zeros((n, 3, 2), np.float32), np.zeros(n, np.int32), ONE_MATERIAL, [], 20, 8)


def scene_pair(name):
    """(product scene, Geometry of the oracle's scene), both with the editor's tree."""
    if name not in _cache:
        if name in ("single", "quad"):
            sc, osc = flat_scene(sw.TRI if name == "single" else sw.QUAD)
        else:
            sc = drt.Scene()
            sc.loadGLTFmodel(scene_path(name))
            b = drt.BVHBuilder()
            b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
            b.buildIterative(sc)
            osc = oracle.Scene.load_glb(scene_path(name)).build_bvh(20, 8)
        _cache[name] = (sc, nr.from_oracle(osc))
    return _cache[name]


def assert_equal(got, ref, what):
    """Bit for bit on every field."""
    assert len(got.t) == len(ref.t), what
    for field in sw.SweepHits._fields:
        g, r = np.ascontiguousarray(getattr(got, field)), np.ascontiguousarray(getattr(ref, field))
        assert g.shape == r.shape and g.dtype == r.dtype, (what, field, g.shape, r.shape, g.dtype, r.dtype)
        bad = np.nonzero((g.view(np.uint32) != r.view(np.uint32)).reshape(len(g), -1).any(axis=1))[0]
        assert len(bad) == 0, "%s: %s differs on %d of %d casts, first %d: %r vs %r" % (what, field, len(bad), len(g), bad[0], g[bad[0]], r[bad[0]])


def assert_all_miss(got, tmax, what):
    n = len(got.t)
    assert (got.prim == -1).all() and (got.feature == -1).all(), what
    assert (got.t.view(np.uint32) == np.ascontiguousarray(np.broadcast_to(np.float32(tmax), n)).view(np.uint32)).all(), what
    for f in (got.point, got.u, got.v):
        assert (np.ascontiguousarray(f).view(np.uint32) == 0).all(), what


def casts_of(g, n, seed):
    """About n casts of the four kinds of sweep_ref.cast_sets: (org, dirs, radius, tmin, tmax), all [N] float32 arrays."""
    return sw.cast_sets(g, n, np.random.default_rng(seed))


@pytest.mark.parametrize("name", ["single", "quad", "cornell_box", "suzanne_plane"])
def test_scene_sweep_bit_equal_to_the_restatement(renderer, name):
    sc, g = scene_pair(name)
    org, dirs, radius, tmin, tmax = casts_of(g, 1800, 11)
    ref = sw.sphere_cast(g, org, dirs, radius, tmin, tmax)
    hit = ref.prim >= 0
    assert hit.sum() > 200 and (~hit).sum() > 100 and len(set(ref.feature.tolist())) >= 9 and (tmin > 0).sum() > 300
    assert_equal(renderer.sphereCast(sc, org, dirs, radius, tmin, tmax), ref, name + " per-cast radius")
    # the variants on every fourth cast (the restatement is the slow side): a scalar radius, the ray, another interval
    org, dirs, radius, tmin, tmax, hit = (a[::4] for a in (org, dirs, radius, tmin, tmax, hit))
    ref = sw.SweepHits(*[f[::4] for f in ref])
    ext = float((nr.bounds(g)[1] - nr.bounds(g)[0]).max())
    for r in (0.02 * ext, 0.0):
        assert_equal(renderer.sphereCast(sc, org, dirs, r, tmin, tmax), sw.sphere_cast(g, org, dirs, r, tmin, tmax), "%s radius %g" % (name, r))
    assert_equal(renderer.sphereCast(sc, org, dirs, radius, 0.125, 4.0), sw.sphere_cast(g, org, dirs, radius, 0.125, 4.0), name + " tmin 0.125, tmax 4")
    # a per-cast mix with negative, NaN and infinite entries: those casts miss, their neighbours do not notice
    mixed = radius.copy()
    mixed[::5], mixed[1::7], mixed[2::11] = -radius[::5] - np.float32(1e-3), np.nan, -np.inf
    ref_m = sw.sphere_cast(g, org, dirs, mixed, tmin, tmax)
    assert (ref_m.prim[~(mixed >= 0)] == -1).all() and (ref_m.prim[mixed >= 0] == ref.prim[mixed >= 0]).all()
    assert_equal(renderer.sphereCast(sc, org, dirs, mixed, tmin, tmax), ref_m, name + " mixed radii")
    # tmax = the t found: a miss by the strict <
    at = np.where(hit, ref.t, tmax).astype(np.float32)
    got = renderer.sphereCast(sc, org, dirs, radius, tmin, at)
    assert_equal(got, sw.sphere_cast(g, org, dirs, radius, tmin, at), name + " tmax = t")
    assert_all_miss(got, at, name + " tmax = t")


def test_hand_derived_contacts_seams_and_zero_directions(renderer):
    sc, g = scene_pair("single")
    o, d, r = (np.float32([h[k] for h in sw.HAND]) for k in range(3))
    got = renderer.sphereCast(sc, o, d, r)
    assert_equal(got, sw.sphere_cast(g, o, d, r), "hand-derived")
    assert got.t.tolist() == [h[3] for h in sw.HAND] and got.feature.tolist() == [h[4] for h in sw.HAND]
    assert got.point.tolist() == [list(map(float, h[7])) for h in sw.HAND]
    zero = np.zeros_like(d)
    zero[::2] = -0.0
    got = renderer.sphereCast(sc, o, zero, r, 0.5)
    assert_equal(got, sw.sphere_cast(g, o, zero, r, 0.5), "zero directions")
    assert (got.prim >= 0).tolist() == [h[4] >= 8 for h in sw.HAND]
    sc, g = scene_pair("quad")
    for radius in (0.05, 1e-3):
        xy = sw.seam_casts(radius)
        o = np.concatenate([xy, np.ones((len(xy), 1))], axis=1).astype(np.float32)
        for d in (sw.DOWN, (0.3, -0.2, -1)):
            d = np.tile(np.float32(d), (len(o), 1))
            got = renderer.sphereCast(sc, (o - d - np.float32([0, 0, 1])).astype(np.float32), d, radius, 0.0, 2.0)
            assert_equal(got, sw.sphere_cast(g, (o - d - np.float32([0, 0, 1])).astype(np.float32), d, radius, 0.0, 2.0), "seams, radius %g" % radius)
            inside = (xy.min(axis=1) >= 0) & (xy.max(axis=1) <= 1)
            assert (got.prim[inside] >= 0).all()                                # nothing slips through the diagonal


def test_an_empty_scene_gives_all_misses(renderer):
    sc = drt.Scene()
    sc.addMaterial(*ONE_MATERIAL[0])
    sc.setGeometry(np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 2), np.float32), np.zeros(0, np.int32))
    drt.BVHBuilder().buildIterative(sc)
    assert len(sc.m_PrimitivesBuffer) == 0
    rng = np.random.default_rng(0)
    o, d = rng.normal(size=(500, 3)).astype(np.float32), rng.normal(size=(500, 3)).astype(np.float32)
    o[7, 1] = np.nan
    assert_all_miss(renderer.sphereCast(sc, o, d, 0.5), np.inf, "empty, inf")
    assert_all_miss(renderer.sphereCast(sc, o, d, 0.5, 0.0, 2.5), 2.5, "empty, 2.5")
    assert_equal(renderer.sphereCast(sc, o, d, 0.5, 0.0, 2.5), sw.sphere_cast(nr.from_product(sc), o, d, 0.5, 0.0, 2.5), "empty")


def test_a_tree_deeper_than_the_lds_stack(renderer):
    sc, osc = rq.programmatic_scene(drt, *rq.soup(3000, 5), 2, 8)
    assert sc.bvh_depth > 8                     # levels beyond the 8 in LDS run through the HBM stack
    g = nr.from_oracle(osc)
    org, dirs, radius, tmin, tmax = casts_of(g, 800, 3)
    radius = (radius * np.float32(3)).astype(np.float32)                        # fat spheres overlap many boxes: deep stacks
    visits = np.zeros(len(org), np.int64)
    ref = sw.sphere_cast(g, org, dirs, radius, tmin, tmax, visits=visits)
    assert visits.max() > 100
    assert_equal(renderer.sphereCast(sc, org, dirs, radius, tmin, tmax), ref, "soup of depth %d" % sc.bvh_depth)
    # a row of NaN rays: they visit nothing
    bad_o, bad_d = org[:72].copy(), dirs[:72].copy()
    bad_o[np.arange(36), np.arange(36) % 3] = np.nan
    bad_d[np.arange(36, 72), np.arange(36) % 3] = np.nan
    visits = np.zeros(72, np.int64)
    ref = sw.sphere_cast(g, bad_o, bad_d, radius[:72], 0.0, 7.0, visits=visits)
    assert visits.sum() == 0
    got = renderer.sphereCast(sc, bad_o, bad_d, radius[:72], 0.0, 7.0)
    assert_equal(got, ref, "NaN rays")
    assert_all_miss(got, 7.0, "NaN rays")


@pytest.fixture(scope="module")
def batch():
    sc, g = scene_pair("suzanne_plane")
    casts = casts_of(g, 2000, 21)
    assert len(casts[0]) == 2000
    return sc, casts, sw.sphere_cast(g, *casts)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2000])
def test_small_batches(renderer, batch, n):
    sc, casts, ref = batch
    assert_equal(renderer.sphereCast(sc, *[c[:n] for c in casts]), sw.SweepHits(*[f[:n] for f in ref]), "n = %d" % n)
    assert_equal(renderer.sphereCast(sc, *[c[-n:] for c in casts]), sw.SweepHits(*[f[-n:] for f in ref]), "last %d" % n)


def _packed(res):
    return torch.cat([res.t[:, None], res.prim.view(torch.float32)[:, None], res.u[:, None], res.v[:, None], res.point,
                      res.feature.view(torch.float32)[:, None]], dim=1).view(torch.int32)


def _packed_rays(casts):
    org, dirs, radius, tmin, tmax = casts
    return np.ascontiguousarray(np.concatenate([org, tmin[:, None], dirs, tmax[:, None]], axis=1), np.float32)


def test_a_batch_beyond_the_grid_a_slice_a_permutation_and_a_second_run(renderer, batch):
    sc, casts, ref = batch
    tiles = 300                                 # 600 000 casts: more than the persistent grid has threads, so lanes are refilled
    assert tiles * 2000 > torch.cuda.get_device_properties(0).multi_processor_count * 2048
    rays = torch.from_numpy(_packed_rays(casts)).to(DEV).repeat(tiles, 1)
    radii = torch.from_numpy(casts[2]).to(DEV).repeat(tiles)
    got = _packed(renderer.sphereCast(sc, rays, radius=radii))
    want = np.concatenate([ref.t[:, None], ref.prim.view(np.float32)[:, None], ref.u[:, None], ref.v[:, None], ref.point,
                           ref.feature.view(np.float32)[:, None]], axis=1)
    want = torch.from_numpy(np.ascontiguousarray(want).view(np.int32)).to(DEV).repeat(tiles, 1)
    bad = (got != want).any(dim=1)
    assert not bad.any(), "%d of %d results differ from the tiled reference, first %d" % (bad.sum(), len(bad), bad.nonzero()[0])
    assert torch.equal(_packed(renderer.sphereCast(sc, rays, radius=radii)), got)                      # two runs: identical bytes
    perm = torch.from_numpy(np.random.default_rng(2).permutation(len(rays))).to(DEV)
    assert torch.equal(_packed(renderer.sphereCast(sc, rays[perm], radius=radii[perm])), got[perm])
    # a slice of the larger tensors: records 1003 .. 4002, radii from a 4-byte-aligned address that is not 16-byte aligned
    assert radii[1003:].data_ptr() % 16 != 0
    assert torch.equal(_packed(renderer.sphereCast(sc, rays[1003:4003], radius=radii[1003:4003])), got[1003:4003])


def _load(name):
    sc = drt.Scene()
    sc.loadGLTFmodel(scene_path(name))
    st = rf.streams(sc.m_PrimitivesBuffer)
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
    b.buildIterative(sc)
    return sc, st


def test_after_a_refit_the_moved_geometry_answers(renderer):
    sc, st = _load("cornell_box")
    moved = (st[0] + np.random.default_rng(1).normal(0, 0.05, st[0].shape)).astype(np.float32)
    host, _ = _load("cornell_box")
    host.refit(moved)                                          # the host scene refitted with the same positions
    g_old, g_new = nr.from_product(sc), nr.from_product(host)
    casts = [np.concatenate([a, b]) for a, b in zip(casts_of(g_old, 800, 4), casts_of(g_new, 800, 5))]
    old, new = sw.sphere_cast(g_old, *casts), sw.sphere_cast(g_new, *casts)
    assert (old.t.view(np.uint32) != new.t.view(np.uint32)).mean() > 0.4
    r = drt.Renderer(0)
    assert_equal(r.sphereCast(sc, *casts), old, "before the refit")
    r.refit(sc, torch.from_numpy(moved).to(DEV))
    assert_equal(r.sphereCast(sc, *casts), new, "after the refit")
    assert_equal(renderer.sphereCast(sc, *casts), old, "a renderer that was not refitted")
    assert_equal(r.sphereCast(sc, *casts), new, "after the other renderer's query")


def test_torch_path_stays_on_the_device_and_orders_with_the_stream(renderer):
    sc, g = scene_pair("cornell_box")
    dev = torch.device(DEV)
    casts = casts_of(g, 4000, 12)
    ref = sw.sphere_cast(g, *casts)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        org, dirs, radius, tmin, tmax = (torch.from_numpy(c).to(dev) for c in casts)
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(2000000)                  # the inputs' producer is still busy when the query is enqueued
        got = renderer.sphereCast(sc, org * 1.0, dirs * 1.0, radius * 1.0, tmin * 1.0, tmax * 1.0)
        packed = renderer.sphereCast(sc, torch.cat([org, tmin[:, None], dirs, tmax[:, None]], dim=1), radius=radius)
        t_copy = got.t.clone()
    assert all(x.device == dev for x in got) and got.prim.dtype == torch.int32 and got.feature.dtype == torch.int32 and got.point.shape == (len(ref.t), 3)
    s.synchronize()
    assert_equal(sw.SweepHits(*[x.cpu().numpy() for x in got]), ref, "device tensors")
    assert_equal(sw.SweepHits(*[x.cpu().numpy() for x in packed]), ref, "packed [N, 8]")
    assert (t_copy.cpu().numpy().view(np.uint32) == ref.t.view(np.uint32)).all()
    assert_equal(renderer.sphereCast(sc, *casts), ref, "numpy")
    assert_equal(renderer.sphereCast(sc, _packed_rays(casts), radius=casts[2]), ref, "packed numpy")


def test_casts_leave_the_renderer_alone_and_work_on_a_sharded_one(renderer):
    sc, g = scene_pair("cornell_box")
    _, pos, fwd, depth = SCENES["cornell_box"]
    cam = drt.Camera(pos)
    cam.m_Forward_dir = np.array(fwd, np.float32)
    casts = casts_of(g, 2000, 6)
    ref = sw.sphere_cast(g, *casts)
    images = []
    for with_queries in (False, True):
        r = drt.Renderer(0)
        r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=depth)
        r.ResizeBuffer(96, 64)
        r.Render(cam, sc)
        if with_queries:
            info, frame, accum, n, span = r.kernelInfo(), r.GetRenderTargetImage(), r.GetAccumulationBuffer(), r.getSampleCount(), r.kernelSpanMs()
            counters = bytes(r.getCounters())
            assert_equal(r.sphereCast(sc, *casts), ref, "between two renders")
            assert r.kernelInfo() == info and r.getSampleCount() == n and r.kernelSpanMs() == span
            assert bytes(r.getCounters()) == counters
            assert r.GetRenderTargetImage().tobytes() == frame.tobytes() and r.GetAccumulationBuffer().tobytes() == accum.tobytes()
        r.Render(cam, sc)
        images.append((r.GetRenderTargetImage(), r.getSampleCount()))
    assert images[0][0].tobytes() == images[1][0].tobytes() and images[0][1] == images[1][1]
    r = drt.Renderer(0)
    r.setShard(8, 1, 2)
    r.ResizeBuffer(96, 64)
    assert_equal(r.sphereCast(sc, *casts), ref, "sharded renderer")


def test_error_paths(renderer):
    sc, g = scene_pair("cornell_box")
    dev = torch.device(DEV)
    rays = torch.zeros((65, 8), dtype=torch.float32, device=dev)
    radii = torch.zeros(66, dtype=torch.float32, device=dev)
    out = torch.zeros((66, 8), dtype=torch.float32, device=dev)
    L, h = drt._lib, renderer._h
    INV = drt.ERR_INVALID
    fn = L.drt_renderer_sphere_cast
    assert fn(h, sc._h, None, radii.data_ptr(), out.data_ptr(), 64, None) == INV
    assert fn(h, sc._h, rays.data_ptr(), None, out.data_ptr(), 64, None) == INV
    assert fn(h, sc._h, rays.data_ptr(), radii.data_ptr(), None, 64, None) == INV
    assert fn(None, sc._h, rays.data_ptr(), radii.data_ptr(), out.data_ptr(), 64, None) == INV
    assert fn(h, None, rays.data_ptr(), radii.data_ptr(), out.data_ptr(), 64, None) == INV
    assert fn(h, sc._h, rays.data_ptr() + 4, radii.data_ptr(), out.data_ptr(), 64, None) == INV        # misaligned
    assert fn(h, sc._h, rays.data_ptr(), radii.data_ptr() + 2, out.data_ptr(), 64, None) == INV
    assert fn(h, sc._h, rays.data_ptr(), radii.data_ptr(), out.data_ptr() + 8, 64, None) == INV
    host_rays, host_radii, host_out = np.zeros((64, 8), np.float32), np.zeros(64, np.float32), np.zeros((64, 8), np.float32)
    assert fn(h, sc._h, host_rays.ctypes.data, radii.data_ptr(), out.data_ptr(), 64, None) == INV       # host memory
    assert fn(h, sc._h, rays.data_ptr(), host_radii.ctypes.data, out.data_ptr(), 64, None) == INV
    assert fn(h, sc._h, rays.data_ptr(), radii.data_ptr(), host_out.ctypes.data, 64, None) == INV
    assert fn(h, sc._h, None, None, None, 0, None) == drt.OK                                            # n == 0: nothing to do
    assert len(renderer.sphereCast(sc, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), 0.5).t) == 0
    torch.cuda.synchronize()
    assert (out == 0).all()                                                                              # nothing was launched
    o3, d3 = rays[:, 0:3], rays[:, 4:7]
    for bad in (lambda: renderer.sphereCast(sc, o3.cpu(), d3.cpu(), 0.5),                               # wrong device
                lambda: renderer.sphereCast(sc, o3.double(), d3.double(), 0.5),                         # wrong dtype
                lambda: renderer.sphereCast(sc, rays[:, :5], radius=0.5),                               # wrong shape
                lambda: renderer.sphereCast(sc, o3, d3, radii[:10]),                                    # mismatched counts
                lambda: renderer.sphereCast(sc, o3, d3, radii[:65].double()),                           # radius dtype
                lambda: renderer.sphereCast(sc, o3, d3, radii[:65].cpu()),                              # radius on the host
                lambda: renderer.sphereCast(sc, o3, d3, host_radii[:65]),                               # numpy mixed with device tensors
                lambda: renderer.sphereCast(sc, o3, d3, "wide"),
                lambda: renderer.sphereCast(sc, rays, radius=0.5, tmin=1.0)):                           # packed rays carry tmin / tmax
        with pytest.raises(drt.DrtError) as e:
            bad()
        assert e.value.code == INV
    # a pending asynchronous batch
    r = drt.Renderer(0)
    r.ResizeBuffer(64, 32)
    r.RenderBatchAsync(drt.Camera(SCENES["cornell_box"][1]), sc, 1)
    with pytest.raises(drt.DrtError) as e:
        r.sphereCast(sc, rays, radius=0.5)
    assert e.value.code == INV
    r.Wait()
    r.sphereCast(sc, rays, radius=0.5)
    # a tree deeper than 64 levels: the chain's centroids double per triangle (scaled down so that no area overflows)
    chain = list(rq.degenerate_chain(110))
    chain[0] = (chain[0] * np.float32(2.0 ** -55)).astype(np.float32)
    deep, _ = rq.programmatic_scene(drt, *chain, 1, 2)
    assert deep.bvh_depth > 64
    with pytest.raises(drt.DrtError) as e:
        renderer.sphereCast(deep, rays, radius=0.5)
    assert e.value.code == drt.ERR_UNSUPPORTED
    casts = casts_of(g, 400, 9)
    assert_equal(renderer.sphereCast(sc, *casts), sw.sphere_cast(g, *casts), "after the errors")
