"""Batched ray queries on the GPU (drt_renderer_trace_rays / drt_renderer_occluded, kernel_ray_query.hip): every field of every
result bit-equal to the restatement in tests/ray_query_ref.py, tied to what the renderer draws, deterministic, on the torch path,
and the error codes of include/drt.h."""
import ctypes as C

import numpy as np
import pytest

import oracle
from tests import ray_query_ref as rq
from tests.scenes import SCENES, scene_path

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

QUERY_SCENES = ["cornell_box", "suzanne_plane", "dense_monkey", "cs16_dust", "mc_transparency", "uv_texture_test"]
_cache = {}


@pytest.fixture(scope="module")
def renderer():
    return drt.Renderer(0)


def scene_pair(name):
    if name not in _cache:
        sc = drt.Scene()
        sc.loadGLTFmodel(scene_path(name))
        b = drt.BVHBuilder()
        b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
        b.buildIterative(sc)
        _cache[name] = (sc, oracle.Scene.load_glb(scene_path(name)).build_bvh(20, 8))
    return _cache[name]


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_hits_equal(got, ref, what):
    for field in ("t", "u", "v"):
        g, r = u32(getattr(got, field)), u32(getattr(ref, field))
        bad = np.nonzero(g != r)[0]
        assert len(bad) == 0, "%s: %s differs on %d rays, first %d: %r vs %r" % (what, field, len(bad), bad[0], getattr(got, field)[bad[0]], getattr(ref, field)[bad[0]])
    bad = np.nonzero(np.asarray(got.prim) != ref.prim)[0]
    assert len(bad) == 0, "%s: prim differs on %d rays" % (what, len(bad))


def check_sets(renderer, sc, osc, sets, what):
    for label, (org, dirs, tmin, tmax) in sets.items():
        got = renderer.traceRays(sc, org, dirs, tmin, tmax)
        assert_hits_equal(got, rq.closest(osc, org, dirs, tmin, tmax), "%s %s closest" % (what, label))
        occ_tmax = np.float32(np.inf) if tmax is rq.FLT_MAX else tmax
        occ = renderer.occluded(sc, org, dirs, tmin, occ_tmax)
        ref = rq.occluded(osc, org, dirs, tmin, occ_tmax)
        assert occ.dtype == bool and (occ == ref).all(), "%s %s occluded: %d rays differ" % (what, label, (occ != ref).sum())


def ray_sets(osc, name, n=2000, seed=7):
    rng = np.random.default_rng(seed)
    _, pos, fwd, _ = SCENES.get(name, (None, (0.0, 0.5, 12.0), (0.0, -0.05, -1.0), 0))
    org, dirs = rq.camera_rays(oracle.default_camera(position=pos, forward=fwd), 64, 36)
    sets = {"camera": (org, dirs, np.float32(0), rq.FLT_MAX)}
    org, dirs = rq.surface_rays(osc, n, rng)
    sets["surface"] = (org, dirs, np.float32(0), rq.FLT_MAX)
    sets["intervals"] = rq.interval_rays(osc, n, rng)
    org, dirs = rq.axis_rays(osc, n // 2, rng)
    sets["axis"] = (org, dirs, np.float32(0), np.float32(np.inf))
    org, dirs = rq.box_rays(osc, n // 2, rng)
    sets["in_boxes"] = (org, dirs, rng.uniform(0, 0.1, n // 2).astype(np.float32), rng.uniform(0.1, 5, n // 2).astype(np.float32))
    return sets


@pytest.mark.parametrize("name", QUERY_SCENES)
def test_queries_bit_equal_to_the_restatement(renderer, name):
    sc, osc = scene_pair(name)
    check_sets(renderer, sc, osc, ray_sets(osc, name), name)


def test_default_intervals_are_traceray_and_raytest(renderer):
    sc, osc = scene_pair("mc_transparency")
    org, dirs = rq.surface_rays(osc, 3000, np.random.default_rng(1))
    assert_hits_equal(renderer.traceRays(sc, org, dirs), rq.closest(osc, org, dirs, np.float32(0), rq.FLT_MAX), "TraceRay")
    assert (renderer.occluded(sc, org, dirs) == rq.occluded(osc, org, dirs, np.float32(0), np.float32(np.inf))).all()
    # packed rays [N, 8] = (org, tmin, dir, tmax)
    packed = np.concatenate([org, np.zeros((len(org), 1), np.float32), dirs, np.full((len(org), 1), rq.FLT_MAX, np.float32)], axis=1)
    assert_hits_equal(renderer.traceRays(sc, packed), rq.closest(osc, org, dirs, np.float32(0), rq.FLT_MAX), "packed")


def test_camera_rays_of_a_1080p_frame_match_the_renderers_images(renderer):
    """Hit/miss = black pixel of the zero-bounce image (no tone mapping, gamma, sun); (1-u-v, u, v) = the barycentric debug view."""
    name = "cornell_box"
    sc, _ = scene_pair(name)
    _, pos, fwd, _ = SCENES[name]
    W, H = 1920, 1080
    org, dirs = rq.camera_rays(oracle.default_camera(position=pos, forward=fwd), W, H)
    hits = renderer.traceRays(sc, org, dirs)
    cam = drt.Camera(pos)
    cam.m_Forward_dir = np.array(fwd, np.float32)
    r = drt.Renderer(0)
    r.ResizeBuffer(W, H)
    r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=0, tone_mapping=0, gamma_correction=0, enableSunlight=0)
    r.Render(cam, sc)
    black = (r.GetRenderTargetImage()[..., :3] == 0).all(axis=-1).ravel()
    hit = hits.prim >= 0
    assert hit.any() and (~hit).any()
    assert (black == hit).all(), "%d pixels disagree" % (black != hit).sum()
    r.m_RendererSettings = drt.RendererSettings(RenderMode=1, DebugMode=2)
    r.resetAccumulationBuffer()
    r.Render(cam, sc)
    dbg = r.GetRenderTargetImage()[..., :3].reshape(-1, 3)[hit]
    bary = np.stack([np.float32(1) - hits.u[hit] - hits.v[hit], hits.u[hit], hits.v[hit]], axis=1).astype(np.float32)
    bary = np.float32(0) + bary          # the frame is added to a zeroed sum (RenderKernel.cu:29): a -0 barycentric shows as +0
    assert (u32(dbg) == u32(bary)).all()


def test_trees_beyond_16_bit_references_and_beyond_the_lds_stack(renderer):
    sc, osc = rq.programmatic_scene(drt, *rq.soup(90000, 1, spread=10.0), 2, 8)
    assert len(sc.m_BVHNodes) > 65535
    check_sets(renderer, sc, osc, ray_sets(osc, "soup", n=1500), "soup of %d nodes" % len(sc.m_BVHNodes))
    sc, osc = rq.programmatic_scene(drt, *rq.degenerate_chain(), 1, 2)
    assert sc.bvh_depth > 16                 # more levels than the kernels keep in LDS (8 closest, 16 occluded)
    rng = np.random.default_rng(4)
    org = np.tile(np.float32([-3.0, 0.0, 0.0]), (3000, 1))
    dirs = np.concatenate([np.ones((3000, 1), np.float32), rng.normal(scale=0.02, size=(3000, 2)).astype(np.float32)], axis=1)
    sets = {"chain": (org, dirs, np.float32(0), rq.FLT_MAX)}
    sets.update(ray_sets(osc, "chain", n=1000))
    check_sets(renderer, sc, osc, sets, "chain of depth %d" % sc.bvh_depth)


def _device_rays(org, dirs, dev):
    return torch.from_numpy(org).to(dev), torch.from_numpy(dirs).to(dev)


def test_results_do_not_depend_on_order_batch_or_run(renderer):
    sc, osc = scene_pair("suzanne_plane")
    rng = np.random.default_rng(9)
    org, dirs = rq.surface_rays(osc, 1000000, rng)
    dev = torch.device("cuda", 0)
    o, d = _device_rays(org, dirs, dev)
    full = renderer.traceRays(sc, o, d)
    full_occ = renderer.occluded(sc, o, d)
    again = renderer.traceRays(sc, o, d)
    for a, b in zip(full, again):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    assert torch.equal(full_occ, renderer.occluded(sc, o, d))
    packed = torch.stack([x.view(torch.int32) if x.dtype == torch.float32 else x for x in full], dim=1)
    for n in (1, 63, 64, 65):
        part = renderer.traceRays(sc, o[:n], d[:n])
        got = torch.stack([x.view(torch.int32) if x.dtype == torch.float32 else x for x in part], dim=1)
        assert torch.equal(got, packed[:n]), n
        assert torch.equal(renderer.occluded(sc, o[:n], d[:n]), full_occ[:n]), n
    perm = torch.from_numpy(rng.permutation(len(org))).to(dev)
    part = renderer.traceRays(sc, o[perm], d[perm])
    got = torch.stack([x.view(torch.int32) if x.dtype == torch.float32 else x for x in part], dim=1)
    assert torch.equal(got, packed[perm])
    assert torch.equal(renderer.occluded(sc, o[perm], d[perm]), full_occ[perm])
    # and the first 3000 are the restatement's
    ref = rq.closest(osc, org[:3000], dirs[:3000], np.float32(0), rq.FLT_MAX)
    assert_hits_equal(rq.Hits(*[x[:3000].cpu().numpy() for x in full]), ref, "1e6 batch")


def test_torch_path_stays_on_the_device_and_orders_with_the_stream(renderer):
    sc, osc = scene_pair("cornell_box")
    dev = torch.device("cuda", 0)
    org, dirs = rq.surface_rays(osc, 50000, np.random.default_rng(12))
    ref = rq.closest(osc, org[:4000], dirs[:4000], np.float32(0), rq.FLT_MAX)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        o, d = _device_rays(org, dirs, dev)
        tmax = torch.full((len(org),), rq.FLT_MAX, device=dev)
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(2000000)                  # the inputs' producer is still busy when the query is enqueued
        hits = renderer.traceRays(sc, o * 1.0, d * 1.0, 0.0, tmax)
        occ = renderer.occluded(sc, o, d)
        t_sum = hits.t[:4000].clone()
    assert all(x.device == dev for x in hits) and occ.device == dev and occ.dtype == torch.bool
    s.synchronize()
    assert (u32(t_sum.cpu().numpy()) == u32(ref.t)).all()
    assert (hits.prim[:4000].cpu().numpy() == ref.prim).all()


def test_queries_leave_the_renderer_alone(renderer):
    sc, osc = scene_pair("cornell_box")
    _, pos, fwd, depth = SCENES["cornell_box"]
    cam = drt.Camera(pos)
    cam.m_Forward_dir = np.array(fwd, np.float32)
    org, dirs = rq.surface_rays(osc, 5000, np.random.default_rng(2))
    images = []
    for with_queries in (False, True):
        r = drt.Renderer(0)
        r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=depth)
        r.ResizeBuffer(96, 64)
        r.Render(cam, sc)
        info = r.kernelInfo()
        if with_queries:
            r.traceRays(sc, org, dirs)
            r.occluded(sc, org, dirs)
            assert r.kernelInfo() == info
        n = r.getSampleCount()
        r.Render(cam, sc)
        images.append((r.GetRenderTargetImage(), n, r.getSampleCount()))
    assert (u32(images[0][0]) == u32(images[1][0])).all()
    assert images[0][1:] == images[1][1:]


def test_error_paths(renderer):
    sc, osc = scene_pair("cornell_box")
    dev = torch.device("cuda", 0)
    rays = torch.zeros((64, 8), dtype=torch.float32, device=dev)
    rays[:, 4] = 1.0
    hits = torch.zeros((65, 4), dtype=torch.float32, device=dev)
    occ = torch.zeros(64, dtype=torch.uint8, device=dev)
    L, h = drt._lib, renderer._h
    assert L.drt_renderer_trace_rays(h, sc._h, None, hits.data_ptr(), 64, None) == drt.ERR_INVALID
    assert L.drt_renderer_trace_rays(h, sc._h, rays.data_ptr(), None, 64, None) == drt.ERR_INVALID
    assert L.drt_renderer_occluded(h, sc._h, rays.data_ptr(), None, 64, None) == drt.ERR_INVALID
    assert L.drt_renderer_trace_rays(None, sc._h, rays.data_ptr(), hits.data_ptr(), 64, None) == drt.ERR_INVALID
    assert L.drt_renderer_trace_rays(h, None, rays.data_ptr(), hits.data_ptr(), 64, None) == drt.ERR_INVALID
    assert L.drt_renderer_trace_rays(h, sc._h, rays.data_ptr() + 4, hits.data_ptr(), 63, None) == drt.ERR_INVALID
    assert L.drt_renderer_trace_rays(h, sc._h, rays.data_ptr(), hits.data_ptr() + 8, 64, None) == drt.ERR_INVALID
    host = np.zeros((64, 8), np.float32)
    assert L.drt_renderer_trace_rays(h, sc._h, host.ctypes.data, hits.data_ptr(), 64, None) == drt.ERR_INVALID
    assert L.drt_renderer_trace_rays(h, sc._h, None, None, 0, None) == drt.OK              # n == 0: nothing to do
    torch.cuda.synchronize()
    for bad in (lambda: renderer.traceRays(sc, rays.cpu()),                                # wrong device
                lambda: renderer.traceRays(sc, rays.double()),                             # wrong dtype
                lambda: renderer.traceRays(sc, rays[:, :6]),                               # wrong shape
                lambda: renderer.occluded(sc, rays[:, :3], rays[:10, 4:7]),                # mismatched counts
                lambda: renderer.traceRays(sc, rays[:, :3].cpu().numpy(), rays[:, 4:7]),   # numpy mixed with device tensors
                lambda: renderer.occluded(sc, host[:, :3].astype(np.float64), host[:, 4:7])):
        with pytest.raises(drt.DrtError) as e:
            bad()
        assert e.value.code == drt.ERR_INVALID
    if torch.cuda.device_count() > 1:
        with pytest.raises(drt.DrtError) as e:
            renderer.traceRays(sc, rays.to("cuda:1"))
        assert e.value.code == drt.ERR_INVALID
    # a pending asynchronous batch
    _, pos, fwd, _ = SCENES["cornell_box"]
    cam = drt.Camera(pos)
    r = drt.Renderer(0)
    r.ResizeBuffer(64, 32)
    r.RenderBatchAsync(cam, sc, 1)
    with pytest.raises(drt.DrtError) as e:
        r.traceRays(sc, rays)
    assert e.value.code == drt.ERR_INVALID
    r.Wait()
    r.traceRays(sc, rays)
    # (depth > 64 -> DRT_ERR_UNSUPPORTED: the builder makes no such tree from any input we can construct -- a degenerate chain
    #  long enough fails the build itself with DRT_ERR_BVH)
