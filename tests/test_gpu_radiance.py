"""Path-traced radiance of arbitrary rays on the GPU (drt_renderer_camera_rays / drt_renderer_radiance, kernel_radiance.hip): camera
rays bit-equal to Camera::GetRay, radiance of the renderer's own primary rays bit-equal to the oracle's frame sample, accumulated
frames and multi-view renders bit-equal to single-camera renderers, arbitrary rays bit-equal to tests/radiance_ref.py, deep and
large trees, refit, determinism, the torch path, the error codes of include/drt.h and the absence of side effects."""
import os

import numpy as np
import pytest

import oracle
from tests import radiance_ref as rr
from tests import ray_query_ref as rq
from tests.scenes import SCENES, scene_path

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

W, H = 48, 32
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


def cameras(name, k=1, defocus=False):
    """k cameras around the scene's pose (drt, oracle); the second one with another exposure, the third with defocus if asked."""
    _, pos, fwd, _ = SCENES[name]
    out = []
    for i in range(k):
        p = (pos[0] + 0.1 * i, pos[1] - 0.05 * i, pos[2] + 0.07 * i)
        f = (fwd[0] + 0.03 * i, fwd[1], fwd[2])
        c = drt.Camera(p)
        c.m_Forward_dir = np.array(f, np.float32)
        c.exposure = np.float32(2.0 + 0.5 * i)
        kw = dict(position=p, forward=f, exposure=float(c.exposure))
        if defocus and i == 2:
            c.defocus_angle, c.focus_dist = 1.5, 3.0
            kw.update(defocus_angle=1.5, focus_dist=3.0)
        oc = oracle.default_camera(**kw)
        out.append((c, oc))
    return out


def settings(depth, sun, **kw):
    return (drt.RendererSettings(ray_bounce_limit=depth, enableSunlight=sun, **kw),
            oracle.default_settings(ray_bounce_limit=depth, enable_sunlight=sun, **kw))


def assert_bits(got, ref, what):
    bad = (u32(got) != u32(ref))
    if bad.ndim > 1:
        bad = bad.any(axis=-1)
    assert not bad.any(), "%s: %d of %d differ, first at %s: %r vs %r" % (
        what, bad.sum(), bad.size, np.argwhere(bad)[0], got[tuple(np.argwhere(bad)[0])], ref[tuple(np.argwhere(bad)[0])])


def frame_sample(r, sc, cam, frame):
    """radiance(camera_rays(cam, W, H, frame)) as the accumulation would hold it: 0 + c."""
    rays = r.cameraRays(cam, W, H, frame)
    return np.float32(0) + r.radiance(sc, rays)[..., :3]


# ---------------------------------------------------------------- camera rays

@pytest.mark.parametrize("size", [(7, 3), (64, 48)])
@pytest.mark.parametrize("frame", [1, 5])
def test_camera_rays_equal_getray(renderer, size, frame):
    w, h = size
    cams = cameras("cornell_box", 3, defocus=True)
    rays = renderer.cameraRays([c for c, _ in cams], w, h, frame)
    assert rays.shape == (3, h, w, 8) and rays.dtype == np.float32
    y, x = np.mgrid[0:h, 0:w]
    x, y = x.ravel().astype(np.uint32), y.ravel().astype(np.uint32)
    uv = np.stack([(x.astype(np.float32) / np.float32(w)) * np.float32(2) - np.float32(1),
                   (y.astype(np.float32) / np.float32(h)) * np.float32(2) - np.float32(1)], axis=1).astype(np.float32)
    seeds = ((x + y * np.uint32(w)) * np.uint32(frame)).astype(np.uint32)
    for k, (_, oc) in enumerate(cams):
        r6, so = oracle.kat_getray(oc, w, h, uv, seeds)
        got = rays[k].reshape(-1, 8)
        assert_bits(got[:, 0:3], r6[:, 0:3], "cam %d org" % k)
        assert_bits(got[:, 4:7], r6[:, 3:6], "cam %d dir" % k)
        assert (got[:, 3].view(np.uint32) == so).all(), "cam %d seed" % k
        assert (got[:, 7] == np.float32(oc.exposure)).all(), "cam %d exposure" % k


# ---------------------------------------------------------------- radiance of the renderer's primary rays = the oracle's frame sample

@pytest.mark.parametrize("name", ["cornell_box", "suzanne_plane", "dense_monkey", "cs16_dust", "mc_transparency", "uv_texture_test"])
@pytest.mark.parametrize("sun", [0, 1])
def test_radiance_of_camera_rays_is_the_frame_sample(renderer, name, sun):
    sc, osc = scene_pair(name)
    (cam, ocam), = cameras(name)
    for depth in (0, 2, 8):
        renderer.m_RendererSettings, ost = settings(depth, sun)
        for frame in (1, 3):
            got = frame_sample(renderer, sc, cam, frame)
            _, ref, _ = oracle.render(osc, ocam, ost, W, H, frame, 1)
            assert_bits(got, ref, "%s sun=%d depth=%d frame %d" % (name, sun, depth, frame))


def test_radiance_with_tone_mapping_and_gamma_off(renderer):
    sc, osc = scene_pair("cornell_box")
    (cam, ocam), = cameras("cornell_box")
    renderer.m_RendererSettings, ost = settings(4, 1, tone_mapping=0, gamma_correction=0)
    _, ref, _ = oracle.render(osc, ocam, ost, W, H, 2, 1)
    assert_bits(frame_sample(renderer, sc, cam, 2), ref, "no tone curve")


@pytest.mark.parametrize("name,model", [("emissive_test", (1, 1, 2.5)), ("cornell_box_gltf", (1, 0, 1.0)), ("glass", (1, 1, 1.5, 1)),
                                        ("glass", (0, 0, 1.0, 1))])
def test_radiance_with_the_material_model(name, model):
    from tests.test_material_model import _glass_scene
    if name == "glass":
        sc, osc = _glass_scene(0)
        pos, fwd, depth = (0.3, 1.6, 2.8), (-0.1, -0.15, -1.0), 7
    else:
        sc, osc = scene_pair(name)
        _, pos, fwd, depth = SCENES[name]
    cam = drt.Camera(pos)
    cam.m_Forward_dir = np.array(fwd, np.float32)
    ocam = oracle.default_camera(position=pos, forward=fwd)
    r = drt.Renderer(0)
    r.setMaterialModel(*model)
    osc.material_model = model
    try:
        for sun in (0, 1):
            r.m_RendererSettings, ost = settings(depth, sun)
            _, ref, _ = oracle.render(osc, ocam, ost, W, H, 2, 1)
            assert_bits(frame_sample(r, sc, cam, 2), ref, "%s %r sun=%d" % (name, model, sun))
    finally:
        osc.material_model = (0, 0, 1.0)


# ---------------------------------------------------------------- accumulation and multi-view = per-camera renderers

def test_accumulated_frames_equal_the_renderer(renderer):
    sc, _ = scene_pair("mc_transparency")
    (cam, _), = cameras("mc_transparency")
    renderer.m_RendererSettings, _ = settings(3, 1)
    acc = None
    for f in range(1, 5):
        rays = renderer.cameraRays(cam, W, H, f, as_torch=True)
        if acc is None:
            acc = torch.zeros(tuple(rays.shape[:-1]) + (4,), dtype=torch.float32, device=rays.device)
        renderer.radiance(sc, rays, out=acc, accumulate=True)
    r = drt.Renderer(0)
    r.m_RendererSettings = renderer.m_RendererSettings
    r.ResizeBuffer(W, H)
    for _ in range(4):
        r.Render(cam, sc)
    got = acc.cpu().numpy()[0]
    assert_bits(got[..., :3], r.GetAccumulationBuffer(), "accumulation over frames 1..4")
    assert (got[..., 3] == 0).all()                               # alpha untouched (it started at 0)


@pytest.mark.parametrize("as_torch", [False, True])
def test_render_views_equal_single_camera_renderers(as_torch):
    sc, _ = scene_pair("cornell_box")
    cams = [c for c, _ in cameras("cornell_box", 3, defocus=True)]
    r = drt.Renderer(0)
    r.m_RendererSettings, _ = settings(4, 1)
    views = r.renderViews(cams, sc, W, H, 3, as_torch=as_torch)
    views = views.cpu().numpy() if as_torch else views
    assert views.shape == (3, H, W, 4)
    for k, cam in enumerate(cams):
        one = drt.Renderer(0)
        one.m_RendererSettings = r.m_RendererSettings
        one.ResizeBuffer(W, H)
        one.RenderBatch(cam, sc, 3)
        assert_bits(views[k], one.GetRenderTargetImage(), "view %d" % k)


# ---------------------------------------------------------------- arbitrary rays = tests/radiance_ref.py

def path_rays(org, dirs, rng):
    """Packed drt_path_ray [n, 8]: org, a random seed state, dir, a random exposure."""
    n = len(org)
    seeds = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    exposure = rng.uniform(0.5, 4.0, n).astype(np.float32)
    return np.concatenate([org, seeds.view(np.float32)[:, None], dirs, exposure[:, None]], axis=1).astype(np.float32)


def check_ref(r, sc, osc, rays, depth, sun, what):
    r.m_RendererSettings, ost = settings(depth, sun)
    got = np.float32(0) + r.radiance(sc, rays)[:, :3]
    ref = np.float32(0) + rr.radiance(osc, rays[:, 0:3], rays[:, 4:7], rays[:, 3].view(np.uint32), rays[:, 7], ost)
    assert_bits(got, ref, what)


@pytest.mark.parametrize("name", ["cornell_box", "mc_transparency", "cs16_dust"])
def test_arbitrary_rays_equal_the_restatement(renderer, name):
    sc, osc = scene_pair(name)
    rng = np.random.default_rng(11)
    sets = {"surface": rq.surface_rays(osc, 800, rng), "axis": rq.axis_rays(osc, 400, rng), "box": rq.box_rays(osc, 400, rng),
            "interval": rq.interval_rays(osc, 400, rng)[:2]}
    for label, (org, dirs) in sets.items():
        rays = path_rays(org, dirs, rng)
        for depth, sun in ((3, 1), (2, 0)):
            check_ref(renderer, sc, osc, rays, depth, sun, "%s %s depth=%d sun=%d" % (name, label, depth, sun))


def test_large_and_deep_trees_equal_the_restatement(renderer):
    sc, osc = rq.programmatic_scene(drt, *rq.soup(90000, 1, spread=10.0), 2, 8)
    assert len(sc.m_BVHNodes) > 65535
    rng = np.random.default_rng(5)
    org, dirs = rq.surface_rays(osc, 600, rng)
    check_ref(renderer, sc, osc, path_rays(org, dirs, rng), 3, 1, "soup of %d nodes" % len(sc.m_BVHNodes))
    sc, osc = rq.programmatic_scene(drt, *rq.degenerate_chain(), 1, 2)
    assert sc.bvh_depth > 16                 # levels beyond the 8 kept in LDS
    org = np.tile(np.float32([-3.0, 0.0, 0.0]), (600, 1))
    dirs = (np.float32([1, 0, 0]) + rng.normal(0, 0.02, (600, 3))).astype(np.float32)
    rays = path_rays(org, dirs, rng)
    check_ref(renderer, sc, osc, rays, 4, 1, "chain of %d levels" % sc.bvh_depth)
    org2, dirs2 = rq.surface_rays(osc, 600, rng)
    check_ref(renderer, sc, osc, path_rays(org2, dirs2, rng), 4, 0, "chain, surface rays")


def test_radiance_follows_a_device_refit():
    from tests import refit_ref as rf
    sc = drt.Scene()
    sc.loadGLTFmodel(scene_path("cornell_box"))
    st = rf.streams(sc.m_PrimitivesBuffer)
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
    b.buildIterative(sc)
    (cam, _), = cameras("cornell_box")
    r = drt.Renderer(0)
    r.m_RendererSettings, _ = settings(3, 1)
    before = frame_sample(r, sc, cam, 1)
    pos = (st[0] + np.random.default_rng(3).normal(0, 0.05, st[0].shape)).astype(np.float32)
    r.refit(sc, pos)
    after = frame_sample(r, sc, cam, 1)
    assert not np.array_equal(u32(before), u32(after))
    r.ResizeBuffer(W, H)
    r.Render(cam, sc)                                   # the renderer's own frame 1 on the refitted copy
    assert_bits(after, r.GetAccumulationBuffer(), "radiance after a refit")


# ---------------------------------------------------------------- determinism, torch path, errors, side effects

def test_same_bits_twice_and_with_or_without_refill(renderer):
    sc, osc = scene_pair("cs16_dust")
    rng = np.random.default_rng(2)
    rays = path_rays(*rq.surface_rays(osc, 5000, rng), rng)
    renderer.m_RendererSettings, _ = settings(5, 1)
    a, b = renderer.radiance(sc, rays), renderer.radiance(sc, rays)
    assert np.array_equal(u32(a), u32(b))
    old = os.environ.get("DRT_RQ_REFILL")
    os.environ["DRT_RQ_REFILL"] = "64"                  # a wave claims new paths only when all 64 lanes are idle
    try:
        plain = drt.Renderer(0)
    finally:
        if old is None:
            os.environ.pop("DRT_RQ_REFILL", None)
        else:
            os.environ["DRT_RQ_REFILL"] = old
    plain.m_RendererSettings = renderer.m_RendererSettings
    assert np.array_equal(u32(plain.radiance(sc, rays)), u32(a))


def test_numpy_and_torch_side_stream_agree(renderer):
    sc, osc = scene_pair("mc_transparency")
    rng = np.random.default_rng(8)
    rays = path_rays(*rq.surface_rays(osc, 3000, rng), rng)
    renderer.m_RendererSettings, _ = settings(4, 1)
    ref = renderer.radiance(sc, rays)
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        t = torch.from_numpy(rays).to(dev).reshape(30, 100, 8)
        out = renderer.radiance(sc, t)
        acc = torch.zeros_like(out)
        renderer.radiance(sc, t, out=acc, accumulate=True)
        renderer.radiance(sc, t, out=acc, accumulate=True)
    side.synchronize()
    assert out.shape == (30, 100, 4)
    assert np.array_equal(u32(out.cpu().numpy().reshape(-1, 4)), u32(ref))
    twice = acc.cpu().numpy().reshape(-1, 4)
    assert np.array_equal(u32(twice[:, :3]), u32((np.float32(0) + ref[:, :3]) + ref[:, :3]))
    assert (twice[:, 3] == 0).all()
    # numpy out: written in place
    o = np.zeros((3000, 4), np.float32)
    assert renderer.radiance(sc, rays, out=o) is o and np.array_equal(u32(o), u32(ref))


def test_error_codes():
    import ctypes as C
    lib = drt._lib
    sc, _ = scene_pair("cornell_box")
    r = drt.Renderer(0)
    r.ResizeBuffer(8, 8)
    dev = torch.device("cuda", 0)
    rays = torch.zeros((64, 8), dtype=torch.float32, device=dev)
    out = torch.zeros((64, 4), dtype=torch.float32, device=dev)
    pod = (drt._CameraPOD * 1)(drt.Camera()._pod())
    h = r._h
    INV, UNS = drt.ERR_INVALID, drt.ERR_UNSUPPORTED
    host = np.zeros((64, 8), np.float32)
    cr = lambda *a: lib.drt_renderer_camera_rays(h, *a)
    ra = lambda *a: lib.drt_renderer_radiance(h, sc._h, *a)
    assert cr(pod, 1, 8, 8, 1, rays.data_ptr(), None) == 0
    assert cr(None, 1, 8, 8, 1, rays.data_ptr(), None) == INV
    assert cr(pod, 1, 8, 8, 1, None, None) == INV
    assert cr(pod, 1, 8, 8, 0, rays.data_ptr(), None) == INV            # frame 0
    assert cr(pod, 0, 8, 8, 1, rays.data_ptr(), None) == INV
    assert cr(pod, 1, 0, 8, 1, rays.data_ptr(), None) == INV
    assert cr(pod, 1, 8, 0, 1, rays.data_ptr(), None) == INV
    assert cr(pod, 1, 65536, 32768, 1, rays.data_ptr(), None) == INV    # 2^31 rays
    assert cr(pod, 1, 8, 8, 1, rays.data_ptr() + 4, None) == INV        # misaligned
    assert cr(pod, 1, 8, 8, 1, host.ctypes.data, None) == INV           # host memory
    assert ra(rays.data_ptr(), out.data_ptr(), 64, 0, None) == 0
    assert ra(rays.data_ptr(), out.data_ptr(), 0, 0, None) == 0         # n == 0: a no-op
    assert lib.drt_renderer_radiance(h, None, rays.data_ptr(), out.data_ptr(), 64, 0, None) == INV
    assert ra(None, out.data_ptr(), 64, 0, None) == INV
    assert ra(rays.data_ptr(), None, 64, 0, None) == INV
    assert ra(rays.data_ptr() + 4, out.data_ptr(), 16, 0, None) == INV
    assert ra(rays.data_ptr(), out.data_ptr() + 4, 16, 0, None) == INV
    assert ra(host.ctypes.data, out.data_ptr(), 64, 0, None) == INV
    assert ra(rays.data_ptr(), out.data_ptr(), 0x80000000, 0, None) == INV
    if torch.cuda.device_count() > 1:                                   # another device's memory
        other = torch.zeros((64, 8), dtype=torch.float32, device=torch.device("cuda", 1))
        assert ra(other.data_ptr(), out.data_ptr(), 64, 0, None) == INV
    r.m_RendererSettings = drt.RendererSettings(RenderMode=1)
    r._push_settings()
    assert ra(rays.data_ptr(), out.data_ptr(), 64, 0, None) == UNS      # debug views stay the framebuffer's
    r.m_RendererSettings = drt.RendererSettings()
    r._push_settings()
    r.RenderBatchAsync(drt.Camera(), sc, 1)
    assert ra(rays.data_ptr(), out.data_ptr(), 64, 0, None) == INV      # an async batch is pending
    assert cr(pod, 1, 8, 8, 1, rays.data_ptr(), None) == INV
    r.Wait()
    assert ra(rays.data_ptr(), out.data_ptr(), 64, 0, None) == 0
    # (a tree deeper than 64 levels -> DRT_ERR_UNSUPPORTED: the builder makes no such tree, see test_gpu_ray_query.py)
    torch.cuda.synchronize()


def test_no_side_effects_and_sharded_renderers_may_call():
    sc, _ = scene_pair("cornell_box")
    (cam, _), = cameras("cornell_box")
    r = drt.Renderer(0)
    r.m_RendererSettings, _ = settings(3, 1)
    r.ResizeBuffer(W, H)
    r.setCounting(True)
    r.RenderBatch(cam, sc, 2)
    img, acc, n, info, cnt = r.GetRenderTargetImage(), r.GetAccumulationBuffer(), r.getSampleCount(), r.kernelInfo(), r.getCounters().as_dict()
    views = r.renderViews([cam], sc, 16, 8, 2)
    assert np.array_equal(u32(r.GetRenderTargetImage()), u32(img)) and np.array_equal(u32(r.GetAccumulationBuffer()), u32(acc))
    assert r.getSampleCount() == n and r.kernelInfo() == info and r.getCounters().as_dict() == cnt
    s = drt.Renderer(0)                                  # a sharded renderer: its stripes are not involved
    s.m_RendererSettings = r.m_RendererSettings
    s.setShard(4, 1, 2)
    s.ResizeBuffer(16, 8)
    assert np.array_equal(u32(s.renderViews([cam], sc, 16, 8, 2)), u32(views))
