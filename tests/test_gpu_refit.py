"""The device refit (drt_renderer_refit, kernel_refit.hip): the renderer's device records equal the host refit's pack byte for byte,
and everything that reads them afterwards -- ray queries, renders, guide buffers -- equals the oracle on the refitted scene of
tests/refit_ref.py.  A refit stays with its renderer, a host change drops it, bad input leaves the host state, stream order holds."""
import numpy as np
import pytest

import oracle
from tests import denoise_ref as dn
from tests import ray_query_ref as rq
from tests import refit_ref as rf
from tests.scenes import SCENES, scene_path

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FAR = ((0.0, 0.5, 12.0), (0.0, -0.05, -1.0))


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make(name):
    """(scene with the editor's BVH, load-order streams, materials, textures, camera position, forward)."""
    if name in ("soup", "chain"):
        s = rq.soup(90000, 1, spread=10.0) if name == "soup" else rq.degenerate_chain()
        sc, _ = rq.programmatic_scene(drt, *s, *((2, 8) if name == "soup" else (1, 2)))
        pose = FAR if name == "soup" else ((-3.0, 0.0, 0.0), (1.0, 0.0, 0.0))
        return sc, tuple(s[:4]), s[4], s[5], pose[0], pose[1]
    sc = drt.Scene()
    sc.loadGLTFmodel(scene_path(name))
    st = rf.streams(sc.m_PrimitivesBuffer)
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
    b.buildIterative(sc)
    osc = oracle.Scene.load_glb(scene_path(name))
    mats = [(tuple(m["albedo"]), int(m["albedo_tex"])) for m in osc.mats[:osc.n_mats]]
    _, pos, fwd, _ = SCENES[name]
    return sc, st, mats, osc.textures, pos, fwd


def jitter(st, seed, scale=0.02):
    rng = np.random.default_rng(seed)
    return (st[0] + rng.normal(0, scale, st[0].shape)).astype(np.float32)


def oracle_scene(sc, st, mats, texs, pos, nrm=None):
    """The oracle's scene after a refit of `sc` (its tree as built) to load-order positions `pos` (normals `nrm` or the stored)."""
    order = sc.triangleOrder()
    osc = oracle.Scene(rf.triangles(pos, st[1] if nrm is None else nrm, st[2], st[3], order=order), mats, texs)
    osc.nodes = rf.oracle_tree(rf.nodes(sc.m_BVHNodes, pos[order]))
    return osc


def assert_records_equal(dev, host, what):
    (di, dh, dr), (hi, hh, hr) = dev, host
    assert di.tobytes() == hi.tobytes(), "%s: InnerNode records differ on %d" % (what, (di != hi).any(axis=1).sum())
    assert u32(dr).tolist() == u32(hr).tolist(), (what, dr, hr)
    d, h = dh.view(np.float32).reshape(-1, 12), hh.view(np.float32).reshape(-1, 12)
    bad = (d.view(np.uint32) != h.view(np.uint32)) & ~(np.isnan(d) & np.isnan(h))       # a NaN face normal may carry another payload
    assert not bad.any(), "%s: TriHot differs on %d triangles" % (what, bad.any(axis=1).sum())


@pytest.mark.parametrize("name", ["cornell_box", "dense_monkey", "cs16_dust", "soup", "chain"])
def test_device_records_equal_the_host_refit(name):
    sc, st, *_ = make(name)
    r = drt.Renderer(0)
    p1, p2 = jitter(st, 1), jitter(st, 2)
    p2[3] = p2[3, 0]                                                     # a zero-area triangle
    n1 = (-st[1]).astype(np.float32)
    ms = r.refit(sc, torch.from_numpy(p1).to(DEV), torch.from_numpy(n1).to(DEV))
    assert ms > 0
    ms = r.refit(sc, torch.from_numpy(p2).to(DEV))                       # normals: the last ones given
    dev = r.debugReadDeviceScene(sc)
    sc.refit(p1, n1)
    sc.refit(p2)
    assert_records_equal(dev, sc.debugPack(), name)


def test_device_build_keeps_the_host_triangle_order():
    s = rq.soup(20000, 4)
    host, _ = rq.programmatic_scene(drt, *s, 4, 8)
    dev = drt.Scene()
    for alb, tex in s[4]:
        dev.addMaterial(alb, tex)
    for t in s[5]:
        dev.addTexture(t)
    dev.setGeometry(*s[:4])
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount, b.m_BuildDevice = 4, 8, 0
    b.buildIterative(dev)
    assert np.array_equal(dev.triangleOrder(), host.triangleOrder())


@pytest.mark.parametrize("name", ["cornell_box", "cs16_dust", "mc_transparency", "soup", "chain"])
def test_ray_queries_after_a_device_refit(name):
    sc, st, mats, texs, pos, fwd = make(name)
    p = jitter(st, 3)
    r = drt.Renderer(0)
    r.refit(sc, torch.from_numpy(p).to(DEV))
    osc = oracle_scene(sc, st, mats, texs, p)
    rng = np.random.default_rng(9)
    org, dirs = rq.camera_rays(oracle.default_camera(position=pos, forward=fwd), 48, 32)
    sets = [(org, dirs, np.float32(0), rq.FLT_MAX), rq.interval_rays(osc, 1000, rng)]
    for o, d, tmin, tmax in sets:
        got = r.traceRays(sc, o, d, tmin, tmax)
        ref = rq.closest(osc, o, d, tmin, tmax)
        for f in ("t", "u", "v"):
            assert (u32(getattr(got, f)) == u32(getattr(ref, f))).all(), (name, f)
        assert (got.prim == ref.prim).all(), name
        occ_tmax = np.float32(np.inf) if tmax is rq.FLT_MAX else tmax
        assert (r.occluded(sc, o, d, tmin, occ_tmax) == rq.occluded(osc, o, d, tmin, occ_tmax)).all(), name


def render_pair(r, sc, osc, pos, fwd, W, H, frames, **kw):
    names = {"enableSunlight": "enable_sunlight", "RenderMode": "render_mode", "DebugMode": "debug_mode"}
    r.m_RendererSettings = drt.RendererSettings(**kw)
    r.ResizeBuffer(W, H)
    r.resetAccumulationBuffer()
    cam = drt.Camera(pos)
    cam.m_Forward_dir = np.array(fwd, np.float32)
    r.RenderBatch(cam, sc, frames)
    ref, _, _ = oracle.render(osc, oracle.default_camera(position=pos, forward=fwd),
                              oracle.default_settings(**{names.get(k, k): v for k, v in kw.items()}), W, H, 1, frames)
    return r.GetRenderTargetImage(), ref


def assert_image(img, ref, what):
    bad = (u32(img) != u32(ref)).any(axis=-1)
    assert not bad.any(), "%s: %d pixels differ (%s)" % (what, bad.sum(), what)


@pytest.mark.parametrize("name,kw", [("cornell_box", dict(ray_bounce_limit=4)), ("cornell_box", dict(ray_bounce_limit=3, enableSunlight=1)),
                                     ("cs16_dust", dict(ray_bounce_limit=3, enableSunlight=1)), ("mc_transparency", dict(ray_bounce_limit=3)),
                                     ("cs16_dust", dict(RenderMode=1, DebugMode=1))])
def test_renders_after_a_device_refit(name, kw):
    sc, st, mats, texs, pos, fwd = make(name)
    r = drt.Renderer(0)
    cam = drt.Camera(pos)
    cam.m_Forward_dir = np.array(fwd, np.float32)
    r.ResizeBuffer(64, 40)
    r.RenderBatch(cam, sc, 1)                                            # the unmoved scene is uploaded and rendered first
    p = jitter(st, 4, 0.05)
    r.refit(sc, torch.from_numpy(p).to(DEV))
    img, ref = render_pair(r, sc, oracle_scene(sc, st, mats, texs, p), pos, fwd, 64, 40, 2, **kw)
    assert ("wave_queue" if "RenderMode" in kw else "path_pool") in r.kernelInfo()
    assert_image(img, ref, "%s %r" % (name, kw))
    W, H = 48, 32                                                         # guides read the refitted copy too
    r.ResizeBuffer(W, H)
    g = r.renderGuides(cam, sc, 1)
    hits = r.traceRays(sc, *dn.camera_rays(oracle.default_camera(position=pos, forward=fwd), W, H))
    assert (g.prim.ravel() == hits.prim).all() and (u32(g.t).ravel() == u32(hits.t)).all()


def test_refit_stays_with_its_renderer_and_host_changes_drop_it():
    sc, st, mats, texs, pos, fwd = make("cornell_box")
    W, H = 48, 32
    moved, other = jitter(st, 5, 0.05), jitter(st, 6, 0.05)
    unmoved = oracle_scene(sc, st, mats, texs, st[0])
    a, b = drt.Renderer(0), drt.Renderer(0)
    a.refit(sc, torch.from_numpy(moved).to(DEV))
    img, ref = render_pair(a, sc, oracle_scene(sc, st, mats, texs, moved), pos, fwd, W, H, 1, ray_bounce_limit=3)
    assert_image(img, ref, "refitted renderer")
    img, ref = render_pair(b, sc, unmoved, pos, fwd, W, H, 1, ray_bounce_limit=3)
    assert_image(img, ref, "second renderer")
    sc.refit(other)                                                      # host refit: the revision moves, a uploads again
    img, ref = render_pair(a, sc, oracle_scene(sc, st, mats, texs, other), pos, fwd, W, H, 1, ray_bounce_limit=3)
    assert_image(img, ref, "after a host refit")
    bad = torch.from_numpy(moved).to(DEV)
    bad[2, 1, 0] = float("nan")
    with pytest.raises(drt.DrtError) as e:
        a.refit(sc, bad)
    assert e.value.code == drt.ERR_INVALID
    img, ref = render_pair(a, sc, oracle_scene(sc, st, mats, texs, other), pos, fwd, W, H, 1, ray_bounce_limit=3)
    assert_image(img, ref, "after a refused refit")
    assert drt._lib.drt_renderer_refit(a._h, sc._h, moved.ctypes.data, None, None, None) == drt.ERR_INVALID     # host memory
    assert drt._lib.drt_renderer_refit(a._h, sc._h, None, None, None, None) == drt.ERR_INVALID
    with pytest.raises(drt.DrtError) as e:
        a.refit(sc, torch.from_numpy(moved[:-1]).to(DEV))                # one triangle short (the binding checks the size)
    assert e.value.code == drt.ERR_INVALID


def test_refit_on_a_side_stream_orders_with_queries_there():
    sc, st, mats, texs, pos, fwd = make("cs16_dust")
    p = jitter(st, 7, 0.05)
    osc = oracle_scene(sc, st, mats, texs, p)
    org, dirs = rq.camera_rays(oracle.default_camera(position=pos, forward=fwd), 48, 32)
    r = drt.Renderer(0)
    r.traceRays(sc, org, dirs)
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(1000000)
        pt = torch.from_numpy(p).to(DEV, non_blocking=True)
        r.refit(sc, pt)
        ot, dt = torch.from_numpy(org).to(DEV), torch.from_numpy(dirs).to(DEV)
        hits = r.traceRays(sc, ot, dt)
        prim, t = hits.prim.clone(), hits.t.clone()
    s.synchronize()
    ref = rq.closest(osc, org, dirs, np.float32(0), rq.FLT_MAX)
    assert (prim.cpu().numpy() == ref.prim).all() and (u32(t.cpu().numpy()) == u32(ref.t)).all()
