"""First-hit guide buffers and the a-trous denoiser on the GPU (drt_renderer_render_guides / drt_renderer_denoise,
kernel_denoise.hip): guides bit-equal to the renderer's own debug views and ray queries, the filter equal to the restatement in
tests/denoise_ref.py, deterministic, free of side effects, worth running, and the error codes of include/drt.h."""
import os
import subprocess

import numpy as np
import pytest

import oracle
from tests import denoise_ref as dn
from tests import ray_query_ref as rq
from tests.scenes import ROOT, SCENES, scene_path

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FAR = ((0.0, 0.5, 12.0), (0.0, -0.05, -1.0))          # the ray-query tests' view of the programmatic scenes
_cache = {}


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def scene(name):
    """(product scene, camera position, forward) -- glTF scenes with the editor's BVH, the two programmatic trees of the ray-query tests."""
    if name not in _cache:
        if name == "soup":
            sc, _ = rq.programmatic_scene(drt, *rq.soup(90000, 1, spread=10.0), 2, 8)
            assert len(sc.m_BVHNodes) > 65535
            _cache[name] = (sc,) + FAR
        elif name == "chain":
            sc, _ = rq.programmatic_scene(drt, *rq.degenerate_chain(), 1, 2)
            assert sc.bvh_depth == 43
            _cache[name] = (sc, (-3.0, 0.0, 0.0), (1.0, 0.0, 0.0))
        else:
            sc = drt.Scene()
            sc.loadGLTFmodel(scene_path(name))
            b = drt.BVHBuilder()
            b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
            b.buildIterative(sc)
            _, pos, fwd, _ = SCENES[name]
            _cache[name] = (sc, pos, fwd)
    return _cache[name]


def camera(pos, fwd):
    cam = drt.Camera(pos)
    cam.m_Forward_dir = np.array(fwd, np.float32)
    return cam


def one_frame_sum(sc, cam, W, H, frame, **settings):
    """The running sum after frame `frame` alone, 0 + c_frame: frames 1 .. frame-1 rendered into a caller-owned sum that is
    then zeroed, then frame `frame`."""
    r = drt.Renderer(0)
    r.m_RendererSettings = drt.RendererSettings(**settings)
    r.ResizeBuffer(W, H)
    acc = torch.zeros((H, W, 3), dtype=torch.float32, device=DEV)
    rgba = torch.zeros((H, W, 4), dtype=torch.float32, device=DEV)
    r.bindBuffers(acc.data_ptr(), rgba.data_ptr())
    torch.cuda.synchronize()
    if frame > 1:
        r.RenderBatch(cam, sc, frame - 1)
        torch.cuda.synchronize()
        acc.zero_()
        torch.cuda.synchronize()
    r.Render(cam, sc)
    torch.cuda.synchronize()
    out = acc.cpu().numpy()
    r.bindBuffers(None, None)
    return out


GUIDE_CASES = [("cornell_box", 96, 64), ("uv_texture_test", 96, 64), ("mc_transparency", 96, 64), ("cs16_dust", 96, 64),
               ("soup", 64, 48), ("chain", 64, 48), ("cornell_box", 1, 1), ("cornell_box", 7, 3)]


@pytest.mark.parametrize("name,W,H", GUIDE_CASES)
@pytest.mark.parametrize("frame", [1, 3])
def test_guides_bit_equal_to_debug_views_and_ray_queries(name, W, H, frame):
    sc, pos, fwd = scene(name)
    cam = camera(pos, fwd)
    r = drt.Renderer(0)
    r.ResizeBuffer(W, H)
    g = r.renderGuides(cam, sc, frame)
    assert g.albedo.shape == (H, W, 3) and g.normal.shape == (H, W, 3) and g.t.shape == (H, W) and g.prim.dtype == np.int32
    albedo = one_frame_sum(sc, cam, W, H, frame, RenderMode=1, DebugMode=0, tone_mapping=0, gamma_correction=0)
    normal = one_frame_sum(sc, cam, W, H, frame, RenderMode=1, DebugMode=1)
    bad = (u32(g.albedo) != u32(albedo)).any(axis=-1)
    assert not bad.any(), "%s frame %d: albedo differs on %d pixels" % (name, frame, bad.sum())
    hit = g.prim >= 0
    bad = (u32(g.normal) != u32(normal)).any(axis=-1) & hit
    assert not bad.any(), "%s frame %d: normal differs on %d hit pixels" % (name, frame, bad.sum())
    assert (u32(g.normal)[~hit] == 0).all()
    org, dirs = dn.camera_rays(oracle.default_camera(position=pos, forward=fwd), W, H, frame)
    hits = r.traceRays(sc, org, dirs)
    assert (g.prim.ravel() == hits.prim).all(), "%s frame %d: prim differs on %d pixels" % (name, frame, (g.prim.ravel() != hits.prim).sum())
    assert (u32(g.t).ravel() == u32(hits.t)).all()
    assert (u32(g.t)[~hit] == u32(np.float32(rq.FLT_MAX))).all()
    if W * H > 100:
        assert hit.any() and (name in ("cs16_dust", "chain") or (~hit).any())


def test_guides_match_the_restatement_and_the_torch_path():
    """cornell_box frame 2 against the oracle's debug renders + the CPU traversal; as_torch=True on a side stream gives the same bits."""
    name, W, H = "cornell_box", 48, 32
    sc, pos, fwd = scene(name)
    cam = camera(pos, fwd)
    r = drt.Renderer(0)
    r.ResizeBuffer(W, H)
    g = r.renderGuides(cam, sc, 2)
    osc = oracle.Scene.load_glb(scene_path(name)).build_bvh(20, 8)
    ref = dn.guides(osc, oracle.default_camera(position=pos, forward=fwd), W, H, 2)
    for field in ("albedo", "normal", "t"):
        assert (u32(getattr(g, field)) == u32(getattr(ref, field))).all(), field
    assert (g.prim == ref.prim).all()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(1000000)
        gt = r.renderGuides(cam, sc, 2, as_torch=True)
        alb = gt.albedo.clone()
    assert all(x.device == torch.device(DEV) for x in gt)
    s.synchronize()
    assert (u32(alb.cpu().numpy()) == u32(g.albedo)).all()
    assert (gt.prim.cpu().numpy() == g.prim).all() and (u32(gt.t.cpu().numpy()) == u32(g.t)).all()


FILTER_CASES = [("suzanne_plane", 320, 200), ("cornell_box", 96, 64), ("uv_texture_test", 96, 64), ("mc_transparency", 80, 56), ("cs16_dust", 80, 56),
                ("soup", 64, 48), ("chain", 64, 48), ("cornell_box", 1, 1), ("cornell_box", 7, 3)]
SIGMAS = [dict(sigma_color=0.5, sigma_normal=0.1, sigma_albedo=0.1), dict(sigma_color=0.8, sigma_normal=0.35, sigma_albedo=0.05)]
_max_diff = []


@pytest.mark.parametrize("name,W,H", FILTER_CASES)
def test_filter_matches_the_restatement(name, W, H):
    sc, pos, fwd = scene(name)
    cam = camera(pos, fwd)
    r = drt.Renderer(0)
    r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=SCENES.get(name, (0, 0, 0, 3))[3])
    r.ResizeBuffer(W, H)
    r.RenderBatch(cam, sc, 3)
    img = r.GetRenderTargetImage()
    g = r.renderGuides(cam, sc, 1)
    worst = 0.0
    for K in (0, 1, 5, 7):                        # (steps up to 64: at these sizes lattice tiles in LDS up to step 16 at most, cache-read taps above;
                                                      #  the LDS kernel at larger steps and both at steps 128 .. 512: test_gpu_filter_kernels.py)
        for sig in SIGMAS:
            out = r.Denoise(cam, sc, K, **sig)
            if K == 0:
                assert (u32(out) == u32(img)).all()
            ref = dn.atrous(img, g.albedo, g.normal, K, **sig)
            diff = float(np.abs(out - ref).max())
            assert diff <= 5e-5, (name, K, sig, diff)
            assert (u32(out[..., 3]) == u32(img[..., 3])).all()
            worst = max(worst, diff)
    _max_diff.append(worst)
    print("%s %dx%d: max |Denoise - atrous()| = %.3e (all K, sigmas; largest so far %.3e)" % (name, W, H, worst, max(_max_diff)))


def test_denoise_and_guides_are_deterministic():
    sc, pos, fwd = scene("mc_transparency")
    cam = camera(pos, fwd)
    r = drt.Renderer(0)
    r.ResizeBuffer(200, 120)
    r.RenderBatch(cam, sc, 2)
    a = r.Denoise(cam, sc)
    b = r.Denoise(cam, sc)
    assert (u32(a) == u32(b)).all()
    assert r.m_LastDenoiseMs > 0
    g1, g2 = r.renderGuides(cam, sc, 1), r.renderGuides(cam, sc, 1)
    for x, y in zip(g1, g2):
        assert (np.ascontiguousarray(x).view(np.uint32) == np.ascontiguousarray(y).view(np.uint32)).all()
    assert r.DeviceDenoisedTarget()
    assert (u32(r.GetDenoisedImage()) == u32(a)).all()


def test_guides_and_denoise_leave_the_renderer_alone():
    sc, pos, fwd = scene("cornell_box")
    cam = camera(pos, fwd)
    images = []
    for with_denoise in (False, True):
        r = drt.Renderer(0)
        r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=8)
        r.ResizeBuffer(96, 64)
        r.setCounting(True)
        r.RenderBatch(cam, sc, 2)
        state = (r.GetAccumulationBuffer(), r.GetRenderTargetImage(), r.getSampleCount(), r.kernelInfo(), r.getCounters().as_dict(),
                 r.kernelSpanMs())
        if with_denoise:
            r.renderGuides(cam, sc, 1)
            r.renderGuides(cam, sc, 4)
            r.Denoise(cam, sc)
            r.Denoise(cam, sc, 0)
            after = (r.GetAccumulationBuffer(), r.GetRenderTargetImage(), r.getSampleCount(), r.kernelInfo(), r.getCounters().as_dict(),
                     r.kernelSpanMs())
            assert (u32(after[0]) == u32(state[0])).all() and (u32(after[1]) == u32(state[1])).all()
            assert after[2:] == state[2:]
        r.RenderBatch(cam, sc, 2)
        images.append((r.GetRenderTargetImage(), r.getSampleCount()))
    assert (u32(images[0][0]) == u32(images[1][0])).all() and images[0][1] == images[1][1]


def test_denoising_lowers_the_noise():
    """cornell_box 160x120: 4 spp denoised against 512 spp, MSE ratio <= 0.25 (the restatement measures 0.132 on the oracle)."""
    sc, pos, fwd = scene("cornell_box")
    cam = camera(pos, fwd)
    W, H = 160, 120
    r = drt.Renderer(0)
    r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=8, max_samples=1000)
    r.ResizeBuffer(W, H)
    r.RenderBatch(cam, sc, 4)
    noisy = r.GetRenderTargetImage()
    out = r.Denoise(cam, sc)
    r.RenderBatch(cam, sc, 508)
    clean = r.GetRenderTargetImage()
    assert r.getSampleCount() == 513
    ratio = dn.mse(out, clean) / dn.mse(noisy, clean)
    print("cornell_box 160x120: MSE denoised / noisy = %.3f" % ratio)
    assert ratio <= 0.25


def _code(fn):
    with pytest.raises(drt.DrtError) as e:
        fn()
    return e.value.code


def test_error_paths():
    import ctypes as C
    sc, pos, fwd = scene("cornell_box")
    cam = camera(pos, fwd)
    L = drt._lib
    r = drt.Renderer(0)
    pod, p, ms = cam._pod(), drt.DenoiseParams(), C.c_float(0)
    # no frame size yet
    assert _code(lambda: r.renderGuides(cam, sc)) == drt.ERR_INVALID
    assert _code(lambda: r.Denoise(cam, sc)) == drt.ERR_INVALID
    r.ResizeBuffer(32, 16)
    assert _code(lambda: r.GetDenoisedImage()) == drt.ERR_INVALID and r.DeviceDenoisedTarget() is None
    g = torch.zeros((16 * 32 + 1, 8), dtype=torch.float32, device=DEV)
    h = r._h
    assert L.drt_renderer_render_guides(h, C.byref(pod), sc._h, 1, g.data_ptr(), None) == drt.OK
    torch.cuda.synchronize()
    for args in ((None, C.byref(pod), sc._h, 1, g.data_ptr(), None), (h, None, sc._h, 1, g.data_ptr(), None),
                 (h, C.byref(pod), None, 1, g.data_ptr(), None), (h, C.byref(pod), sc._h, 1, None, None),
                 (h, C.byref(pod), sc._h, 0, g.data_ptr(), None),                                    # frame index 0
                 (h, C.byref(pod), sc._h, 1, g.data_ptr() + 4, None),                                # misaligned
                 (h, C.byref(pod), sc._h, 1, np.zeros(16 * 32 * 8, np.float32).ctypes.data, None)):  # host memory
        assert L.drt_renderer_render_guides(*args) == drt.ERR_INVALID, args
    if torch.cuda.device_count() > 1:
        g1 = torch.zeros((16 * 32, 8), dtype=torch.float32, device="cuda:1")
        assert L.drt_renderer_render_guides(h, C.byref(pod), sc._h, 1, g1.data_ptr(), None) == drt.ERR_INVALID
    for args in ((None, C.byref(pod), sc._h, C.byref(p), C.byref(ms)), (h, None, sc._h, C.byref(p), C.byref(ms)),
                 (h, C.byref(pod), None, C.byref(p), C.byref(ms)), (h, C.byref(pod), sc._h, None, C.byref(ms))):
        assert L.drt_renderer_denoise(*args) == drt.ERR_INVALID
    for bad in (dict(iterations=-1), dict(iterations=11), dict(sigma_color=0.0), dict(sigma_normal=-1.0), dict(sigma_albedo=float("nan")),
                dict(sigma_color=float("inf"))):
        assert _code(lambda: r.Denoise(cam, sc, **bad)) == drt.ERR_INVALID, bad
    r.Denoise(cam, sc, iterations=10)                     # the bounds themselves are accepted
    r.Denoise(cam, sc, iterations=0)
    # a pending asynchronous batch
    r.RenderBatchAsync(cam, sc, 1)
    assert _code(lambda: r.renderGuides(cam, sc)) == drt.ERR_INVALID
    assert _code(lambda: r.Denoise(cam, sc)) == drt.ERR_INVALID
    r.Wait()
    r.Denoise(cam, sc)
    # resize frees the buffers
    assert r.DeviceDenoisedTarget() is not None
    r.ResizeBuffer(40, 16)
    assert r.DeviceDenoisedTarget() is None and _code(lambda: r.GetDenoisedImage()) == drt.ERR_INVALID
    assert r.Denoise(cam, sc).shape == (16, 40, 4)
    # a sharded renderer
    s = drt.Renderer(0)
    s.setShard(8, 0, 2)
    s.ResizeBuffer(32, 32)
    assert _code(lambda: s.Denoise(cam, sc)) == drt.ERR_UNSUPPORTED
    assert L.drt_renderer_render_guides(s._h, C.byref(pod), sc._h, 1, g.data_ptr(), None) == drt.ERR_UNSUPPORTED
    # a scene that cannot be rendered fails as rendering it would
    broken = drt.Scene()
    broken.setGeometry(np.float32([[0, 0, 0, 1, 0, 0, 0, 1, 0]]), np.zeros((1, 9), np.float32), np.zeros((1, 6), np.float32), [3])
    b = drt.BVHBuilder()
    b.buildIterative(broken)
    want = _code(lambda: r.Render(cam, broken))
    assert want < 0
    assert _code(lambda: r.renderGuides(cam, broken)) == want
    assert _code(lambda: r.Denoise(cam, broken)) == want
    # (a tree deeper than 64 levels -> DRT_ERR_UNSUPPORTED: the builder makes no such tree, see test_gpu_ray_query.py)


def _read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        W, H = map(int, f.readline().split())
        f.readline()
        return np.frombuffer(f.read(), np.float32).reshape(H, W, 3)


def test_cli_denoise(tmp_path):
    exe = tmp_path / "drt_render"
    lib_dir = os.path.dirname(drt.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "drt_render.cpp"),
                    "-L" + lib_dir, "-ldrt_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    _, pos, fwd, depth = SCENES["cornell_box"]
    args = [str(exe), scene_path("cornell_box"), None, "64", "48", "4", str(depth)] + ["%g" % v for v in pos + fwd]
    plain, den = str(tmp_path / "plain.pfm"), str(tmp_path / "den.pfm")
    out = subprocess.run(args[:2] + [plain] + args[3:], capture_output=True, text=True, check=True).stdout
    assert "denoised" not in out
    out = subprocess.run(args[:2] + [den] + args[3:] + ["--denoise"], capture_output=True, text=True, check=True).stdout
    assert "denoised: 5 passes" in out
    sc, _, _ = scene("cornell_box")
    cam = camera(pos, fwd)
    r = drt.Renderer(0)
    r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=depth, max_samples=5)
    r.ResizeBuffer(64, 48)
    r.RenderBatch(cam, sc, 4)
    assert (u32(_read_pfm(plain)) == u32(r.GetRenderTargetImage()[..., :3])).all()
    assert (u32(_read_pfm(den)) == u32(r.Denoise(cam, sc)[..., :3])).all()
