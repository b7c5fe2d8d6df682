"""drt_renderer_upscale on the GPU (kernel_upscale.hip): the kernel against the restatement in tests/upscale_ref.py on made-up guides,
the full-size guides bit-equal to a renderer's own at that size, identity at equal sizes, the denoised target as the source,
deterministic, free of side effects, worth running, and the error codes of include/drt.h."""
import ctypes as C

import numpy as np
import pytest

from tests import ray_query_ref as rq
from tests import upscale_ref as up
from tests.scenes import SCENES, scene_path

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

_cache = {}
# One expf per tap on display-referred colour: the a-trous test's tolerance (tests/test_gpu_denoise.py)
TOL = 5e-5
# Largest |float32 - float64 restatement| over the made-up inputs with demodulate 1 (values up to 65: colour / 0.01), measured on
# the CPU: DEMOD_MEASURED.  The tolerance for demodulated output is four times what the test measures, or TOL if that is larger.
DEMOD_MEASURED = 2.75e-6


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def scene(name):
    """(product scene, camera position, forward, bounce limit)"""
    if name not in _cache:
        if name == "chain":
            sc, _ = rq.programmatic_scene(drt, *rq.degenerate_chain(), 1, 2)
            assert sc.bvh_depth == 43
            _cache[name] = (sc, (-3.0, 0.0, 0.0), (1.0, 0.0, 0.0), 3)
        else:
            sc = drt.Scene()
            sc.loadGLTFmodel(scene_path(name))
            b = drt.BVHBuilder()
            b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
            b.buildIterative(sc)
            _, pos, fwd, depth = SCENES[name]
            _cache[name] = (sc, pos, fwd, depth)
    return _cache[name]


def camera(pos, fwd):
    cam = drt.Camera(pos)
    cam.m_Forward_dir = np.array(fwd, np.float32)
    return cam


def renderer(W, H, depth, **settings):
    r = drt.Renderer(0)
    r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=depth, **settings)
    r.ResizeBuffer(W, H)
    return r


def guides_at(cam, sc, W, H):
    """Frame 1's guides of a renderer resized to W x H"""
    r = drt.Renderer(0)
    r.ResizeBuffer(W, H)
    return r.renderGuides(cam, sc, 1)


def demod_tolerance():
    if "tol1" not in _cache:
        worst = 0.0
        for sz in up.MADE_UP_SIZES:
            c, lo, hi = up.made_up(*sz)
            par = dict(up.EXACT, demodulate=1)
            worst = max(worst, float(np.abs(up.upscale(c, lo, hi, **par) - up.upscale(c, lo, hi, dtype=np.float64, **par)).max()))
        print("demodulate 1: max |float32 - float64 restatement| on the made-up inputs = %.3e (recorded %.3e)" % (worst, DEMOD_MEASURED))
        _cache["tol1"] = max(4 * worst, TOL)
    return _cache["tol1"]


@pytest.mark.parametrize("demodulate", [0, 1])
@pytest.mark.parametrize("W,H,Wo,Ho", up.MADE_UP_SIZES)
def test_kernel_matches_the_restatement_on_made_up_guides(W, H, Wo, Ho, demodulate):
    """drt_debug_upscale against upscale_ref.upscale on upscale_ref.made_up (tests/test_upscale_ref.py asserts from the stage map
    that these inputs hold every stage, taps of the other class, e == 16 and just above, a stage-2 tie and NaN guides), with the
    exact sigmas and with the defaults.  demodulate 0: max |GPU - ref| <= 5e-5.  demodulate 1: four times the largest |float32 -
    float64 restatement| on these inputs (measured on the CPU: 2.75e-6, so 1.1e-5), or 5e-5 if larger: 5e-5."""
    c, lo, hi = up.made_up(W, H, Wo, Ho)
    tol = demod_tolerance() if demodulate else TOL
    for par in (up.EXACT, dict(sigma_normal=0.1, sigma_depth=0.05, sigma_albedo=0.1, albedo_floor=0.01)):
        ref, stage = up.upscale(c, lo, hi, stages=True, demodulate=demodulate, **par)
        out = drt.debug_upscale(c, up.pack_guides(lo), up.pack_guides(hi), demodulate=demodulate, **par)
        assert out.shape == (Ho, Wo, 4) and np.isfinite(out).all() and (out[..., 3] == 1).all()
        diff = np.abs(out - ref).max(axis=-1)
        print("%dx%d -> %dx%d demodulate %d sigma_normal %g: max |GPU - restatement| = %.3e (tolerance %.1e); by stage %s"
              % (W, H, Wo, Ho, demodulate, par["sigma_normal"], diff.max(), tol, [float(diff[stage == k].max()) if (stage == k).any() else None for k in (1, 2, 3)]))
        assert diff.max() <= tol
        assert (u32(out)[stage != 1] == u32(ref)[stage != 1]).all()     # stages 2 and 3 copy a value (and scale it): no expf, bit-equal


CASES = [("cornell_box", 48, 32, 96, 64), ("uv_texture_test", 48, 32, 96, 64), ("mc_transparency", 48, 32, 96, 64), ("chain", 48, 32, 96, 64),
         ("cornell_box", 7, 3, 16, 9)]


@pytest.mark.parametrize("name,W,H,Wo,Ho", CASES)
def test_upscale_uses_the_guides_of_a_renderer_at_the_output_size(name, W, H, Wo, Ho):
    """Upscale == the restatement fed with this renderer's image and guides and the guides of a second renderer resized to Wo x Ho:
    the full-size guide pass inside drt_renderer_upscale is drt_renderer_render_guides at that size."""
    sc, pos, fwd, depth = scene(name)
    cam = camera(pos, fwd)
    r = renderer(W, H, depth)
    r.RenderBatch(cam, sc, 2)
    img, lo = r.GetRenderTargetImage(), r.renderGuides(cam, sc, 1)
    hi = guides_at(cam, sc, Wo, Ho)
    assert (hi.prim >= 0).any()
    seen = set()
    for demodulate in (0, 1):
        ref, stage = up.upscale(img, lo, hi, stages=True, demodulate=demodulate)
        out = r.Upscale(cam, sc, Wo, Ho, demodulate=demodulate)
        diff = float(np.abs(out - ref).max())
        print("%s %dx%d -> %dx%d demodulate %d: max |Upscale - restatement| = %.3e, stages %s"
              % (name, W, H, Wo, Ho, demodulate, diff, [int((stage == k).sum()) for k in (1, 2, 3)]))
        assert out.shape == (Ho, Wo, 4) and diff <= (demod_tolerance() if demodulate else TOL)
        assert (u32(out)[stage != 1] == u32(ref)[stage != 1]).all()
        seen |= set(np.unique(stage).tolist())
    assert r.m_LastUpscaleMs > 0 and r.DeviceUpscaledTarget()
    assert (u32(r.GetUpscaledImage()) == u32(out)).all()
    if name != "chain" and Wo > 16:
        assert {1, 2} <= seen, seen                                     # silhouettes reach the search


@pytest.mark.parametrize("W,H", [(96, 64), (7, 3)])
def test_equal_sizes_give_the_framebuffer(W, H):
    sc, pos, fwd, depth = scene("cornell_box")
    cam = camera(pos, fwd)
    r = renderer(W, H, depth)
    r.RenderBatch(cam, sc, 2)
    out = r.Upscale(cam, sc, W, H, demodulate=0)
    assert (u32(out[..., :3]) == u32(r.GetRenderTargetImage()[..., :3])).all() and (out[..., 3] == 1).all()


def test_the_denoised_target_as_the_source():
    sc, pos, fwd, depth = scene("cornell_box")
    cam = camera(pos, fwd)
    W, H, Wo, Ho = 48, 32, 96, 64
    r = renderer(W, H, depth)
    r.Render(cam, sc)
    with pytest.raises(drt.DrtError) as e:
        r.Upscale(cam, sc, Wo, Ho, source=1)                            # before any denoise call
    assert e.value.code == drt.ERR_INVALID
    den = r.TemporalDenoise(cam, sc)
    lo, hi = r.renderGuides(cam, sc, 1), guides_at(cam, sc, Wo, Ho)
    out = r.Upscale(cam, sc, Wo, Ho, source=1)
    assert (u32(r.GetDenoisedImage()) == u32(den)).all()
    assert float(np.abs(out - up.upscale(den, lo, hi)).max()) <= TOL
    img = r.GetRenderTargetImage()
    assert float(np.abs(r.Upscale(cam, sc, Wo, Ho) - up.upscale(img, lo, hi)).max()) <= TOL      # source 0 is still the framebuffer
    assert np.abs(den - img).max() > 1e-3
    den2 = r.Denoise(cam, sc, 2)                                        # the last of Denoise / TemporalDenoise
    assert float(np.abs(r.Upscale(cam, sc, Wo, Ho, source=1) - up.upscale(den2, lo, hi)).max()) <= TOL


def test_upscale_is_deterministic_and_leaves_the_renderer_alone():
    sc, pos, fwd, _ = scene("cornell_box")
    cam = camera(pos, fwd)
    images = []
    for with_upscale in (False, True):
        r = rendered(sc, cam)
        den = r.TemporalDenoise(cam, sc)

        def snapshot():
            return (r.GetAccumulationBuffer(), r.GetRenderTargetImage(), r.GetDenoisedImage(), *r.GetTemporalHistory(), r.getSampleCount(),
                    r.kernelInfo(), r.getCounters().as_dict(), r.kernelSpanMs(), r.DeviceDenoisedTarget(), r.DeviceTemporalHistory(0))
        state = snapshot()
        if with_upscale:
            a = r.Upscale(cam, sc, 192, 128)
            b = r.Upscale(cam, sc, 200, 70, source=1, demodulate=1)     # (another output size: the buffers are allocated again)
            c = r.Upscale(cam, sc, 192, 128)
            assert (u32(a) == u32(c)).all() and b.shape == (70, 200, 4)
            assert (u32(rendered(sc, cam).Upscale(cam, sc, 192, 128)) == u32(a)).all()      # and on a fresh renderer
            after = snapshot()
            for x, y in zip(after[:8], state[:8]):
                assert (u32(x) == u32(y)).all()
            assert after[8:] == state[8:]
            assert (u32(r.TemporalDenoise(cam, sc)) == u32(second_temporal(sc, cam))).all()      # the history went on undisturbed
        else:
            r.TemporalDenoise(cam, sc)
        r.RenderBatch(cam, sc, 2)
        images.append((r.GetRenderTargetImage(), r.getSampleCount(), den))
    assert (u32(images[0][0]) == u32(images[1][0])).all() and images[0][1] == images[1][1] and (u32(images[0][2]) == u32(images[1][2])).all()


def rendered(sc, cam):
    r = renderer(96, 64, 8)
    r.setCounting(True)
    r.trackMotion(True)
    r.RenderBatch(cam, sc, 2)
    return r


def second_temporal(sc, cam):
    """The second TemporalDenoise of the test above on a renderer that never upscaled"""
    r = rendered(sc, cam)
    r.TemporalDenoise(cam, sc)
    return r.TemporalDenoise(cam, sc)


def test_resize_drops_every_stage_target():
    """ResizeBuffer drops the denoised target, the temporal history and the upscaled image, and the stages that run afterwards give,
    bit for bit, what a renderer gives that only ever had the new size: the buffers are allocated again at that size, the upscaler's
    source 1 reads the target the temporal filter just wrote, and no stage keeps state (history, armed motion) from the old size."""
    sc, pos, fwd, depth = scene("cornell_box")
    cam = camera(pos, fwd)

    def stages(r, Wo, Ho):
        r.RenderBatch(cam, sc, 1)
        r.Denoise(cam, sc)
        r.TemporalDenoise(cam, sc)
        r.motionVectors(cam, sc, prev_cam=cam)
        r.Upscale(cam, sc, Wo, Ho, source=1)
        return (r.GetDenoisedImage(), *r.GetTemporalHistory(), r.GetUpscaledImage())

    a = renderer(32, 16, depth)
    stages(a, 64, 32)
    assert a.DeviceDenoisedTarget() and a.DeviceTemporalHistory(0) and a.DeviceUpscaledTarget()
    a.ResizeBuffer(40, 16)
    assert a.DeviceDenoisedTarget() is None and a.DeviceTemporalHistory(0) is None and a.DeviceUpscaledTarget() is None
    for read in (a.GetDenoisedImage, a.GetTemporalHistory, a.GetUpscaledImage):
        assert _code(read) == drt.ERR_INVALID
    after = stages(a, 80, 32)
    fresh = stages(renderer(40, 16, depth), 80, 32)
    assert after[0].shape == (16, 40, 4) and after[-1].shape == (32, 80, 4) and len(after) == len(fresh) == 7
    for x, y in zip(after, fresh):
        assert x.shape == y.shape and (u32(x) == u32(y)).all()


# MSE(upscaled) / MSE(plain bilinear of the same 80 x 60, 64-spp image) against 512 spp at 160 x 120, measured with the restatement on
# the CPU oracle (which shares the renderer's image bit for bit; only expf differs): the bound is that ratio plus 25 %
ORACLE_RATIO = {"cornell_box": 0.3385, "uv_texture_test": 0.2702}


@pytest.mark.parametrize("name", ["cornell_box", "uv_texture_test"])
def test_upscaling_beats_plain_bilinear(name):
    """80 x 60 at 64 spp upscaled to 160 x 120 against a 160 x 120 render at 512 spp: MSE(upscaled) / MSE(bilinear) < the oracle's
    ratio * 1.25.  Oracle: cornell_box 0.3385 (bound 0.4231), uv_texture_test 0.2702 (bound 0.3378), both with demodulate 0.  With
    demodulate 1 the oracle measures 167.8 and 633.6 -- no gain on the textured scene (nor on the other), so the default is
    demodulate 0 and nothing is asserted of demodulate 1 (include/drt.h says why); its ratio is printed."""
    sc, pos, fwd, depth = scene(name)
    cam = camera(pos, fwd)
    r = renderer(80, 60, depth, max_samples=1000)
    r.RenderBatch(cam, sc, 64)
    low = r.GetRenderTargetImage()
    out = r.Upscale(cam, sc, 160, 120)
    out1 = r.Upscale(cam, sc, 160, 120, demodulate=1)
    t = renderer(160, 120, depth, max_samples=1000)
    t.RenderBatch(cam, sc, 512)
    truth = t.GetRenderTargetImage()
    assert t.getSampleCount() == 513
    base = up.mse(up.bilinear(low, 160, 120), truth)
    ratio, ratio1 = up.mse(out, truth) / base, up.mse(out1, truth) / base
    print("%s 80x60 -> 160x120: MSE upscaled / bilinear = %.4f (oracle %.4f, bound %.4f); with demodulate 1: %.1f"
          % (name, ratio, ORACLE_RATIO[name], 1.25 * ORACLE_RATIO[name], ratio1))
    assert ratio < 1.25 * ORACLE_RATIO[name]


def _code(fn):
    with pytest.raises(drt.DrtError) as e:
        fn()
    return e.value.code


def test_error_codes():
    sc, pos, fwd, _ = scene("cornell_box")
    cam = camera(pos, fwd)
    L = drt._lib
    r = drt.Renderer(0)
    pod, p, ms = cam._pod(), drt.UpscaleParams(), C.c_float(0)
    assert _code(lambda: r.Upscale(cam, sc, 64, 32)) == drt.ERR_INVALID                       # no frame size
    r.ResizeBuffer(32, 16)
    assert _code(lambda: r.GetUpscaledImage()) == drt.ERR_INVALID and r.DeviceUpscaledTarget() is None      # before the first call
    h = r._h
    for args in ((None, C.byref(pod), sc._h, 64, 32, C.byref(p), C.byref(ms)), (h, None, sc._h, 64, 32, C.byref(p), C.byref(ms)),
                 (h, C.byref(pod), None, 64, 32, C.byref(p), C.byref(ms)), (h, C.byref(pod), sc._h, 64, 32, None, C.byref(ms))):
        assert L.drt_renderer_upscale(*args) == drt.ERR_INVALID
    for size in ((31, 16), (32, 15), (0, 0), (1 << 16, (1 << 15) + 1)):                      # smaller in either axis, more than 2^31 pixels
        assert _code(lambda: r.Upscale(cam, sc, *size)) == drt.ERR_INVALID, size
    for bad in (dict(source=2), dict(source=-1), dict(source=1), dict(demodulate=2), dict(demodulate=-1), dict(sigma_normal=0.0),
                dict(sigma_depth=-1.0), dict(sigma_albedo=float("nan")), dict(sigma_depth=float("inf")), dict(albedo_floor=0.0),
                dict(albedo_floor=float("nan"))):
        assert _code(lambda: r.Upscale(cam, sc, 64, 32, **bad)) == drt.ERR_INVALID, bad
    assert r.DeviceUpscaledTarget() is None
    assert L.drt_renderer_upscale(h, C.byref(pod), sc._h, 64, 32, C.byref(p), None) == drt.OK     # delta_ms is optional
    buf = np.zeros(64 * 32 * 4, np.float32)
    assert L.drt_renderer_read_upscaled_rgba32f(h, buf.ctypes.data, buf.size) == drt.OK
    assert L.drt_renderer_read_upscaled_rgba32f(h, buf.ctypes.data, buf.size - 1) == drt.ERR_INVALID  # dst too short
    assert L.drt_renderer_read_upscaled_rgba32f(h, None, buf.size) == drt.ERR_INVALID
    r.Denoise(cam, sc)
    assert r.Upscale(cam, sc, 32, 16, source=1).shape == (16, 32, 4)                         # the frame size itself is accepted
    r.RenderBatchAsync(cam, sc, 1)                                                           # a pending asynchronous batch
    assert _code(lambda: r.Upscale(cam, sc, 64, 32)) == drt.ERR_INVALID
    r.Wait()
    r.Upscale(cam, sc, 64, 32)
    r.ResizeBuffer(40, 16)                                                                   # resize frees the result
    assert r.DeviceUpscaledTarget() is None and _code(lambda: r.GetUpscaledImage()) == drt.ERR_INVALID
    s = drt.Renderer(0)                                                                      # a sharded renderer
    s.setShard(8, 0, 2)
    s.ResizeBuffer(32, 32)
    assert _code(lambda: s.Upscale(cam, sc, 64, 64)) == drt.ERR_UNSUPPORTED
    broken = drt.Scene()                                                                     # a scene that cannot be rendered fails as rendering it would
    broken.setGeometry(np.float32([[0, 0, 0, 1, 0, 0, 0, 1, 0]]), np.zeros((1, 9), np.float32), np.zeros((1, 6), np.float32), [3])
    drt.BVHBuilder().buildIterative(broken)
    assert _code(lambda: r.Upscale(cam, broken, 80, 32)) == _code(lambda: r.Render(cam, broken))
    assert r.DeviceUpscaledTarget() is None
    # (a tree deeper than 64 levels -> DRT_ERR_UNSUPPORTED through the guide pass: the builder makes no such tree, see test_gpu_ray_query.py)
