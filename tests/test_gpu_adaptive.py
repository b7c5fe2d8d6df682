"""Adaptive sampling on the GPU (drt_renderer_render_adaptive, kernel_adaptive.hip).  The yardstick needs no tolerance: a pixel
that has received n samples holds the uniform renderer's accumulation after n frames, bit for bit; weights, counts and moments
equal tests/adaptive_ref.py's restatement, bit for bit; the scan and the counts alone equal numpy at every size where the scan
takes another path; pixel ranges, repetition and a refitted scene change no bit; nothing else of the renderer is touched; the
error codes are include/drt.h's."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import adaptive_ref as ar
from tests import refit_ref as rf
from tests.scenes import SCENES, scene_path

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

W, H = 64, 48
PX = W * H
CALLS, SPP, MAX_SPP = 3, 3, 8                  # (of a config that does not say otherwise)
_scenes, _runs = {}, {}

# name -> (scene, settings[, what the config sets of its own: size (w, h), camera (Camera -> None), material (the model's arguments,
# on both renderers), spp (one per call), max_spp])
CONFIGS = {
    "cornell_box": ("cornell_box", dict(ray_bounce_limit=4)),
    "sunlight": ("cornell_box", dict(ray_bounce_limit=4, enableSunlight=1)),
    "no_tone_curve": ("cornell_box", dict(ray_bounce_limit=4, tone_mapping=0, gamma_correction=0)),
    "alpha_cutouts": ("uv_texture_test", dict(ray_bounce_limit=4)),
    # a thin lens: every camera constant the ray list copies is live (disk_u != disk_v: the camera looks along -x)
    "lens": ("cornell_box", dict(ray_bounce_limit=4), dict(camera=lambda cam: vars(cam).update(
        defocus_angle=1.5, focus_dist=3.0, exposure=2.5, vfov_rad=float(np.float32(np.deg2rad(47.0)))))),
    "odd_size": ("cornell_box", dict(ray_bounce_limit=4), dict(size=(61, 37))),      # 2 257 pixels: no multiple of 8, 64, 256, 1024
    "hbm_scene": ("cs16_dust", dict(ray_bounce_limit=4)),                            # tree and triangles live in HBM
    "materials": ("emissive_test", dict(ray_bounce_limit=4), dict(material=(1, 1, 2.5))),
    # the ray buffers regrow, then are too large: 1, 8, 1 -- three calls the rule makes uniform whatever the pose (n = 1 is unknown;
    # a budget of min_spp per pixel leaves no extra) -- and then the same with ragged counts: 16 regrows them again, 1
    "growing": ("cornell_box", dict(ray_bounce_limit=4), dict(spp=(1, 8, 1, 16, 1), max_spp=32)),
}


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def scene(name):
    if name not in _scenes:
        sc = drt.Scene()
        sc.loadGLTFmodel(scene_path(name))
        streams = rf.streams(sc.m_PrimitivesBuffer)          # (load order: taken before the build)
        b = drt.BVHBuilder()
        b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
        b.buildIterative(sc)
        _scenes[name] = (sc, streams)
    return _scenes[name][0]


def camera(name, setup=None):
    _, pos, fwd, _ = SCENES[name]
    cam = drt.Camera(pos)
    cam.m_Forward_dir = np.array(fwd, np.float32)
    if setup:
        setup(cam)
    return cam


def renderer(settings, w=W, h=H):
    r = drt.Renderer(0)
    r.m_RendererSettings = drt.RendererSettings(**settings)
    r.ResizeBuffer(w, h)
    return r


def state_of(r):
    """The renderer's adaptive state as adaptive_ref.State over the pixels, plus (last_q, last_count)."""
    s = r.GetAdaptiveState()
    return ar.State(s.sum.reshape(-1, 3), s.count.reshape(-1), s.m1.reshape(-1), s.m2.reshape(-1)), s.last_q.reshape(-1), s.last_count.reshape(-1)


def uniform_accumulations(r, cam, sc, frames):
    """accum_after[k] = the accumulation buffer after k Render calls from a reset, [frames + 1, P, 3]."""
    r.resetAccumulationBuffer()
    out = [np.zeros((r.getBufferWidth() * r.getBufferHeight(), 3), np.float32)]
    for _ in range(frames):
        r.Render(cam, sc)
        out.append(r.GetAccumulationBuffer().reshape(-1, 3))
    return np.stack(out)


def run(config):
    """The config's adaptive calls on one renderer (three of SPP unless it says otherwise), everything the tests look at read back
    once; and the uniform renderer's view of the same frames from another one."""
    if config not in _runs:
        name, settings, own = (CONFIGS[config] + ({},))[:3]
        w, h = own.get("size", (W, H))
        spp, max_spp = own.get("spp", (SPP,) * CALLS), own.get("max_spp", MAX_SPP)
        sc, cam = scene(name), camera(name, own.get("camera"))
        plain, r = renderer(settings, w, h), renderer(settings, w, h)
        if "material" in own:
            plain.setMaterialModel(*own["material"])
            r.setMaterialModel(*own["material"])
        steps = []
        before = ar.empty_state(w * h)
        for s in spp:
            info = r.RenderAdaptive(cam, sc, spp=s, max_spp=max_spp)
            after, q, c = state_of(r)
            steps.append(dict(before=before, after=after, q=q, c=c, info=info, image=r.GetRenderTargetImage().reshape(-1, 4), spp=s))
            before = after
        frames = int(before.n.max())                   # (no pixel has received more samples than this)
        accum_after = uniform_accumulations(plain, cam, sc, frames)
        samples = {k: plain.radiance(sc, plain.cameraRays(cam, w, h, k))[0, ..., :3].reshape(-1, 3) for k in range(1, frames + 1)}
        _runs[config] = dict(steps=steps, accum_after=accum_after, samples=samples, px=w * h, max_spp=max_spp, frames=len(spp) * max_spp)
    return _runs[config]


def assert_bits(got, ref, what):
    bad = u32(got) != u32(ref)
    if bad.ndim > 1:
        bad = bad.any(axis=-1)
    assert not bad.any(), "%s: %d of %d differ, first at %s: %r vs %r" % (
        what, bad.sum(), bad.size, np.argwhere(bad)[0], got[tuple(np.argwhere(bad)[0])], ref[tuple(np.argwhere(bad)[0])])


# ---------------------------------------------------------------- 1. the invariant

@pytest.mark.parametrize("config", list(CONFIGS))
def test_a_pixel_with_n_samples_holds_the_uniform_accumulation_after_n_frames(config):
    d = run(config)
    pixels = np.arange(d["px"])
    for i, st in enumerate(d["steps"]):
        n = st["after"].n
        assert n.max() <= d["frames"] and st["info"].samples == int(st["c"].sum()) <= st["spp"] * d["px"]
        assert_bits(st["after"].sum, d["accum_after"][n, pixels], "%s call %d: sum vs accumulation after n frames" % (config, i))
        assert_bits(st["image"], ar.image(st["after"]), "%s call %d: framebuffer vs sum / n" % (config, i))
    first, last = d["steps"][0], d["steps"][-1]
    assert (first["c"] == first["spp"]).all() and first["info"].max_count == first["spp"]      # every pixel unknown: uniform
    assert len(np.unique(last["after"].n)) > 2, "the later calls must not be uniform: the test would show nothing"


# ---------------------------------------------------------------- 2. plan and moments equal the restatement

@pytest.mark.parametrize("config", list(CONFIGS))
def test_weights_counts_and_moments_equal_the_restatement(config):
    d = run(config)
    for i, st in enumerate(d["steps"]):
        q, c = ar.plan(st["before"], st["spp"] * d["px"], max_spp=d["max_spp"])
        assert (st["q"] == q).all(), "%s call %d: %d weights differ" % (config, i, (st["q"] != q).sum())
        assert (st["c"] == c).all(), "%s call %d: %d counts differ" % (config, i, (st["c"] != c).sum())
        assert st["info"].active_pixels == int((q > 0).sum()) and st["info"].max_count == int(c.max())
        ref = ar.fold(st["before"], c, lambda k: d["samples"][k])
        assert (st["after"].n == ref.n).all()
        assert_bits(st["after"].m1, ref.m1, "%s call %d: m1" % (config, i))
        assert_bits(st["after"].m2, ref.m2, "%s call %d: m2" % (config, i))
        assert_bits(st["after"].sum, ref.sum, "%s call %d: sum" % (config, i))


# ---------------------------------------------------------------- 3. counts and scan alone

B = 1024                                        # the scan's block (csrc/adaptive.hpp kScanBlock)
CAP = 16777215


def plan_cases(n, rng):
    one = lambda i: np.bincount([i], minlength=n).astype(np.uint32) * np.uint32(77777)
    yield "all zero", np.zeros(n, np.uint32), dict(budget=3 * n + 5, min_spp=2, max_spp=9)
    yield "all cap", np.full(n, CAP, np.uint32), dict(budget=5 * n + n // 2, min_spp=1, max_spp=64)
    for i in sorted({0, n - 1, min(n - 1, B - 1), min(n - 1, B), n // 2}):
        yield "single at %d" % i, one(i), dict(budget=n + 1000, min_spp=1, max_spp=300)
    q = rng.integers(0, CAP + 1, n, dtype=np.uint32)
    q[rng.random(n) < 0.25] = 0
    yield "random", q, dict(budget=n + 40 * n, min_spp=1, max_spp=50)
    yield "random, budget near 2^31", q, dict(budget=(1 << 31) - 1, min_spp=0, max_spp=(1 << 31) - 1)


@pytest.mark.parametrize("n", [1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1, B * B + 1])
def test_counts_and_scan_alone_equal_numpy(n):
    rng = np.random.default_rng(n)
    for what, q, params in plan_cases(n, rng):
        for th in (False, True):
            counts, offsets, Q = drt.debug_adaptive_plan(q, thresholded=th, **params)
            ref, ref_Q = ar.counts(q, params["budget"], params["min_spp"], params["max_spp"], thresholded=th)
            assert Q == ref_Q, (n, what, th)
            assert (counts == ref).all(), (n, what, th, int((counts != ref).sum()))
            assert (offsets == ar.offsets(ref)).all(), (n, what, th, int(np.argmax(offsets != ar.offsets(ref))))
            assert int(ref.sum(dtype=np.uint64)) <= params["budget"]


# ---------------------------------------------------------------- 4. pixel ranges

def _renderer_with_env(env, settings):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return renderer(settings)               # the knobs are read when the renderer is created
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_pixel_ranges_change_no_bit():
    sc, cam = scene("cornell_box"), camera("cornell_box")
    settings = dict(ray_bounce_limit=4)
    whole, split = renderer(settings), _renderer_with_env({"DRT_SAMPLE_MB": "1"}, settings)
    for call in range(2):                       # the second call's counts are ragged
        a, b = (r.RenderAdaptive(cam, sc, spp=24, max_spp=64) for r in (whole, split))
        assert 48 * b.samples > 3 << 20, "more than three ranges of at most 1 MiB each"
        assert (a.samples, a.active_pixels, a.max_count) == (b.samples, b.active_pixels, b.max_count)
        for x, y in zip(whole.GetAdaptiveState(), split.GetAdaptiveState()):
            assert (x.view(np.uint32) == y.view(np.uint32)).all(), call
        assert_bits(split.GetRenderTargetImage(), whole.GetRenderTargetImage(), "image, call %d" % call)
    assert len(np.unique(whole.GetAdaptiveState().last_count)) > 2


# ---------------------------------------------------------------- 5. convergence

def test_a_converged_frame_gets_nothing_and_stays_as_it_is():
    sc = scene("cornell_box")
    cam = drt.Camera((1000.0, 1000.0, 1000.0))                  # sees only sky
    cam.m_Forward_dir = np.array([1.0, 0.2, 0.0], np.float32)
    r = renderer(dict(ray_bounce_limit=4))
    first = r.RenderAdaptive(cam, sc, spp=4, target_error=1e-3)
    assert (first.samples, first.active_pixels) == (4 * PX, PX)
    before, image = r.GetAdaptiveState(), r.GetRenderTargetImage()
    second = r.RenderAdaptive(cam, sc, spp=4, target_error=1e-3)
    assert (second.active_pixels, second.samples, second.max_count) == (0, 0, 0)
    after = r.GetAdaptiveState()
    for name in ("sum", "count", "m1", "m2"):
        assert (getattr(before, name).view(np.uint32) == getattr(after, name).view(np.uint32)).all(), name
    assert (after.last_q == 0).all() and (after.last_count == 0).all()
    assert_bits(r.GetRenderTargetImage(), image, "image")


def test_converged_pixels_receive_no_samples():
    sc, cam = scene("cornell_box"), camera("cornell_box")
    r = renderer(dict(ray_bounce_limit=4))
    seen = 0
    for _ in range(4):
        st0, _, _ = state_of(r) if r.DeviceAdaptiveState() else (ar.empty_state(PX), None, None)
        info = r.RenderAdaptive(cam, sc, spp=4, max_spp=16, target_error=0.05)
        st, q, c = state_of(r)
        assert (c[q == 0] == 0).all() and (c[q > 0] >= 1).all()
        assert (st.n[q == 0] == st0.n[q == 0]).all()
        assert info.active_pixels == int((q > 0).sum()) and info.samples == int(c.sum()) <= 4 * PX
        seen += int((q == 0).sum())
    assert seen > 0, "no pixel ever converged: the test would show nothing"


# ---------------------------------------------------------------- 6. the same bits twice, also after a refit on the device

def test_same_bits_twice_and_the_samples_follow_a_device_refit():
    sc, cam = scene("cornell_box"), camera("cornell_box")
    pos = _scenes["cornell_box"][1][0]
    moved = (pos + np.random.default_rng(5).normal(0, 0.02, pos.shape)).astype(np.float32)
    settings = dict(ray_bounce_limit=4)
    r = renderer(settings)
    r.refit(sc, moved)
    runs = []
    for _ in range(2):
        r.resetAdaptive()
        for _ in range(2):
            r.RenderAdaptive(cam, sc, spp=3, max_spp=8)
        runs.append((r.GetAdaptiveState(), r.GetRenderTargetImage()))
    for x, y in zip(runs[0][0], runs[1][0]):
        assert (x.view(np.uint32) == y.view(np.uint32)).all()
    assert_bits(runs[0][1], runs[1][1], "image")
    st = runs[0][0]
    n = st.count.reshape(-1)
    accum_after = uniform_accumulations(r, cam, sc, int(n.max()))        # the same renderer: the refitted copy
    assert_bits(st.sum.reshape(-1, 3), accum_after[n, np.arange(PX)], "sum vs the refitted renderer's accumulation")
    still = run("cornell_box")["accum_after"]
    assert (u32(accum_after[1]) != u32(still[1])).any(), "the refit must change the image: the test would show nothing"


# ---------------------------------------------------------------- 7. no side effects

def test_nothing_else_is_touched():
    sc, cam = scene("cornell_box"), camera("cornell_box")
    settings = dict(ray_bounce_limit=4)
    r, twin = renderer(settings), renderer(settings)
    for x in (r, twin):
        x.setCounting(True)
        x.RenderBatch(cam, sc, 2)
        x.TemporalDenoise(cam, sc)
    accum, count, counters = r.GetAccumulationBuffer(), r.getSampleCount(), r.getCounters().as_dict()
    history, denoised, info, span = r.GetTemporalHistory(), r.GetDenoisedImage(), r.kernelInfo(), r.kernelSpanMs()
    assert r.DeviceAdaptiveState() is None
    with pytest.raises(drt.DrtError) as e:
        r.GetAdaptiveState()                                    # a read before the first call
    assert e.value.code == drt.ERR_INVALID
    r.RenderAdaptive(cam, sc, spp=2)
    r.RenderAdaptive(cam, sc, spp=2)
    st, _, _ = state_of(r)
    assert_bits(r.GetRenderTargetImage().reshape(-1, 4), ar.image(st), "the framebuffer shows sum / n")
    assert_bits(r.GetAccumulationBuffer(), accum, "accumulation")
    assert r.getSampleCount() == count and r.getCounters().as_dict() == counters
    assert r.kernelInfo() == info and r.kernelSpanMs() == span
    for a, b in zip(r.GetTemporalHistory(), history):
        assert_bits(a, b, "temporal history")
    assert_bits(r.GetDenoisedImage(), denoised, "denoised target")
    # Denoise reads what the adaptive call wrote: the same as on a renderer whose bound framebuffer holds that image
    img = r.GetRenderTargetImage()
    dev = torch.device("cuda", 0)
    acc_t, rgba_t = torch.zeros((H, W, 3), device=dev), torch.from_numpy(img).to(dev)
    other = renderer(settings)
    other.bindBuffers(acc_t.data_ptr(), rgba_t.data_ptr())
    assert_bits(r.Denoise(cam, sc), other.Denoise(cam, sc), "Denoise after an adaptive call")
    other.bindBuffers(None, None)
    # a Render after it yields what a renderer without any adaptive call yields
    r.Render(cam, sc)
    twin.Render(cam, sc)
    assert_bits(r.GetRenderTargetImage(), twin.GetRenderTargetImage(), "Render after an adaptive call")
    assert_bits(r.GetAccumulationBuffer(), twin.GetAccumulationBuffer(), "accumulation after a Render")
    assert state_of(r)[0].n.min() >= 3                         # (Render does not drop the state: 2 samples, then at least min_spp)
    # the adaptive image goes to bound buffers
    r.bindBuffers(acc_t.data_ptr(), rgba_t.data_ptr())
    r.RenderAdaptive(cam, sc, spp=1)
    assert_bits(rgba_t.cpu().numpy().reshape(-1, 4), ar.image(state_of(r)[0]), "bound framebuffer")
    r.bindBuffers(None, None)
    # resetAccumulationBuffer and ResizeBuffer drop the state: the next call is uniform again
    for drop in (r.resetAccumulationBuffer, lambda: r.ResizeBuffer(W - 8, H), r.resetAdaptive):
        assert r.DeviceAdaptiveState() is not None
        drop()
        assert r.DeviceAdaptiveState() is None and r.DeviceAdaptiveState(1) is None
        with pytest.raises(drt.DrtError) as e:
            r.GetAdaptiveState()
        assert e.value.code == drt.ERR_INVALID
        i = r.RenderAdaptive(cam, sc, spp=2)
        s = r.GetAdaptiveState()
        assert (s.count == 2).all() and (s.last_count == 2).all() and (s.last_q == CAP).all() and i.samples == 2 * s.count.size


# ---------------------------------------------------------------- 8. errors

def _code(fn):
    with pytest.raises(drt.DrtError) as e:
        fn()
    return e.value.code


def test_error_codes():
    sc, cam = scene("cornell_box"), camera("cornell_box")
    L = drt._lib
    r = drt.Renderer(0)
    assert _code(lambda: r.RenderAdaptive(cam, sc, budget=16)) == drt.ERR_INVALID              # no frame size
    r.ResizeBuffer(32, 16)
    pod, p, info = cam._pod(), drt.AdaptiveParams(), drt.AdaptiveInfo()
    h = r._h
    for args in ((None, C.byref(pod), sc._h, C.byref(p), C.byref(info)), (h, None, sc._h, C.byref(p), C.byref(info)),
                 (h, C.byref(pod), None, C.byref(p), C.byref(info)), (h, C.byref(pod), sc._h, None, C.byref(info))):
        assert L.drt_renderer_render_adaptive(*args) == drt.ERR_INVALID
    for bad in (dict(min_spp=3, max_spp=2), dict(max_spp=0, min_spp=0), dict(budget=511), dict(budget=1 << 31), dict(min_spp=5),
                dict(target_error=-1.0), dict(target_error=float("nan")), dict(luma_floor=0.0), dict(luma_floor=float("inf"))):
        assert _code(lambda: r.RenderAdaptive(cam, sc, **bad)) == drt.ERR_INVALID, bad
    assert r.DeviceAdaptiveState() is None
    assert L.drt_renderer_render_adaptive(h, C.byref(pod), sc._h, C.byref(p), None) == drt.OK      # info is optional; budget 0 = 4 per pixel
    assert (r.GetAdaptiveState().count == 4).all()
    buf = np.zeros(32 * 16 * 4, np.float32)
    assert L.drt_renderer_read_adaptive(h, 0, buf.ctypes.data, buf.nbytes) == drt.OK
    assert L.drt_renderer_read_adaptive(h, 1, buf.ctypes.data, buf.nbytes - 1) == drt.ERR_INVALID    # dst too short
    assert L.drt_renderer_read_adaptive(h, 2, buf.ctypes.data, buf.nbytes) == drt.ERR_INVALID
    assert L.drt_renderer_read_adaptive(h, 0, None, buf.nbytes) == drt.ERR_INVALID
    assert r.DeviceAdaptiveState(2) is None
    r.m_RendererSettings.RenderMode = drt.RendererSettings.DEBUGMODE
    assert _code(lambda: r.RenderAdaptive(cam, sc)) == drt.ERR_UNSUPPORTED
    r.m_RendererSettings.RenderMode = drt.RendererSettings.NORMALMODE
    r.RenderBatchAsync(cam, sc, 1)                                                             # a pending asynchronous batch
    assert _code(lambda: r.RenderAdaptive(cam, sc)) == drt.ERR_INVALID
    assert _code(r.resetAdaptive) == drt.ERR_INVALID
    r.Wait()
    assert r.RenderAdaptive(cam, sc).samples > 0
    s = drt.Renderer(0)                                                                        # a sharded renderer
    s.setShard(8, 0, 2)
    s.ResizeBuffer(32, 32)
    assert _code(lambda: s.RenderAdaptive(cam, sc)) == drt.ERR_UNSUPPORTED and s.DeviceAdaptiveState() is None
    broken = drt.Scene()                                                                       # a scene that cannot be rendered fails as rendering it would
    broken.setGeometry(np.float32([[0, 0, 0, 1, 0, 0, 0, 1, 0]]), np.zeros((1, 9), np.float32), np.zeros((1, 6), np.float32), [3])
    drt.BVHBuilder().buildIterative(broken)
    fresh = renderer({}, 32, 16)
    assert _code(lambda: fresh.RenderAdaptive(cam, broken)) == _code(lambda: fresh.Render(cam, broken))
    assert fresh.DeviceAdaptiveState() is None
    # (a tree deeper than 64 levels -> DRT_ERR_UNSUPPORTED through upload_scene: the builder makes no such tree, see test_gpu_ray_query.py)
