"""drt_renderer_temporal_denoise on the GPU (kernel_temporal.hip): stage (b) bit-equal to the restatement in tests/temporal_ref.py,
stage (c) equal to it within a measured gate, deterministic, free of side effects, worth running, and the error codes of
include/drt.h."""
import ctypes as C

import numpy as np
import pytest

from tests import ray_query_ref as rq
from tests import temporal_ref as tp
from tests.scenes import SCENES, scene_path

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

_cache = {}


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def scene(name):
    """(product scene, camera position, forward, bounce limit)"""
    if name not in _cache:
        if name == "two_quads":
            sc, _ = rq.programmatic_scene(drt, *tp.two_quads(), 2, 8)
            _cache[name] = (sc, (0.0, 0.1, 8.0), (0.0, 0.0, -1.0), 3)
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


def poses(pos, fwd, n, step=0.02, dolly=0.03):
    """n poses: an orbit about the vertical through the point 3 units ahead, `step` rad per pose, then (second half) a dolly
    along the view direction as well."""
    pos, fwd = np.float64(pos), np.float64(fwd) / np.linalg.norm(fwd)
    centre = pos + 3.0 * fwd
    out = []
    for k in range(n):
        a = step * k
        co, si = np.cos(a), np.sin(a)
        rot = lambda v: np.array([v[0] * co - v[2] * si, v[1], v[0] * si + v[2] * co])
        f = rot(fwd)
        p = centre + rot(pos - centre) + (dolly * max(0, k - n // 2)) * f
        out.append((tuple(np.float32(p)), tuple(np.float32(f))))
    return out


def renderer(W, H, depth):
    r = drt.Renderer(0)
    r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=depth)
    r.ResizeBuffer(W, H)
    return r


def run_sequence(r, sc, seq, check=None, **params):
    """One reset, 1-spp render and TemporalDenoise per pose; check(k, cam, img, out) after each; returns the outputs."""
    outs = []
    for k, (pos, fwd) in enumerate(seq):
        cam = camera(pos, fwd)
        r.resetAccumulationBuffer()
        r.Render(cam, sc)
        img = r.GetRenderTargetImage()
        out = r.TemporalDenoise(cam, sc, **params)
        if check:
            check(k, cam, img, out)
        outs.append(out)
    return outs


SCENE_NAMES = ["cornell_box", "uv_texture_test", "mc_transparency", "cs16_dust", "two_quads"]
SIZES = [(96, 64), (7, 3)]
FIELDS = ("color", "length", "m1", "m2", "variance", "weight")


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_reprojection_is_bit_equal_to_the_restatement(name, W, H):
    """Colour, N, moments, variance and weight sum as uint32, every pixel, after each of 6 poses (orbit + dolly, 1 spp each), for
    alpha_min in {0, 0.2} x max_history in {4, 32}."""
    sc, pos, fwd, depth = scene(name)
    seq = poses(pos, fwd, 6)
    for alpha_min, max_history in ((0.0, 32), (0.2, 4), (0.0, 4), (0.2, 32)):
        r = renderer(W, H, depth)
        state = {"hist": None, "reused": 0}

        def check(k, cam, img, out):
            g = r.renderGuides(cam, sc, 1)
            ref = tp.reproject(state["hist"], img, g, tp.pinhole_of(cam, W, H), max_history=max_history, alpha_min=alpha_min)
            h = r.GetTemporalHistory()
            got = dict(color=h.color, length=h.length, m1=h.moments[..., 0], m2=h.moments[..., 1], variance=h.variance, weight=h.weight)
            for f in FIELDS:
                bad = u32(got[f]) != u32(getattr(ref, f))
                assert not bad.any(), "%s %dx%d pose %d alpha_min %g max_history %d: %s differs on %d pixels (first %s: %r vs %r)" % (
                    name, W, H, k, alpha_min, max_history, f, bad.sum(), np.argwhere(bad)[0], got[f][bad][0], getattr(ref, f)[bad][0])
            state["hist"] = ref
            state["reused"] += int((ref.length > 1).sum())
        run_sequence(r, sc, seq, check, iterations=0, alpha_min=alpha_min, max_history=max_history)
        if W * H > 100:
            assert state["reused"] > W * H, "the sequence reuses history"
            assert state["hist"].length.max() == min(6, max_history)


SIGMAS = [dict(sigma_luma=4.0, sigma_normal=0.1, sigma_albedo=0.1), dict(sigma_luma=1.5, sigma_normal=0.35, sigma_albedo=0.05)]
# Largest |TemporalDenoise - atrous_var()| measured on the MI355X over every case below: FILTER_MEASURED.  The
# gate is 10 times that, and never looser than 1e-3 (a quarter of an 8-bit step of the display-referred values).
FILTER_MEASURED = 1.431e-6
FILTER_GATE = 10 * FILTER_MEASURED
_max_diff = []


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_filter_matches_the_restatement(name, W, H):
    """Stage (c) on the GPU's own stage (b) (bit-equal to the restatement's, above): 1, 5 and 7 passes, two sigma sets, after
    every pose of the sequence (spatial variance everywhere at first, then a history of mixed lengths and variances)."""
    sc, pos, fwd, depth = scene(name)
    seq = poses(pos, fwd, 6)
    worst = [0.0]
    for K in (1, 5, 7):
        for sig in SIGMAS:
            r = renderer(W, H, depth)

            def check(k, cam, img, out):
                g, h = r.renderGuides(cam, sc, 1), r.GetTemporalHistory()
                ref = tp.atrous_var(h.color, h.variance, g.albedo, g.normal, iterations=K, **sig)
                diff = float(np.abs(out - ref).max())
                print("%s %dx%d pose %d K %d sigma_luma %g: max |GPU - restatement| = %.3e" % (name, W, H, k, K, sig["sigma_luma"], diff))
                worst[0] = max(worst[0], diff)
                assert (out[..., 3] == 1).all() and np.isfinite(out).all()
            run_sequence(r, sc, seq, check, iterations=K, **sig)
    worst = worst[0]
    _max_diff.append(worst)
    print("%s %dx%d: max %.3e (largest so far %.3e, gate %.1e)" % (name, W, H, worst, max(_max_diff), FILTER_GATE))
    assert worst <= FILTER_GATE, (name, W, H, worst)


def test_zero_passes_give_the_integrated_colour():
    sc, pos, fwd, depth = scene("cornell_box")
    r = renderer(64, 40, depth)
    outs = run_sequence(r, sc, poses(pos, fwd, 3), iterations=0)
    h = r.GetTemporalHistory()
    assert (u32(outs[-1][..., :3]) == u32(h.color)).all() and (outs[-1][..., 3] == 1).all()
    assert (h.length > 1).any()


def test_temporal_denoise_is_deterministic():
    sc, pos, fwd, depth = scene("mc_transparency")
    seq = poses(pos, fwd, 5)
    r = renderer(120, 72, depth)
    a = run_sequence(r, sc, seq)
    ha = r.GetTemporalHistory()
    assert r.m_LastTemporalMs > 0
    r.resetTemporalHistory()
    assert r.DeviceTemporalHistory(0) is None
    b = run_sequence(r, sc, seq)
    hb = r.GetTemporalHistory()
    c = run_sequence(renderer(120, 72, depth), sc, seq)
    for x, y, z in zip(a, b, c):
        assert (u32(x) == u32(y)).all() and (u32(x) == u32(z)).all()
    for x, y in zip(ha, hb):
        assert (u32(x) == u32(y)).all()
    assert (ha.length > 1).any()
    assert (u32(r.GetDenoisedImage()) == u32(b[-1])).all() and r.DeviceDenoisedTarget()


def test_temporal_denoise_leaves_the_renderer_alone():
    sc, pos, fwd, _ = scene("cornell_box")
    cam = camera(pos, fwd)
    images = []
    for with_temporal in (False, True):
        r = renderer(96, 64, 8)
        r.setCounting(True)
        r.RenderBatch(cam, sc, 2)
        before_denoise = r.Denoise(cam, sc)

        def snapshot():
            return (r.GetAccumulationBuffer(), r.GetRenderTargetImage(), r.getSampleCount(), r.kernelInfo(), r.getCounters().as_dict(),
                    r.kernelSpanMs())
        state = snapshot()
        if with_temporal:
            r.TemporalDenoise(cam, sc)
            r.TemporalDenoise(cam, sc, iterations=0)
            r.resetTemporalHistory()
            r.TemporalDenoise(cam, sc, iterations=2)
            after = snapshot()
            assert (u32(after[0]) == u32(state[0])).all() and (u32(after[1]) == u32(state[1])).all()
            assert after[2:] == state[2:]
            assert (u32(r.Denoise(cam, sc)) == u32(before_denoise)).all()       # Denoise gives what it gave before
        r.RenderBatch(cam, sc, 2)
        images.append((r.GetRenderTargetImage(), r.getSampleCount()))
    assert (u32(images[0][0]) == u32(images[1][0])).all() and images[0][1] == images[1][1]


def test_resize_drops_the_history():
    sc, pos, fwd, depth = scene("cornell_box")
    r = renderer(64, 40, depth)
    run_sequence(r, sc, poses(pos, fwd, 3))
    assert (r.GetTemporalHistory().length > 1).any() and r.DeviceTemporalHistory(0) and r.DeviceTemporalHistory(1)
    r.ResizeBuffer(72, 40)                                  # (a resize to the size it has is a no-op, as in the reference)
    assert r.DeviceTemporalHistory(0) is None
    with pytest.raises(drt.DrtError):
        r.GetTemporalHistory()
    run_sequence(r, sc, poses(pos, fwd, 1))
    h = r.GetTemporalHistory()
    assert (h.length == 1).all() and (h.weight == 0).all()


def test_temporal_beats_the_single_frame_filter():
    """cornell_box 192x128, a 12-pose orbit of small steps at 1 spp per pose, against the renderer's own 256-frame render of the
    last pose: RMSE(temporal) / RMSE(raw 1 spp) < 1 and RMSE(temporal) / RMSE(Denoise of that 1-spp frame, defaults) < 1.
    Measured on the MI355X: 0.170 and 0.181."""
    sc, pos, fwd, depth = scene("cornell_box")
    W, H = 192, 128
    seq = poses(pos, fwd, 12, step=0.004, dolly=0.0)
    r = renderer(W, H, depth)
    r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=depth, max_samples=1000)
    out = run_sequence(r, sc, seq)[-1]
    cam = camera(*seq[-1])
    raw = r.GetRenderTargetImage()
    assert r.getSampleCount() == 2                          # (one frame rendered: the next frame index)
    single = r.Denoise(cam, sc)
    r.resetAccumulationBuffer()
    r.RenderBatch(cam, sc, 256)
    truth = r.GetRenderTargetImage()
    e_t, e_raw, e_single = tp.rmse(out, truth), tp.rmse(raw, truth), tp.rmse(single, truth)
    print("cornell_box %dx%d, 12 poses: RMSE temporal %.5f, raw 1 spp %.5f, Denoise(1 spp) %.5f; ratios %.3f and %.3f"
          % (W, H, e_t, e_raw, e_single, e_t / e_raw, e_t / e_single))
    assert e_t / e_raw < 1
    assert e_t / e_single < 1


def _code(fn):
    with pytest.raises(drt.DrtError) as e:
        fn()
    return e.value.code


def test_error_codes():
    sc, pos, fwd, _ = scene("cornell_box")
    cam = camera(pos, fwd)
    L = drt._lib
    r = drt.Renderer(0)
    pod, p, ms = cam._pod(), drt.TemporalParams(), C.c_float(0)
    assert _code(lambda: r.TemporalDenoise(cam, sc)) == drt.ERR_INVALID                       # no frame size
    r.ResizeBuffer(32, 16)
    assert _code(lambda: r.GetTemporalHistory()) == drt.ERR_INVALID and r.DeviceTemporalHistory(0) is None      # before the first call
    h = r._h
    for args in ((None, C.byref(pod), sc._h, C.byref(p), C.byref(ms)), (h, None, sc._h, C.byref(p), C.byref(ms)),
                 (h, C.byref(pod), None, C.byref(p), C.byref(ms)), (h, C.byref(pod), sc._h, None, C.byref(ms))):
        assert L.drt_renderer_temporal_denoise(*args) == drt.ERR_INVALID
    for bad in (dict(iterations=-1), dict(iterations=11), dict(max_history=0), dict(alpha_min=-0.1), dict(alpha_min=1.5),
                dict(alpha_min=float("nan")), dict(normal_cos_min=float("inf")), dict(sigma_luma=0.0), dict(sigma_normal=-1.0),
                dict(sigma_albedo=float("nan")), dict(sigma_luma=float("inf"))):
        assert _code(lambda: r.TemporalDenoise(cam, sc, **bad)) == drt.ERR_INVALID, bad
    r.TemporalDenoise(cam, sc, iterations=10, max_history=1, alpha_min=1.0)                  # the bounds themselves are accepted
    r.TemporalDenoise(cam, sc, iterations=0, alpha_min=0.0)
    buf = np.zeros(32 * 16 * 4, np.float32)
    assert L.drt_renderer_read_temporal(h, 0, buf.ctypes.data, buf.size) == drt.OK
    assert L.drt_renderer_read_temporal(h, 2, buf.ctypes.data, buf.size) == drt.ERR_INVALID  # which outside 0..1
    assert L.drt_renderer_read_temporal(h, -1, buf.ctypes.data, buf.size) == drt.ERR_INVALID
    assert L.drt_renderer_read_temporal(h, 1, buf.ctypes.data, buf.size - 1) == drt.ERR_INVALID      # dst too short
    assert L.drt_renderer_read_temporal(h, 1, None, buf.size) == drt.ERR_INVALID
    assert L.drt_renderer_device_temporal(h, 2) is None
    r.RenderBatchAsync(cam, sc, 1)                                                           # a pending asynchronous batch
    assert _code(lambda: r.TemporalDenoise(cam, sc)) == drt.ERR_INVALID
    assert _code(lambda: r.resetTemporalHistory()) == drt.ERR_INVALID
    r.Wait()
    r.TemporalDenoise(cam, sc)
    s = drt.Renderer(0)                                                                      # a sharded renderer
    s.setShard(8, 0, 2)
    s.ResizeBuffer(32, 32)
    assert _code(lambda: s.TemporalDenoise(cam, sc)) == drt.ERR_UNSUPPORTED
    # (a tree deeper than 64 levels -> DRT_ERR_UNSUPPORTED through the guide pass: the builder makes no such tree, see test_gpu_ray_query.py)
