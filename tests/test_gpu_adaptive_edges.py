"""Adaptive sampling on the GPU where tests/test_gpu_adaptive.py does not go: the weights stage alone on made-up states (every
branch and rounding border of the weight rule, tests/adaptive_cases.py), degenerate frames, a budget below one sample per pixel,
pixel ranges of one pixel and ranges next to converged pixels, a frame above 2^20 pixels, and the temporal filter and the upscaler
as readers of the adaptive image.  Bit for bit throughout, as there."""
import numpy as np
import pytest

from tests import adaptive_cases as ac
from tests import adaptive_ref as ar
from tests.test_gpu_adaptive import CAP, _renderer_with_env, assert_bits, camera, renderer, scene, state_of, uniform_accumulations

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SETTINGS = dict(ray_bounce_limit=4)


# ---------------------------------------------------------------- 1. the weights stage alone

@pytest.mark.parametrize("luma_floor", ac.LUMA_FLOORS)
@pytest.mark.parametrize("size", [1, 63, 64, 65, 255, 256, 257, 3000])       # wave and workgroup borders of the reduction
def test_weights_of_made_up_states_equal_the_restatement(size, luma_floor):
    st = ac.states(size, luma_floor)
    for te in (0.0, ac.TARGET_ERROR):
        q, Q, active = drt.debug_adaptive_weights(st, target_error=te, luma_floor=luma_floor)
        ref = ar.weights(st, te, luma_floor)
        bad = np.flatnonzero(q != ref)
        assert bad.size == 0, "size %d, target_error %g, luma_floor %g: %d weights differ, first (n, m1, m2) = (%d, %r, %r): %d vs %d" % (
            size, te, luma_floor, bad.size, st.n[bad[0]], st.m1[bad[0]], st.m2[bad[0]], q[bad[0]], ref[bad[0]])
        assert Q == int(ref.sum(dtype=np.uint64)) and active == int((ref > 0).sum())


def test_the_weights_entry_reads_an_adaptive_state_as_well():
    """What GetAdaptiveState returns goes in as it is: the last call's q are the weights of the state before it."""
    sc, cam = scene("cornell_box"), camera("cornell_box")
    r = renderer(SETTINGS)
    r.RenderAdaptive(cam, sc, spp=3, max_spp=8)
    before = r.GetAdaptiveState()
    r.RenderAdaptive(cam, sc, spp=3, max_spp=8)
    q, Q, active = drt.debug_adaptive_weights(before)
    last_q = r.GetAdaptiveState().last_q.reshape(-1)
    assert (q == last_q).all() and Q == int(last_q.sum(dtype=np.uint64)) and active == int((last_q > 0).sum())


# ---------------------------------------------------------------- 2. the pipeline: degenerate frames, less than a sample per pixel

def assert_invariant(r, plain, cam, sc, what):
    """A pixel with n samples holds the uniform accumulation after n frames, and the framebuffer shows sum / n."""
    st, _, _ = state_of(r)
    accum_after = uniform_accumulations(plain, cam, sc, int(st.n.max()))
    assert_bits(st.sum, accum_after[st.n, np.arange(len(st.n))], what + ": sum vs accumulation after n frames")
    assert_bits(r.GetRenderTargetImage().reshape(-1, 4), ar.image(st), what + ": framebuffer vs sum / n")
    return st


@pytest.mark.parametrize("w,h", [(1, 1), (1, 70), (70, 1)])
def test_degenerate_frames(w, h):
    sc, cam = scene("cornell_box"), camera("cornell_box")
    r, plain = renderer(SETTINGS, w, h), renderer(SETTINGS, w, h)
    for call in range(2):
        before = state_of(r)[0] if call else ar.empty_state(w * h)
        info = r.RenderAdaptive(cam, sc, spp=3, max_spp=8)
        st = assert_invariant(r, plain, cam, sc, "%dx%d call %d" % (w, h, call))
        q, c = ar.plan(before, 3 * w * h, max_spp=8)
        _, got_q, got_c = state_of(r)
        assert (got_q == q).all() and (got_c == c).all() and (st.n == before.n + c).all()
        assert (info.samples, info.active_pixels, info.max_count) == (int(c.sum()), int((q > 0).sum()), int(c.max()))


def test_a_budget_below_one_sample_per_pixel_gives_no_pixel_a_sample():
    """drt.h "Counts": with min_spp == 0 and budget < pixels on a state where all weights are equal every floor is 0."""
    sc, cam = scene("cornell_box"), camera("cornell_box")
    W, H = 64, 48
    r, plain = renderer(SETTINGS), renderer(SETTINGS)
    info = r.RenderAdaptive(cam, sc, budget=W * H // 2, min_spp=0)
    assert (info.samples, info.max_count, info.active_pixels) == (0, 0, W * H)
    s = r.GetAdaptiveState()
    assert (s.count == 0).all() and (s.last_count == 0).all() and (s.last_q == CAP).all()
    assert not s.sum.any() and not s.m1.any() and not s.m2.any()
    image = r.GetRenderTargetImage().reshape(-1, 4)
    assert_bits(image, np.tile(np.float32([0, 0, 0, 1]), (W * H, 1)), "image of a call without samples")
    info = r.RenderAdaptive(cam, sc, spp=3, max_spp=8)            # the uniform first call, as on a fresh renderer
    st = assert_invariant(r, plain, cam, sc, "the call after it")
    assert (st.n == 3).all() and (info.samples, info.max_count, info.active_pixels) == (3 * W * H, 3, W * H)


# ---------------------------------------------------------------- 3. pixel ranges

def assert_twins(whole, split, a, b, what):
    assert (a.samples, a.active_pixels, a.max_count) == (b.samples, b.active_pixels, b.max_count), what
    for x, y in zip(whole.GetAdaptiveState(), split.GetAdaptiveState()):
        assert (x.view(np.uint32) == y.view(np.uint32)).all(), what
    assert_bits(split.GetRenderTargetImage(), whole.GetRenderTargetImage(), "image, " + what)


def test_a_pixel_with_more_samples_than_a_range_holds_is_a_range_of_its_own():
    sc, cam = scene("cornell_box"), camera("cornell_box")
    W, H, EACH = 8, 4, 30000
    params = dict(budget=W * H * EACH, min_spp=0, max_spp=40000)
    settings = dict(SETTINGS, max_samples=100000)               # (the frame loop stops at max_samples: the pin below needs 30 000 frames)
    whole, split = renderer(settings, W, H), _renderer_with_env({"DRT_SAMPLE_MB": "1"}, settings)
    split.ResizeBuffer(W, H)
    a, b = (r.RenderAdaptive(cam, sc, **params) for r in (whole, split))
    assert b.max_count > 21845, "a range of 1 MiB holds 21 845 samples: every pixel must exceed it"
    assert (split.GetAdaptiveState().last_count == EACH).all()
    assert_twins(whole, split, a, b, "call 0")
    plain = renderer(settings, W, H)                              # the independent pin: the frame loop's accumulation after 30 000 frames
    plain.RenderBatch(cam, sc, EACH)
    assert plain.getSampleCount() == EACH + 1
    assert_bits(split.GetAdaptiveState().sum, plain.GetAccumulationBuffer(), "sum vs RenderBatch(30000)")
    a, b = (r.RenderAdaptive(cam, sc, **params) for r in (whole, split))        # ragged: ranges of one pixel and of several
    assert_twins(whole, split, a, b, "call 1")
    c = split.GetAdaptiveState().last_count
    assert len(np.unique(c)) > 2 and c.max() > 21845


def test_pixel_ranges_next_to_converged_pixels_change_no_bit():
    sc, cam = scene("cornell_box"), camera("cornell_box")
    whole, split = renderer(SETTINGS), _renderer_with_env({"DRT_SAMPLE_MB": "1"}, SETTINGS)
    shown = 0
    for call in range(3):
        a, b = (r.RenderAdaptive(cam, sc, spp=24, max_spp=64, target_error=0.05) for r in (whole, split))
        assert_twins(whole, split, a, b, "call %d" % call)
        s = split.GetAdaptiveState()
        q, c = s.last_q.reshape(-1), s.last_count.reshape(-1)
        assert (c[q == 0] == 0).all() and (c[q > 0] >= 1).all()
        if 48 * b.samples > 3 << 20 and (q == 0).any() and (q > 0).any():
            shown += 1
    assert shown > 0, "no call that splits had converged and active pixels: the test would show nothing"


# ---------------------------------------------------------------- 4. above 2^20 pixels

def test_a_frame_above_two_to_the_twenty_pixels():
    sc, cam = scene("cornell_box"), camera("cornell_box")
    W, H = 1040, 1010                                           # 1 050 400 pixels > 1024 * 1024: the scan's second level carries
    r, plain = renderer(SETTINGS, W, H), renderer(SETTINGS, W, H)
    for call in range(2):
        info = r.RenderAdaptive(cam, sc, spp=2, max_spp=4)
        assert info.samples <= 2 * W * H
    st, _, c = state_of(r)
    assert st.n.max() <= 8 and info.samples == int(c.sum(dtype=np.uint64))
    assert len(np.unique(st.n)) > 2, "the second call must not be uniform: the test would show nothing"
    accum_after = uniform_accumulations(plain, cam, sc, int(st.n.max()))
    assert_bits(st.sum, accum_after[st.n, np.arange(W * H)], "sum vs accumulation after n frames")
    assert_bits(r.GetRenderTargetImage().reshape(-1, 4), ar.image(st), "framebuffer vs sum / n")


# ---------------------------------------------------------------- 5. the other readers of the adaptive image

def test_the_temporal_filter_and_the_upscaler_read_the_adaptive_image():
    """Both read the framebuffer and the first-hit guides, nothing of the frame loop's state (the sample count is not read): a fresh
    renderer whose bound framebuffer holds the adaptive image gives the same bits.  The temporal filter also reads its own history,
    which both renderers build from the same images."""
    sc, cam = scene("cornell_box"), camera("cornell_box")
    W, H = 64, 48
    r, other = renderer(SETTINGS), renderer(SETTINGS)
    dev = torch.device("cuda", 0)
    acc_t, rgba_t = torch.zeros((H, W, 3), device=dev), torch.zeros((H, W, 4), device=dev)
    other.bindBuffers(acc_t.data_ptr(), rgba_t.data_ptr())
    for call in range(2):                                       # the second call: ragged counts, and a history to reproject
        r.RenderAdaptive(cam, sc, spp=3, max_spp=8)
        img = r.GetRenderTargetImage()
        assert_bits(img.reshape(-1, 4), ar.image(state_of(r)[0]), "the framebuffer shows sum / n")
        rgba_t.copy_(torch.from_numpy(img).to(dev))
        torch.cuda.synchronize()
        assert_bits(r.TemporalDenoise(cam, sc), other.TemporalDenoise(cam, sc), "TemporalDenoise after adaptive call %d" % call)
        for x, y in zip(r.GetTemporalHistory(), other.GetTemporalHistory()):
            assert_bits(x, y, "temporal history after adaptive call %d" % call)
        assert_bits(r.Upscale(cam, sc, 2 * W, 2 * H, source=0), other.Upscale(cam, sc, 2 * W, 2 * H, source=0),
                    "Upscale after adaptive call %d" % call)
        assert_bits(r.GetRenderTargetImage(), img, "the filters leave the framebuffer as it is")
    assert len(np.unique(state_of(r)[0].n)) > 2
    other.bindBuffers(None, None)
