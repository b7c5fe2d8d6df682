"""Motion tracking on the GPU (kernel_motion.hip): with drt_renderer_track_motion on, stage (b) of the temporal filter is bit-equal
to tests/motion_ref.py over sequences with device refits between the calls, drt_renderer_motion_vectors equals its restatement,
the snapshot's life cycle is the header's, tracking off is the parent's result, and nothing else of the renderer is touched."""
import ctypes as C

import numpy as np
import pytest

from tests import motion_ref as mo
from tests import ray_query_ref as rq
from tests import refit_ref as rf
from tests import temporal_ref as tp
from tests.scenes import SCENES, scene_path
from tests.test_gpu_temporal import FILTER_GATE, camera, poses, renderer, u32

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
_cache = {}


def scene(name):
    """(product scene, load-order positions, load indices of the triangles that move, camera position, forward, bounce limit)"""
    if name not in _cache:
        if name == "two_quads":
            s = tp.two_quads()
            sc, _ = rq.programmatic_scene(drt, *s, 2, 8)
            _cache[name] = (sc, s[0].copy(), np.array([2, 3]), (0.0, 0.1, 8.0), (0.0, 0.0, -1.0), 3)
        else:
            sc = drt.Scene()
            sc.loadGLTFmodel(scene_path(name))
            pos0 = rf.streams(sc.m_PrimitivesBuffer)[0].copy()
            b = drt.BVHBuilder()
            b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
            b.buildIterative(sc)
            if name == "cornell_box":                      # one of the two boxes: its drt_mesh range
                m = sc.m_Meshes[1]
                sel = np.arange(int(m["primitives_offset"]), int(m["primitives_offset"]) + int(m["tris_count"]))
            elif name == "uv_texture_test":
                sel = np.array([6, 7])                      # the textured quad nearest the camera
            else:                                           # a few per cent of the triangles, the ones nearest the camera's axis
                _, pos, fwd, _ = SCENES[name]
                c = pos0.mean(axis=1) - F(pos)
                f = F(fwd) / np.linalg.norm(fwd)
                along = c @ f
                off = np.linalg.norm(c - along[:, None] * f, axis=1)
                sel = np.argsort(np.where(along > 0, off / np.maximum(along, 1e-3), np.inf))[:max(1, len(pos0) // 20)]
            _, pos, fwd, depth = SCENES[name]
            _cache[name] = (sc, pos0, sel, pos, fwd, depth)
    return _cache[name]


def mover(kind, pos0, sel, scale):
    """k -> load-order positions of pose k: the selected triangles translated, turned about a vertical through their centre, or
    bent by a travelling sine."""
    centre = pos0[sel].reshape(-1, 3).mean(axis=0)

    def at(k):
        p = pos0.copy()
        if kind == "translate":
            p[sel] += F([0.05, 0.02, 0.0]) * F(scale * k)
        elif kind == "rotate":
            p[sel] = mo.rotate_about(pos0[sel], centre, (0, 1, 0), 0.1 * k)
        else:
            q = pos0[sel]
            p[sel] = q + (F(0.05 * scale) * np.sin(3.0 * q[..., 0:1] + 0.7 * k) * F([0, 1, 1])).astype(F)
        return p
    return at


def got_history(r):
    h = r.GetTemporalHistory()
    return dict(color=h.color, length=h.length, m1=h.moments[..., 0], m2=h.moments[..., 1], variance=h.variance, weight=h.weight)


def assert_history(got, ref, what, where=None, fields=mo.FIELDS):
    for f in fields:
        bad = u32(got[f]) != u32(getattr(ref, f))
        if bad.ndim == 3:
            bad = bad.any(axis=-1)
        if where is not None:
            bad &= where
        assert not bad.any(), "%s: %s differs on %d pixels (first %s: %r vs %r)" % (
            what, f, bad.sum(), np.argwhere(bad)[0], got[f][bad][0], getattr(ref, f)[bad][0])


def dev(p):
    return torch.from_numpy(np.ascontiguousarray(p, F)).to(DEV)


SIZES = [(96, 64), (7, 3)]


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("cam_moves", [False, True])
@pytest.mark.parametrize("kind", ["translate", "rotate", "deform"])
@pytest.mark.parametrize("name", ["two_quads", "cornell_box", "cs16_dust"])
def test_reprojection_follows_refitted_geometry(name, kind, cam_moves, W, H):
    """Seven calls with device refits between them, for alpha_min in {0, 0.2} x max_history in {4, 32}: colour, N, moments, variance
    and weight sum as uint32 on every pixel against reproject_motion with the device's own TriHot records of this call and the
    previous one.  Call 2 follows TWO refits (the snapshot keeps the oldest state), call 3 follows none (static), call 4 follows a
    refit away and one back (nothing moved), the others one refit each.  motionVectors (asked before the call, previous camera
    NULL = the last call's) equals its restatement bit for bit.  Pixels whose triangle did not move equal the static restatement."""
    sc, pos0, sel, pos, fwd, depth = scene(name)
    at = mover(kind, pos0, sel, 4.0 if name == "cs16_dust" else 1.0)
    n = 7
    seq = poses(pos, fwd, n) if cam_moves else [(pos, fwd)] * n
    for alpha_min, max_history in ((0.0, 32), (0.2, 4), (0.0, 4), (0.2, 32)):
        r = renderer(W, H, depth)
        r.trackMotion()
        hist = static_hist = hot_prev = ph_prev = None
        moved_px = reused = 0
        for k, (cp, cf) in enumerate(seq):
            cam = camera(cp, cf)
            if k == 2:
                r.refit(sc, dev(at(1.5)))
                r.refit(sc, dev(at(k)))
            elif k == 4:
                r.refit(sc, dev(at(9)))
                r.refit(sc, dev(at(2)))                     # call 3 saw the positions of call 2
            elif k != 3:
                r.refit(sc, dev(at(k)))
            hot = r.debugReadDeviceScene(sc)[1].copy()
            ph = tp.pinhole_of(cam, W, H)
            r.resetAccumulationBuffer()
            r.Render(cam, sc)
            img = r.GetRenderTargetImage()
            g = r.renderGuides(cam, sc, 1)
            what = "%s %s cam_moves %d %dx%d call %d alpha_min %g max_history %d" % (name, kind, cam_moves, W, H, k, alpha_min, max_history)
            if k > 0:
                mv = r.motionVectors(cam, sc)
                mv_ref = mo.motion_vectors(g, ph, ph_prev, hot, hot_prev)
                bad = (u32(mv) != u32(mv_ref)).any(axis=-1)
                assert not bad.any(), "%s: motion vectors differ on %d pixels (first %s: %r vs %r)" % (
                    what, bad.sum(), np.argwhere(bad)[0], mv[bad][0], mv_ref[bad][0])
                if k in (3, 4):
                    assert (mv[..., 3] <= 1).all(), what
            r.TemporalDenoise(cam, sc, iterations=0, alpha_min=alpha_min, max_history=max_history)
            ref = mo.reproject_motion(hist, img, g, ph, hot, hot_prev, max_history=max_history, alpha_min=alpha_min)
            got = got_history(r)
            assert_history(got, ref, what)
            _, _, rule = mo.previous_points(g, ph, hot, hot_prev)
            static = tp.reproject(hist, img, g, ph, max_history=max_history, alpha_min=alpha_min)
            assert_history(got, static, what + " (unmoved pixels)", where=rule != mo.MOVED, fields=("color", "length", "m1", "m2", "weight"))
            assert_history(got, static, what + " (unmoved pixels, temporal variance)", where=(rule != mo.MOVED) & (static.length >= 4),
                           fields=("variance",))
            moved_px += int((rule == mo.MOVED).sum())
            reused += int(((rule == mo.MOVED) & (ref.length > 1)).sum())
            hist, hot_prev, ph_prev = ref, hot, ph
        if W * H > 100:
            assert moved_px > 50, "the sequence moves visible triangles"
            assert reused > 20, "moved pixels keep a history"


def _one_move(name="cornell_box", W=96, H=64, track=True, k_move=1.0):
    """A renderer after one call at the scene's pose and a device refit: (r, sc, cam, hist, hot0, hot1, ph)."""
    sc, pos0, sel, pos, fwd, depth = scene(name)
    r = renderer(W, H, depth)
    if track:
        r.trackMotion()
    cam = camera(pos, fwd)
    ph = tp.pinhole_of(cam, W, H)
    r.refit(sc, dev(pos0))                                  # (arms a snapshot equal to the current records: static)
    hot0 = r.debugReadDeviceScene(sc)[1].copy()
    r.Render(cam, sc)
    hist = tp.reproject(None, r.GetRenderTargetImage(), r.renderGuides(cam, sc, 1), ph)
    r.TemporalDenoise(cam, sc, iterations=0)
    assert_history(got_history(r), hist, "first call")
    r.refit(sc, dev(mover("translate", pos0, sel, 1.0)(k_move * 3)))
    hot1 = r.debugReadDeviceScene(sc)[1].copy()
    return r, sc, cam, hist, hot0, hot1, ph


def _next_call(r, sc, cam, **params):
    r.resetAccumulationBuffer()
    r.Render(cam, sc)
    img, g = r.GetRenderTargetImage(), r.renderGuides(cam, sc, 1)
    out = r.TemporalDenoise(cam, sc, **params)
    return img, g, out


def test_tracking_off_and_no_refit_are_the_static_result():
    r, sc, cam, hist, hot0, hot1, ph = _one_move(track=False)
    assert (r.motionVectors(cam, sc)[..., 3] <= 1).all()    # works with tracking off: no moved flag
    img, g, _ = _next_call(r, sc, cam, iterations=0)
    assert mo.moved_triangles(hot1, hot0).any()
    assert_history(got_history(r), tp.reproject(hist, img, g, ph), "tracking off after a refit")
    r = renderer(96, 64, 8)
    r.trackMotion()
    sc, _, _, pos, fwd, _ = scene("cornell_box")
    h = None
    for cp, cf in poses(pos, fwd, 3):
        cam = camera(cp, cf)
        img, g, _ = _next_call(r, sc, cam, iterations=0)
        h = tp.reproject(h, img, g, tp.pinhole_of(cam, 96, 64))
        assert_history(got_history(r), h, "tracking on, no refit")


def test_snapshot_life_cycle():
    """advanceMotion disarms; trackMotion(False) frees; a host refit's re-upload drops the snapshot; a temporal reset, a resize and
    a destroy with an armed snapshot are clean."""
    for how in ("advance", "off", "host_refit"):
        r, sc, cam, hist, hot0, hot1, ph = _one_move()
        assert (r.motionVectors(cam, sc)[..., 3] == 2).any()
        host_pos = None
        if how == "advance":
            r.advanceMotion()
        elif how == "off":
            r.trackMotion(False)
        else:
            _, pos0, sel, *_ = scene("cornell_box")
            host_pos = mover("translate", pos0, sel, 1.0)(2)
            sc.refit(host_pos)
        try:
            assert (r.motionVectors(cam, sc)[..., 3] <= 1).all(), how
            img, g, _ = _next_call(r, sc, cam, iterations=0)
            assert_history(got_history(r), tp.reproject(hist, img, g, ph), how)
        finally:
            if host_pos is not None:
                sc.refit(scene("cornell_box")[1])           # (the scene is shared by the tests of this file)
    r, sc, cam, hist, hot0, hot1, ph = _one_move()
    r.resetTemporalHistory()
    with pytest.raises(drt.DrtError):
        r.motionVectors(cam, sc)                            # no previous camera any more
    img, g, _ = _next_call(r, sc, cam, iterations=0)
    h = got_history(r)
    assert (h["length"] == 1).all() and (h["weight"] == 0).all()
    r, sc, cam, *_ = _one_move()                            # a failed refit drops the snapshot with the half-written copy
    bad = scene("cornell_box")[1].copy()
    bad[0, 0, 0] = np.nan
    assert _code(lambda: r.refit(sc, dev(bad))) == drt.ERR_INVALID
    r.advanceMotion()
    assert (r.motionVectors(cam, sc, prev_cam=cam)[..., 3] <= 1).all()
    _next_call(r, sc, cam)
    r, sc, cam, *_ = _one_move()
    r.ResizeBuffer(72, 40)
    assert (r.motionVectors(cam, sc, prev_cam=cam)[..., 3] == 2).any() and r.motionVectors(cam, sc, prev_cam=cam).shape == (40, 72, 4)
    _next_call(r, sc, cam)
    r, *_ = _one_move()
    del r


def test_motion_vectors_numpy_and_torch_agree():
    r, sc, cam, hist, hot0, hot1, ph = _one_move()
    a = r.motionVectors(cam, sc)
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        b = r.motionVectors(cam, sc, as_torch=True)
        c = r.motionVectors(cam, sc, prev_cam=cam, as_torch=True)
    s.synchronize()
    assert (u32(a) == u32(b.cpu().numpy())).all() and (u32(a) == u32(c.cpu().numpy())).all()
    g = r.renderGuides(cam, sc, 1)
    assert (u32(a) == u32(mo.motion_vectors(g, ph, ph, hot1, hot0))).all()
    flags = a[..., 3]
    assert ((flags == 0) == (g.prim < 0)).all() and (flags == 2).any() and (flags == 1).any()
    assert (a[flags == 0] == 0).all()


def test_filter_on_a_motion_sequence_keeps_the_parents_gate():
    """Stage (c) is the parent's code: |TemporalDenoise - atrous_var()| within test_gpu_temporal.py's gate on a moving sequence."""
    sc, pos0, sel, pos, fwd, depth = scene("cornell_box")
    at = mover("translate", pos0, sel, 1.0)
    r = renderer(96, 64, depth)
    r.trackMotion()
    worst = 0.0
    for k, (cp, cf) in enumerate(poses(pos, fwd, 6)):
        cam = camera(cp, cf)
        r.refit(sc, dev(at(k)))
        img, g, out = _next_call(r, sc, cam, iterations=5)
        h = r.GetTemporalHistory()
        ref = tp.atrous_var(h.color, h.variance, g.albedo, g.normal, iterations=5)
        worst = max(worst, float(np.abs(out - ref).max()))
        assert (out[..., 3] == 1).all() and np.isfinite(out).all()
    print("max |GPU - restatement| = %.3e (gate %.3e)" % (worst, FILTER_GATE))
    assert worst <= FILTER_GATE


def _run(name, kind, n, track, reset_each=False, W=96, H=64, r=None, truth_frames=0):
    sc, pos0, sel, pos, fwd, depth = scene(name)
    at = mover(kind, pos0, sel, 1.0)
    r = r or renderer(W, H, depth)
    r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=depth, max_samples=100000)
    r.trackMotion(track)
    cam = camera(pos, fwd)
    outs = []
    for k in range(n):
        r.refit(sc, dev(at(k)))
        if reset_each:
            r.resetTemporalHistory()
        _next_call(r, sc, cam, iterations=0)
        outs.append(got_history(r))
    truth = None
    if truth_frames:
        r.resetAccumulationBuffer()
        r.RenderBatch(cam, sc, truth_frames)
        truth = r.GetRenderTargetImage()
        g = r.renderGuides(cam, sc, 1)
        order = sc.triangleOrder()
        truth = (truth, np.isin(g.prim, np.nonzero(np.isin(order, sel))[0]))
    return outs, truth


def test_determinism():
    a, _ = _run("cornell_box", "rotate", 5, True)
    b, _ = _run("cornell_box", "rotate", 5, True)
    for x, y in zip(a, b):
        for f in mo.FIELDS:
            assert (u32(x[f]) == u32(y[f])).all(), f
    assert (a[-1]["length"] > 1).any()


def test_a_moving_object_converges_on_the_gpu():
    """The check of test_motion_ref.py on the GPU's own 1-spp frames: the textured quad of uv_texture_test moving across 10 poses
    under a still camera, against the renderer's 256-frame render of the last pose, over the moved triangles' pixels: RMSE with
    tracking on < RMSE with tracking off, and < RMSE with a history reset at every move."""
    moved, (truth, sel) = _run("uv_texture_test", "translate", 10, True, truth_frames=256)
    static, _ = _run("uv_texture_test", "translate", 10, False)
    reset, _ = _run("uv_texture_test", "translate", 10, True, reset_each=True)
    assert sel.sum() > 200
    e = [tp.rmse(h[-1]["color"][sel], truth[..., :3][sel]) for h in (moved, static, reset)]
    print("RMSE over the moved triangles' pixels: tracking on %.5f, tracking off %.5f, reset at every move %.5f" % tuple(e))
    assert e[0] < e[1]
    assert e[0] < e[2]


def test_the_new_calls_leave_the_renderer_alone():
    sc, pos0, sel, pos, fwd, _ = scene("cornell_box")
    cam = camera(pos, fwd)
    r = renderer(96, 64, 8)
    r.setCounting(True)
    r.RenderBatch(cam, sc, 2)
    r.TemporalDenoise(cam, sc)

    def snapshot():
        return (r.GetAccumulationBuffer(), r.GetRenderTargetImage(), r.getSampleCount(), r.kernelInfo(), r.getCounters().as_dict(),
                r.kernelSpanMs(), r.GetDenoisedImage(), r.GetTemporalHistory())
    state = snapshot()
    r.trackMotion()
    r.motionVectors(cam, sc)
    r.advanceMotion()
    r.motionVectors(cam, sc, prev_cam=cam, as_torch=True)
    r.trackMotion(False)
    after = snapshot()
    for i in (0, 1, 6):
        assert (u32(after[i]) == u32(state[i])).all()
    assert after[2:6] == state[2:6]
    for x, y in zip(after[7], state[7]):
        assert (u32(x) == u32(y)).all()


def _code(fn):
    with pytest.raises(drt.DrtError) as e:
        fn()
    return e.value.code


def test_error_codes():
    sc, _, _, pos, fwd, _ = scene("cornell_box")
    cam = camera(pos, fwd)
    L = drt._lib
    r = drt.Renderer(0)
    pod = cam._pod()
    assert _code(lambda: r.motionVectors(cam, sc, prev_cam=cam)) == drt.ERR_INVALID          # no frame size
    r.ResizeBuffer(32, 16)
    assert _code(lambda: r.motionVectors(cam, sc)) == drt.ERR_INVALID                       # no temporal call yet, prev_cam NULL
    out = torch.empty((16 * 32 * 4 + 4,), dtype=torch.float32, device=DEV)
    h, p = r._h, C.byref(pod)
    assert L.drt_renderer_motion_vectors(h, p, p, sc._h, out.data_ptr(), None) == drt.OK
    for args in ((None, p, p, sc._h, out.data_ptr(), None), (h, None, p, sc._h, out.data_ptr(), None), (h, p, p, None, out.data_ptr(), None),
                 (h, p, p, sc._h, None, None)):
        assert L.drt_renderer_motion_vectors(*args) == drt.ERR_INVALID
    assert L.drt_renderer_motion_vectors(h, p, p, sc._h, out.data_ptr() + 4, None) == drt.ERR_INVALID      # misaligned
    host = np.zeros(16 * 32 * 4 + 4, np.float32)
    assert L.drt_renderer_motion_vectors(h, p, p, sc._h, (host.ctypes.data + 15) & ~15, None) == drt.ERR_INVALID   # host memory
    r.RenderBatchAsync(cam, sc, 1)                                                           # a pending asynchronous batch
    assert _code(lambda: r.motionVectors(cam, sc, prev_cam=cam)) == drt.ERR_INVALID
    r.Wait()
    r.TemporalDenoise(cam, sc)
    assert r.motionVectors(cam, sc).shape == (16, 32, 4)
    s = drt.Renderer(0)                                                                      # a sharded renderer
    s.setShard(8, 0, 2)
    s.ResizeBuffer(32, 32)
    s.trackMotion()
    s.advanceMotion()
    s.trackMotion(False)
    assert _code(lambda: s.motionVectors(cam, sc, prev_cam=cam)) == drt.ERR_UNSUPPORTED
    assert _code(lambda: s.TemporalDenoise(cam, sc)) == drt.ERR_UNSUPPORTED
    # (a tree deeper than 64 levels -> DRT_ERR_UNSUPPORTED, checked before anything is allocated: the builder makes no such tree, see
    # test_gpu_ray_query.py)
