"""guide_kernel, temporal_reproject_kernel + temporal_variance_kernel and motion_reproject_kernel + motion_vectors_kernel at the
frame sizes people run (1920x1080, 3840x2160 where no CPU restatement is needed) and at 1283x721 (odd, prime width: the last 8x8
tile of a row holds 3 columns).  The assertions are those of test_gpu_denoise.py, test_gpu_temporal.py and test_gpu_motion.py at
96x64 -- uint32 equality on every pixel -- at sizes where the fp32 chain pixel -> ray -> world -> previous pixel rounds as it does
at x near 1919 or 3839, not as at x <= 95."""
import concurrent.futures

import numpy as np
import pytest

import oracle
from tests import denoise_ref as dn
from tests import motion_ref as mo
from tests import ray_query_ref as rq
from tests import temporal_ref as tp
from tests import test_gpu_denoise as gd
from tests import test_gpu_motion as gm
from tests import test_gpu_temporal as gt

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

u32 = gt.u32


def _parallel(jobs):
    """{key: thunk} -> {key: result}, one thread each (numpy releases the GIL in its loops)."""
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(jobs)) as ex:
        futures = {k: ex.submit(f) for k, f in jobs.items()}
        return {k: f.result() for k, f in futures.items()}


@pytest.mark.parametrize("W,H", [(1920, 1080), (1283, 721), (3840, 2160)])
@pytest.mark.parametrize("frame", [1, 3])
@pytest.mark.parametrize("name", ["cornell_box", "cs16_dust"])
def test_guides_bit_equal_to_debug_views_and_ray_queries_at_full_size(name, frame, W, H):
    """The body of test_gpu_denoise.py::test_guides_bit_equal_to_debug_views_and_ray_queries: albedo and normal against the ALBEDO /
    NORMAL debug views of frame `frame` alone, t and prim against traceRays on the same camera rays."""
    sc, pos, fwd = gd.scene(name)
    cam = gd.camera(pos, fwd)
    r = drt.Renderer(0)
    r.ResizeBuffer(W, H)
    g = r.renderGuides(cam, sc, frame)
    assert g.albedo.shape == (H, W, 3) and g.normal.shape == (H, W, 3) and g.t.shape == (H, W) and g.prim.dtype == np.int32
    albedo = gd.one_frame_sum(sc, cam, W, H, frame, RenderMode=1, DebugMode=0, tone_mapping=0, gamma_correction=0)
    normal = gd.one_frame_sum(sc, cam, W, H, frame, RenderMode=1, DebugMode=1)
    bad = (u32(g.albedo) != u32(albedo)).any(axis=-1)
    assert not bad.any(), "%s frame %d: albedo differs on %d pixels (first %s)" % (name, frame, bad.sum(), np.argwhere(bad)[0])
    hit = g.prim >= 0
    bad = (u32(g.normal) != u32(normal)).any(axis=-1) & hit
    assert not bad.any(), "%s frame %d: normal differs on %d hit pixels (first %s)" % (name, frame, bad.sum(), np.argwhere(bad)[0])
    assert (u32(g.normal)[~hit] == 0).all()
    org, dirs = dn.camera_rays(oracle.default_camera(position=pos, forward=fwd), W, H, frame)
    hits = r.traceRays(sc, org, dirs)
    assert (g.prim.ravel() == hits.prim).all(), "%s frame %d: prim differs on %d pixels" % (name, frame, (g.prim.ravel() != hits.prim).sum())
    assert (u32(g.t).ravel() == u32(hits.t)).all()
    assert (u32(g.t)[~hit] == u32(np.float32(rq.FLT_MAX))).all()
    assert hit.any() and (name == "cs16_dust" or (~hit).any())


SIZES = [(1920, 1080), (1283, 721)]


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", ["cornell_box", "two_quads"])
def test_reprojection_is_bit_equal_to_the_restatement_at_full_size(name, W, H):
    """test_gpu_temporal.py::test_reprojection_is_bit_equal_to_the_restatement over a 4-pose orbit + dolly: colour, N, moments,
    variance and weight sum as uint32 on every pixel after each pose, (alpha_min, max_history) = (0, 32) and (0.2, 4)."""
    sc, pos, fwd, depth = gt.scene(name)
    seq = gt.poses(pos, fwd, 4)
    for alpha_min, max_history in ((0.0, 32), (0.2, 4)):
        r = gt.renderer(W, H, depth)
        state = {"hist": None, "reused": 0}

        def check(k, cam, img, out):
            g = r.renderGuides(cam, sc, 1)
            ref = tp.reproject(state["hist"], img, g, tp.pinhole_of(cam, W, H), max_history=max_history, alpha_min=alpha_min)
            h = r.GetTemporalHistory()
            got = dict(color=h.color, length=h.length, m1=h.moments[..., 0], m2=h.moments[..., 1], variance=h.variance, weight=h.weight)
            for f in gt.FIELDS:
                bad = u32(got[f]) != u32(getattr(ref, f))
                assert not bad.any(), "%s %dx%d pose %d alpha_min %g max_history %d: %s differs on %d pixels (first %s: %r vs %r)" % (
                    name, W, H, k, alpha_min, max_history, f, bad.sum(), np.argwhere(bad)[0], got[f][bad][0], getattr(ref, f)[bad][0])
            state["hist"] = ref
            state["reused"] += int((ref.length > 1).sum())
        gt.run_sequence(r, sc, seq, check, iterations=0, alpha_min=alpha_min, max_history=max_history)
        assert state["reused"] > W * H, "the sequence reuses history"
        assert state["hist"].length.max() == min(4, max_history)


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("kind,alpha_min,max_history", [("translate", 0.0, 32), ("rotate", 0.2, 4)])
def test_reprojection_follows_refitted_geometry_at_full_size(kind, alpha_min, max_history, W, H):
    """test_gpu_motion.py::test_reprojection_follows_refitted_geometry on cornell_box with the camera moving: 4 calls, a device
    refit before each, every History field and the motion vectors as uint32 against reproject_motion / motion_vectors with the
    device's own TriHot records; pixels whose triangle did not move equal the static restatement."""
    name = "cornell_box"
    sc, pos0, sel, pos, fwd, depth = gm.scene(name)
    at = gm.mover(kind, pos0, sel, 1.0)
    r = gt.renderer(W, H, depth)
    r.trackMotion()
    hist = hot_prev = ph_prev = None
    moved_px = reused = 0
    for k, (cp, cf) in enumerate(gt.poses(pos, fwd, 4)):
        cam = gt.camera(cp, cf)
        r.refit(sc, gm.dev(at(k)))
        hot = r.debugReadDeviceScene(sc)[1].copy()
        ph = tp.pinhole_of(cam, W, H)
        r.resetAccumulationBuffer()
        r.Render(cam, sc)
        img = r.GetRenderTargetImage()
        g = r.renderGuides(cam, sc, 1)
        what = "%s %s %dx%d call %d alpha_min %g max_history %d" % (name, kind, W, H, k, alpha_min, max_history)
        mv = r.motionVectors(cam, sc) if k > 0 else None
        r.TemporalDenoise(cam, sc, iterations=0, alpha_min=alpha_min, max_history=max_history)
        got = gm.got_history(r)
        jobs = {"ref": lambda: mo.reproject_motion(hist, img, g, ph, hot, hot_prev, max_history=max_history, alpha_min=alpha_min),
                "static": lambda: tp.reproject(hist, img, g, ph, max_history=max_history, alpha_min=alpha_min),
                "rule": lambda: mo.previous_points(g, ph, hot, hot_prev)[2]}
        if k > 0:
            jobs["mv"] = lambda: mo.motion_vectors(g, ph, ph_prev, hot, hot_prev)
        res = _parallel(jobs)
        if k > 0:
            bad = (u32(mv) != u32(res["mv"])).any(axis=-1)
            assert not bad.any(), "%s: motion vectors differ on %d pixels (first %s: %r vs %r)" % (
                what, bad.sum(), np.argwhere(bad)[0], mv[bad][0], res["mv"][bad][0])
        ref, static, rule = res["ref"], res["static"], res["rule"]
        gm.assert_history(got, ref, what)
        gm.assert_history(got, static, what + " (unmoved pixels)", where=rule != mo.MOVED, fields=("color", "length", "m1", "m2", "weight"))
        gm.assert_history(got, static, what + " (unmoved pixels, temporal variance)", where=(rule != mo.MOVED) & (static.length >= 4),
                          fields=("variance",))
        moved_px += int((rule == mo.MOVED).sum())
        reused += int(((rule == mo.MOVED) & (ref.length > 1)).sum())
        hist, hot_prev, ph_prev = ref, hot, ph
    scale = (W * H) / (96.0 * 64.0)
    assert moved_px > 50 * scale, "the sequence moves visible triangles"
    assert reused > 20 * scale, "moved pixels keep a history"
