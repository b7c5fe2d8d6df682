"""The motion rule's restatement (tests/motion_ref.py) on the CPU: equal to temporal_ref.reproject when nothing moved, a
hand-derivable translation and rotation on the two-quad scene, degenerate triangles, and what the rule is for -- a moving object
under a still camera converges where the static rule ghosts and a reset starts over.  TriHot records come from the host pack
(Scene.debugPack) before and after a host refit; frames and guides from the oracle on the refitted scene."""
import numpy as np
import pytest

import oracle
from tests import denoise_ref as dn
from tests import motion_ref as mo
from tests import ray_query_ref as rq
from tests import refit_ref as rf
from tests import temporal_ref as tp
from tests.scenes import SCENES, scene_path

drt = pytest.importorskip("dustraytracer_amd")
F = np.float32
U = 2.0 ** -24
W, H = 96, 64
QUAD_CAM = ((0.0, 0.1, 8.0), (0.0, 0.0, -1.0))


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _frame(osc, pos, fwd, depth=3):
    cam = oracle.default_camera(position=pos, forward=fwd)
    img, _, _ = oracle.render(osc, cam, oracle.default_settings(ray_bounce_limit=depth), W, H, 1, 1)
    return img, dn.guides(osc, cam, W, H, 1), tp.pinhole(pos, fwd, W, H, cam.vfov_rad, cam.focus_dist)


def assert_same_history(a, b, where=None, what=""):
    for f in mo.FIELDS:
        x, y = u32(getattr(a, f)), u32(getattr(b, f))
        bad = x != y
        if where is not None:
            bad = bad[where]
        assert not bad.any(), "%s: %s differs on %d values" % (what, f, bad.sum())


class Quads:
    """The two-quad scene as a product scene (for the packs and the refit) with the oracle's view of every refitted state."""

    def __init__(self):
        self.s = tp.two_quads()
        self.sc, self.osc0 = rq.programmatic_scene(drt, *self.s, 2, 8)
        self.pos0 = self.s[0].copy()
        order = self.sc.triangleOrder()
        self.fg = np.isin(order, [2, 3])                   # prims (triangle order) of the foreground quad

    def refit(self, pos):
        """Host refit to load-order positions: (oracle scene, TriHot records)."""
        self.sc.refit(pos)
        return mo.oracle_scene(self.sc, self.s[:4], self.s[4], self.s[5], pos), self.sc.debugPack()[1].copy()

    def moved_fg(self, fn):
        pos = self.pos0.copy()
        pos[2:4] = fn(pos[2:4])
        return pos


def test_host_pack_runs_without_a_gpu_and_follows_a_refit():
    q = Quads()
    hot0 = q.sc.debugPack()[1].copy()
    _, hot1 = q.refit(q.moved_fg(lambda p: p + F([0.5, 0, 0])))
    assert hot0.shape == (4, 48)
    assert (mo.moved_triangles(hot1, hot0) == q.fg).all()
    a, b = mo.records(hot0), mo.records(hot1)
    assert (u32(a[:, 3:]) == u32(b[:, 3:])).all()           # a translation by a representable step keeps e1, e2 and fn


@pytest.mark.parametrize("case", ["cornell_still", "cornell_step", "uv_still", "quads_step"])
def test_nothing_moved_equals_the_static_restatement(case):
    """hot_prev None, and hot_prev == hot: every field of reproject_motion equals temporal_ref.reproject's, as uint32, over the
    pose sequences of test_temporal_ref.py."""
    if case == "quads_step":
        q = Quads()
        osc, hot = q.osc0, q.sc.debugPack()[1]
        seq = [((-0.4, 0.1, 8.0), QUAD_CAM[1]), ((0.5, 0.1, 8.0), QUAD_CAM[1]), ((0.5, 0.1, 8.0), QUAD_CAM[1])]
    else:
        name = "uv_texture_test" if case == "uv_still" else "cornell_box"
        osc = oracle.Scene.load_glb(scene_path(name)).build_bvh(20, 8)
        sc = drt.Scene()
        sc.loadGLTFmodel(scene_path(name))
        b = drt.BVHBuilder()
        b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
        b.buildIterative(sc)
        hot = sc.debugPack()[1]
        _, pos, fwd, _ = SCENES[name]
        step = (0.05 if case == "cornell_step" else 0.0)
        seq = [((pos[0], pos[1] + step * k, pos[2] + step * k), fwd) for k in range(4)]
    for hot_prev in (None, hot.copy()):
        ref = got = None
        for pos, fwd in seq:
            img, g, ph = _frame(osc, pos, fwd)
            ref = tp.reproject(ref, img, g, ph, max_history=4)
            got = mo.reproject_motion(got, img, g, ph, hot, hot_prev, max_history=4)
            assert_same_history(got, ref, what=case)
            assert (u32(got.normal) == u32(ref.normal)).all() and (got.prim == ref.prim).all()
            mv = mo.motion_vectors(g, ph, ph, hot, hot_prev)
            assert set(np.unique(mv[..., 3])) <= {0.0, 1.0}
        assert (ref.length > 1).any()


def test_translation_inside_the_plane():
    """Still camera, the foreground quad (z = 2, 2 x 2) moved by d = (0.5, 0, 0).

    P' against P - d.  With u = 2^-24, |w|, |e1|, |e2| <= 2 sqrt(2), d11, d12, d22 <= 8 and den = 16 (all exact: small integers):
    w = P - v0 carries u |w|; w1 and w2 (three products, two sums, the error of w) at most 4 u |w| |e|; a numerator d22 w1 - d12 w2
    (two products, a difference) at most 6 u (d22 |w| |e1| + d12 |w| |e2|) <= 768 u, so b1 and b2 at most 768 u / 16 + u < 50 u;
    P' = (v0' + e1' b1) + e2' b2 at most (|e1'| + |e2'|) 50 u + 3 roundings of values below 4 < 300 u = 1.8e-5 per component.
    That holds for x and y.  P itself lies a little off the plane (g.t belongs to the jittered primary ray, d0 is the unjittered
    one: about 1e-3 in z here); the barycentric coordinates drop that component (e1.z = e2.z = 0 exactly), so P'.z = 2 exactly.

    The vector: right' = (1, 0, 0) for forward (0, 0, -1), so the previous position lies d / z * focus / plane_w * W / 2 =
    d H / (4 z tan(vfov / 4)) = 0.5 * 64 / (4 * 6 * tan 15 deg) = 4.98 pixels to the LEFT: mv = (-4.98, 0) within one pixel, z = 6."""
    q = Quads()
    hot0 = q.sc.debugPack()[1].copy()
    d = F([0.5, 0, 0])
    img0, g0, ph = _frame(q.osc0, *QUAD_CAM)
    osc1, hot1 = q.refit(q.moved_fg(lambda p: p + d))
    img1, g1, _ = _frame(osc1, *QUAD_CAM)
    fg = q.fg[np.clip(g1.prim, 0, 3)] & (g1.prim >= 0)
    bg = ~fg & (g1.prim >= 0)
    assert fg.sum() > 100 and bg.sum() > 1000
    Pp, n_tap, rule = mo.previous_points(g1, ph, hot1, hot0)
    P, _, _ = mo.previous_points(g1, ph, hot1, None)
    assert (rule[fg] == mo.MOVED).all() and (rule[bg] == mo.STATIC).all() and (rule[g1.prim < 0] == 0).all()
    err = np.abs(Pp[fg].astype(np.float64) - (P[fg].astype(np.float64) - d))[:, :2]
    print("largest |P' - (P - d)| = %.3e (bound %.3e)" % (err.max(), 300 * U))
    assert err.max() <= 300 * U
    assert (Pp[fg][:, 2] == F(2)).all()
    assert (u32(Pp[bg]) == u32(P[bg])).all() and (u32(n_tap) == u32(g1.normal)).all()

    mv = mo.motion_vectors(g1, ph, ph, hot1, hot0)
    expected = 0.5 * H / (4 * 6.0 * np.tan(np.radians(15.0)))
    assert (mv[fg][:, 3] == 2).all() and (mv[bg][:, 3] == 1).all() and (mv[g1.prim < 0] == 0).all()
    assert (np.abs(mv[fg][:, 0] + expected) < 1).all() and (np.abs(mv[fg][:, 1]) < 1).all() and (np.abs(mv[fg][:, 2] - 6) < 1e-4).all()
    assert (np.abs(mv[bg][:, :2]) < 1e-3).all() and (np.abs(mv[bg][:, 2] - 8) < 0.02).all()      # (P is off the plane by the jitter and the lens)

    h0 = tp.reproject(None, img0, g0, ph)
    moved = mo.reproject_motion(h0, img1, g1, ph, hot1, hot0)
    static = tp.reproject(h0, img1, g1, ph)
    assert_same_history(moved, static, where=bg, what="background pixels")
    assert (u32(moved.normal) == u32(static.normal)).all() and (moved.prim == static.prim).all()     # the key is the current one
    # a foreground pixel five pixels inside the quad's previous outline finds its own surface point again: N = 2 with weight 1
    fx, fy = np.mgrid[0:H, 0:W][1] + mv[..., 0], np.mgrid[0:H, 0:W][0] + mv[..., 1]
    ix, iy = np.clip(np.floor(fx).astype(int), 0, W - 2), np.clip(np.floor(fy).astype(int), 0, H - 2)
    seen = fg & (g0.prim[iy, ix] == g1.prim) & (g0.prim[iy + 1, ix] == g1.prim) & (g0.prim[iy, ix + 1] == g1.prim) & (g0.prim[iy + 1, ix + 1] == g1.prim)
    assert seen.sum() > 50
    assert (moved.length[seen] == 2).all() and (np.abs(moved.weight[seen] - 1) < 1e-5).all()


def test_rotation_keeps_the_history_through_the_previous_normal():
    """The foreground quad turned by 30 degrees about the vertical through its centre, normal_cos_min = 0.9 > cos 30 = 0.866: the
    static rule compares the stored normal (0, 0, 1) with the turned one and rejects every tap (N = 1); the moved rule compares it
    with the previous face normal n' = (0, 0, 1) and keeps the pixels it sees again (all four taps on the same triangle: N = 2)."""
    q = Quads()
    hot0 = q.sc.debugPack()[1].copy()
    img0, g0, ph = _frame(q.osc0, *QUAD_CAM)
    osc1, hot1 = q.refit(q.moved_fg(lambda p: mo.rotate_about(p, (0, 0, 2), (0, 1, 0), np.radians(30.0))))
    img1, g1, _ = _frame(osc1, *QUAD_CAM)
    fg = q.fg[np.clip(g1.prim, 0, 3)] & (g1.prim >= 0)
    assert fg.sum() > 100
    assert (np.abs(g1.normal[fg][:, 2] - np.cos(np.radians(30.0))) < 1e-5).all()
    h0 = tp.reproject(None, img0, g0, ph, normal_cos_min=0.9)
    moved = mo.reproject_motion(h0, img1, g1, ph, hot1, hot0, normal_cos_min=0.9)
    static = mo.reproject_motion(h0, img1, g1, ph, hot1, None, normal_cos_min=0.9)
    mv = mo.motion_vectors(g1, ph, ph, hot1, hot0)
    assert (mv[fg][:, 3] == 2).all()
    y, x = np.mgrid[0:H, 0:W]
    ix, iy = np.clip(np.floor(x + mv[..., 0]).astype(int), 0, W - 2), np.clip(np.floor(y + mv[..., 1]).astype(int), 0, H - 2)
    seen = fg & (g0.prim[iy, ix] == g1.prim) & (g0.prim[iy + 1, ix] == g1.prim) & (g0.prim[iy, ix + 1] == g1.prim) & (g0.prim[iy + 1, ix + 1] == g1.prim)
    assert seen.sum() > 50
    assert (moved.length[seen] >= 2).all()
    assert (static.length[fg] == 1).all()
    assert_same_history(moved, static, where=~fg, what="pixels off the turned quad")


def test_degenerate_triangles():
    """A current record without area or with a NaN takes the static rule (den is not > 0); a snapshot record without area (its face
    normal is NaN) or all NaN leaves no history on its pixels and no NaN anywhere."""
    q = Quads()
    hot0 = q.sc.debugPack()[1].copy()
    img0, g0, ph = _frame(q.osc0, *QUAD_CAM)
    osc1, hot1 = q.refit(q.moved_fg(lambda p: p + F([0.5, 0, 0])))
    img1, g1, _ = _frame(osc1, *QUAD_CAM)
    h0 = tp.reproject(None, img0, g0, ph)
    static = tp.reproject(h0, img1, g1, ph)
    k0, k1 = np.nonzero(q.fg)[0]
    on0, on1 = g1.prim == k0, g1.prim == k1
    assert on0.sum() > 50 and on1.sum() > 50

    cur = mo.records(hot1).copy()
    cur[k0, 6:9] = cur[k0, 3:6]                             # e2 = e1: no area
    cur[k1, 4] = np.nan
    _, _, rule = mo.previous_points(g1, ph, cur, hot0)
    assert (rule[on0] == mo.STATIC).all() and (rule[on1] == mo.STATIC).all()
    assert_same_history(mo.reproject_motion(h0, img1, g1, ph, cur, hot0), static, what="degenerate current records")
    mv = mo.motion_vectors(g1, ph, ph, cur, hot0)
    assert np.isfinite(mv).all() and (mv[on0 | on1][:, 3] == 1).all()

    old = mo.records(hot0).copy()
    old[k0, 6:9] = old[k0, 3:6]
    old[k0, 9:12] = np.nan                                  # what a refit stores for a triangle without area
    old[k1] = np.nan
    got = mo.reproject_motion(h0, img1, g1, ph, hot1, old)
    for f in mo.FIELDS:
        assert np.isfinite(getattr(got, f)).all(), f
    assert (got.length[on0 | on1] == 1).all() and (got.weight[on0 | on1] == 0).all()
    assert_same_history(got, static, where=~(on0 | on1), what="pixels off the degenerate snapshot records")
    mv = mo.motion_vectors(g1, ph, ph, hot1, old)
    assert (mv[on1] == 0).all()                             # z is NaN: no vector


# ---- what the rule is for: a textured object moving under a still camera ----
MOVING = dict(name="uv_texture_test", mesh=3, step=(0.06, 0.0, 0.0), poses=10, truth_spp=256)


def quality(frames):
    """frames: [(img, guides, pinhole, hot)] per pose, truth of the last pose, moved prims -> the three RMSEs."""
    seq, truth, moved_prims = frames
    hm = hs = None
    hot_prev = None
    for img, g, ph, hot in seq:
        hm = mo.reproject_motion(hm, img, g, ph, hot, hot_prev)
        hs = tp.reproject(hs, img, g, ph)
        hot_prev = hot
    hr = tp.reproject(None, *seq[-1][:3])                   # the history reset at every move: this pose's frame alone
    g = seq[-1][1]
    sel = np.isin(g.prim, moved_prims)
    assert sel.sum() > 200
    return tuple(tp.rmse(h.color[sel], truth[sel]) for h in (hm, hs, hr)), hm


def oracle_moving_frames(cfg=MOVING):
    name = cfg["name"]
    sc = drt.Scene()
    sc.loadGLTFmodel(scene_path(name))
    st = rf.streams(sc.m_PrimitivesBuffer)
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
    b.buildIterative(sc)
    base = oracle.Scene.load_glb(scene_path(name))
    mats = [(tuple(m["albedo"]), int(m["albedo_tex"])) for m in base.mats[:base.n_mats]]
    _, pos, fwd, depth = SCENES[name]
    mesh = sc.m_Meshes[cfg["mesh"]]
    lo, n = int(mesh["primitives_offset"]), int(mesh["tris_count"])
    moved_prims = np.nonzero(np.isin(sc.triangleOrder(), np.arange(lo, lo + n)))[0]
    seq, truth = [], None
    for k in range(cfg["poses"]):
        p = st[0].copy()
        p[lo:lo + n] += F(cfg["step"]) * F(k)
        sc.refit(p)
        osc = mo.oracle_scene(sc, st, mats, base.textures, p)
        img, g, ph = _frame(osc, pos, fwd, depth)
        seq.append((img, g, ph, sc.debugPack()[1].copy()))
        if k == cfg["poses"] - 1:
            cam = oracle.default_camera(position=pos, forward=fwd)
            truth, _, _ = oracle.render(osc, cam, oracle.default_settings(ray_bounce_limit=depth, max_samples=100000), W, H, 1, cfg["truth_spp"])
    return seq, truth[..., :3], moved_prims


def test_a_moving_object_converges_under_the_moved_rule():
    """1-spp oracle frames of uv_texture_test with one textured mesh moving 0.06 per pose across 10 poses under a still camera,
    against the oracle's 256-spp render of the last pose, over the pixels of the moved triangles: RMSE(moved rule) <
    RMSE(static rule) (which blends what the triangle showed elsewhere) and RMSE(moved rule) < RMSE(reset at every move) (one
    sample per pixel).  Strict inequalities between runs of the restatement on the same inputs; the figures are in DESIGN 5.12."""
    (e_moved, e_static, e_reset), hm = quality(oracle_moving_frames())
    print("RMSE over the moved triangles' pixels: moved rule %.5f, static rule %.5f, reset at every move %.5f" % (e_moved, e_static, e_reset))
    assert hm.length.max() >= 8
    assert e_moved < e_static
    assert e_moved < e_reset
