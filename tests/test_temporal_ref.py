"""The restatement of drt_renderer_temporal_denoise (tests/temporal_ref.py) on the CPU: properties that can be derived by hand --
history lengths under a still camera, the projection as the inverse of the camera's ray map, disocclusion on a two-quad scene,
and the two degenerate parameter choices (alpha_min = 1, zero passes)."""
import numpy as np
import pytest

import oracle
from tests import denoise_ref as dn
from tests import ray_query_ref as rq
from tests import temporal_ref as tp
from tests.scenes import SCENES, scene_path

drt = pytest.importorskip("dustraytracer_amd")
F = np.float32
_osc = {}


def _scene(name):
    if name not in _osc:
        _osc[name] = oracle.Scene.load_glb(scene_path(name)).build_bvh(20, 8)
    return _osc[name]


def _frame(osc, pos, fwd, W, H, depth=3):
    """(framebuffer of a 1-frame render, guides of frame 1, pinhole) of one pose, all from the oracle."""
    cam = oracle.default_camera(position=pos, forward=fwd)
    img, _, _ = oracle.render(osc, cam, oracle.default_settings(ray_bounce_limit=depth), W, H, 1, 1)
    return img, dn.guides(osc, cam, W, H, 1), tp.pinhole(pos, fwd, W, H, cam.vfov_rad, cam.focus_dist)


@pytest.mark.parametrize("name", ["cornell_box", "uv_texture_test"])
def test_still_camera_history_length(name):
    """k calls from one pose: the tap next to the pixel itself is always valid (same prim, same normal), every valid tap holds the
    same N, so N = min(k, max_history) on every hit pixel; a miss pixel never has a history."""
    _, pos, fwd, _ = SCENES[name]
    W, H = 48, 32
    img, g, ph = _frame(_scene(name), pos, fwd, W, H)
    hit = g.prim >= 0
    assert hit.any() and (~hit).any()
    hist = None
    for k in range(1, 7):
        hist = tp.reproject(hist, img, g, ph, max_history=4)
        assert (hist.length[hit] == min(k, 4)).all(), k
        assert (hist.length[~hit] == 1).all() and (hist.weight[~hit] == 0).all()
        if k > 1:
            assert (hist.weight[hit] > 0.99).all()


def test_projection_inverts_the_camera_ray_map():
    """project(pos + t * d0(p)) into the same camera gives (x, y) up to float32 rounding.  With u = 2^-24 and |pos| the largest
    coordinate magnitude: each component of P = pos + d0 * t carries at most u (|pos| + 6 t) (normalize: 3 roundings of d0, the
    product, the sum, then the difference P - pos); a dot with a unit vector at most sqrt(3) times that plus 3 u t, so <=
    u (2 |pos| + 14 t) for both dot(pv, right) and z.  z >= 0.9 t inside the default frustum at aspect <= 1.5 (tan of the half
    angles 0.4 and 0.268), focus / (z plane_h) <= 2.07 / t and plane_h / focus = 0.536, so |d sv| <= 2.07 * 1.536 * u (2 |pos| / t
    + 14) + 4 u <= u (7 |pos| / t + 50) (su: smaller).  The camera's own constants (uv, horizontal, fwd_focus, a basis that is
    orthonormal to 3 u, the final (s + 1) * 0.5 * W) add at most 30 u.  So |fx - x| <= (W / 2) u (7 |pos| / t + 80), and likewise
    with H: 0.018 pixel at W = 1920, |pos| / t = 32."""
    rng = np.random.default_rng(11)
    u = 2.0 ** -24
    worst = 0.0
    for W, H in ((1920, 1280), (96, 64), (64, 64), (7, 5)):
        for _ in range(12):
            pos = rng.uniform(-16, 16, 3).astype(F)
            fwd = rng.normal(size=3).astype(F)
            fwd[1] *= 0.3                                     # (not along the up axis, where the basis degenerates)
            ph = tp.pinhole(pos, fwd, W, H)
            d0 = tp.primary_directions(ph, W, H)
            t = rng.uniform(0.5, 60.0, (H, W)).astype(F)
            P = (ph.pos + d0 * t[..., None]).astype(F)
            fx, fy, ok = tp.project(ph, P, W, H)
            assert ok.all()
            y, x = np.mgrid[0:H, 0:W]
            ratio = float(np.abs(pos).max()) / t
            bx, by = (W / 2) * u * (7 * ratio + 80), (H / 2) * u * (7 * ratio + 80)
            ex, ey = np.abs(fx.astype(np.float64) - x), np.abs(fy.astype(np.float64) - y)
            worst = max(worst, float((ex / bx).max()), float((ey / by).max()))
            assert (ex <= bx).all() and (ey <= by).all(), (W, H, float((ex / bx).max()), float((ey / by).max()))
    print("largest |f - pixel| / bound = %.3f" % worst)


def _erode(mask, r):
    out = mask.copy()
    H, W = mask.shape
    p = np.pad(mask, r, constant_values=False)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out &= p[dy:dy + H, dx:dx + W]
    return out


def test_disocclusion_on_two_quads():
    """A foreground quad in front of a background quad, the camera stepping sideways.  A background point that the previous
    camera could not see reprojects onto foreground pixels, whose prim differs: no history (one pixel of erosion: a bilinear tap of
    a pixel on the set's rim can reach a background pixel).  A background point seen by both cameras, two pixels from every prim
    boundary in both frames and a pixel inside the previous image, finds four valid taps: N = 2."""
    W, H = 96, 64
    _, osc = rq.programmatic_scene(drt, *tp.two_quads(), 2, 8)
    fwd = (0.0, 0.0, -1.0)
    pos_a, pos_b = (-0.4, 0.1, 8.0), (0.5, 0.1, 8.0)
    img_a, g_a, ph_a = _frame(osc, pos_a, fwd, W, H)
    img_b, g_b, ph_b = _frame(osc, pos_b, fwd, W, H)
    h1 = tp.reproject(None, img_a, g_a, ph_a)
    h2 = tp.reproject(h1, img_b, g_b, ph_b)
    assert (h1.length == 1).all()

    def z_of(g):            # which quad a pixel shows: the depth of its hit (background z = 0, foreground z = 2, miss nan)
        return np.where(g.prim >= 0, np.where(g.t > 7.0, 0, 2), -1)
    back_b = z_of(g_b) == 0
    assert back_b.any() and (z_of(g_b) == 2).any()
    P = (ph_b.pos + tp.primary_directions(ph_b, W, H) * g_b.t[..., None]).astype(F)[back_b]
    to_a = (np.asarray(pos_a, F) - P).astype(F)
    occ = np.zeros((H, W), bool)
    occ[back_b] = rq.occluded(osc, P, to_a, F(1e-3), F(1.0)).astype(bool)
    assert occ.sum() > 20, "the step uncovers background"
    core = _erode(occ, 1)
    assert core.any()
    assert (h2.length[core] == 1).all() and (h2.weight[core] == 0).all()

    def interior(g):        # two pixels from any prim boundary
        same = np.ones((H, W), bool)
        p = np.pad(g.prim, 2, mode="edge")
        for dy in range(5):
            for dx in range(5):
                same &= p[dy:dy + H, dx:dx + W] == g.prim
        return same
    fx, fy, ok = tp.project(ph_a, (ph_b.pos + tp.primary_directions(ph_b, W, H) * g_b.t[..., None]).astype(F), W, H)
    inside = ok & (fx >= 1) & (fx < W - 2) & (fy >= 1) & (fy < H - 2)
    ix = np.clip(np.floor(np.where(ok, fx, 0)).astype(int), 0, W - 1)
    iy = np.clip(np.floor(np.where(ok, fy, 0)).astype(int), 0, H - 1)
    good = back_b & ~occ & inside & interior(g_b) & interior(g_a)[iy, ix] & (g_a.prim[iy, ix] == g_b.prim)
    assert good.sum() > 500
    assert (h2.length[good] == 2).all()
    assert (np.abs(h2.weight[good] - 1) < 1e-5).all()


def test_alpha_min_one_keeps_the_framebuffer():
    _, pos, fwd, _ = SCENES["cornell_box"]
    W, H = 40, 24
    osc = _scene("cornell_box")
    img1, g1, ph1 = _frame(osc, pos, fwd, W, H)
    pos2 = (pos[0], pos[1] + 0.05, pos[2] + 0.05)
    img2, g2, ph2 = _frame(osc, pos2, fwd, W, H)
    h = tp.reproject(None, img1, g1, ph1, alpha_min=1.0)
    h = tp.reproject(h, img2, g2, ph2, alpha_min=1.0)
    assert (h.length > 1).any()
    assert (h.color.view(np.uint32) == np.ascontiguousarray(img2[..., :3]).view(np.uint32)).all()


def test_zero_passes_give_the_integrated_colour():
    _, pos, fwd, _ = SCENES["cornell_box"]
    W, H = 40, 24
    img, g, ph = _frame(_scene("cornell_box"), pos, fwd, W, H)
    h, _ = tp.temporal_denoise(None, img, g, ph)
    h, out = tp.temporal_denoise(h, img, g, ph, iterations=0)
    assert (out[..., :3].view(np.uint32) == h.color.view(np.uint32)).all() and (out[..., 3] == 1).all()
    _, filtered = tp.temporal_denoise(None, img, g, ph, iterations=3)
    assert np.isfinite(filtered).all() and (filtered[..., 3] == 1).all() and np.abs(filtered[..., :3] - h.color).max() > 1e-3


# ---- the float32 restatement of stage (c) against the same formulas in float64: 96x64, oracle frames, 1 .. 10 passes ----
FP64_BOUND = 1e-3         # a quarter of an 8-bit step of display-referred values (the bound test_gpu_temporal.py names)


@pytest.mark.parametrize("sig", [dict(sigma_luma=4.0, sigma_normal=0.1, sigma_albedo=0.1), dict(sigma_luma=1.5, sigma_normal=0.35, sigma_albedo=0.05)])
@pytest.mark.parametrize("name", ["cornell_box", "uv_texture_test", "two_quads"])
def test_float32_filter_stays_near_the_float64_filter(name, sig):
    """atrous_var(dtype=float32), which the GPU is pinned to, against atrous_var(dtype=float64) on the history after one pose (the
    7x7 spatial variance everywhere) and after three (mixed history lengths and variances), after each of 10 passes.  The filter
    divides by sigma_luma * sqrt(gv) + 1e-4 and by wsum^2: where the variance is 0 the luminance term is 1e4 |dl|, and this is
    the check that float32 rounding under those divisions stays below the bound through step 512."""
    W, H = 96, 64
    if name == "two_quads":
        _, osc = rq.programmatic_scene(drt, *tp.two_quads(), 2, 8)
        seq, depth = [((0.1 * k, 0.1, 8.0), (0.0, 0.0, -1.0)) for k in range(3)], 3
    else:
        osc = _scene(name)
        _, pos, fwd, depth = SCENES[name]
        seq = [((pos[0], pos[1] + 0.02 * k, pos[2] + 0.03 * k), fwd) for k in range(3)]
    hist = None
    for k, (pos, fwd) in enumerate(seq):
        img, g, ph = _frame(osc, pos, fwd, W, H, depth)
        hist = tp.reproject(hist, img, g, ph)
        if k == 1:
            continue
        p32 = tp.atrous_var_passes(hist.color, hist.variance, g.albedo, g.normal, 10, **sig)
        p64 = tp.atrous_var_passes(hist.color, hist.variance, g.albedo, g.normal, 10, dtype=np.float64, **sig)
        errs = []
        for c32, c64 in zip(p32, p64):
            assert c32.dtype == np.float32 and c64.dtype == np.float64 and np.isfinite(c64).all()
            errs.append(float(np.abs(c32 - c64).max()))
        assert len(errs) == 10
        print("%s pose %d sigma_luma %g: max |fp32 - fp64| after passes 1..10 = %s" % (name, k, sig["sigma_luma"], " ".join("%.2e" % e for e in errs)))
        for K, e in enumerate(errs, 1):
            assert e <= FP64_BOUND, (name, k, K, e)
    assert (hist.length > 1).any() and (hist.length >= 3).any()
