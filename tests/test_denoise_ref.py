"""The a-trous restatement (tests/denoise_ref.py) on the CPU: identity at 0 passes, constants stay constant, a plain B3-spline
a-trous blur when nothing stops the edges, and what it does to the noise of oracle renders."""
import numpy as np
import pytest

import oracle
from tests import denoise_ref as dn
from tests.scenes import SCENES, scene_path


def _random_frame(H, W, seed):
    rng = np.random.default_rng(seed)
    rgba = rng.uniform(0, 1, (H, W, 4)).astype(np.float32)
    albedo = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
    normal = rng.normal(size=(H, W, 3)).astype(np.float32)
    return rgba, albedo, normal


def test_zero_passes_are_the_identity():
    rgba, albedo, normal = _random_frame(13, 17, 1)
    out = dn.atrous(rgba, albedo, normal, iterations=0)
    assert (out.view(np.uint32) == rgba.view(np.uint32)).all()


@pytest.mark.parametrize("shape", [(1, 1), (3, 7), (40, 33)])
def test_a_constant_image_stays_constant(shape):
    H, W = shape
    _, albedo, normal = _random_frame(H, W, 2)
    rgba = np.empty((H, W, 4), np.float32)
    rgba[...] = np.float32([0.3, 0.55, 0.8, 0.25])
    out = dn.atrous(rgba, albedo, normal, iterations=5)
    assert np.abs(out - rgba).max() <= 1e-6
    assert (out[..., 3] == rgba[..., 3]).all()


def _plain_atrous(rgb, iterations):
    """B3-spline a-trous blur with edge-clamped taps: padded copies, no edge stopping."""
    c = rgb.astype(np.float64)
    H, W = c.shape[:2]
    for i in range(iterations):
        s = 1 << i
        p = np.pad(c, ((2 * s, 2 * s), (2 * s, 2 * s), (0, 0)), mode="edge")
        out = np.zeros_like(c)
        for b in range(5):
            for a in range(5):
                out += float(dn.B3[a]) * float(dn.B3[b]) * p[b * s:b * s + H, a * s:a * s + W]
        c = out
    return c


def test_uniform_guides_and_huge_sigmas_are_a_plain_blur():
    rgba, _, _ = _random_frame(37, 29, 3)
    albedo = np.full((37, 29, 3), 0.5, np.float32)
    normal = np.tile(np.float32([0, 1, 0]), (37, 29, 1))
    out = dn.atrous(rgba, albedo, normal, iterations=4, sigma_color=1e6, sigma_normal=1.0, sigma_albedo=1.0)
    assert np.abs(out[..., :3] - _plain_atrous(rgba[..., :3], 4)).max() < 2e-6
    assert (out[..., 3] == rgba[..., 3]).all()


def test_edges_stop_the_blur():
    """Two halves with different albedo: no colour crosses the seam, whatever the colour distance."""
    H, W = 16, 32
    rgba = np.zeros((H, W, 4), np.float32)
    rgba[:, W // 2:, :3] = 1.0
    albedo = np.zeros((H, W, 3), np.float32)
    albedo[:, W // 2:] = 1.0
    normal = np.tile(np.float32([0, 0, 1]), (H, W, 1))
    out = dn.atrous(rgba, albedo, normal, iterations=5, sigma_color=1e6)
    assert np.abs(out[..., :3] - rgba[..., :3]).max() < 1e-30


# ---- quality: 160x120, 4 spp against 512 spp of the oracle, guides of frame 1, default parameters ----
W, H = 160, 120
GATES = {"cornell_box": 0.25, "suzanne_plane": 0.5, "uv_texture_test": 1.0}


@pytest.mark.parametrize("name", sorted(GATES))
def test_denoised_noise_is_lower(name):
    _, pos, fwd, depth = SCENES[name]
    osc = oracle.Scene.load_glb(scene_path(name)).build_bvh(20, 8)
    cam = oracle.default_camera(position=pos, forward=fwd)
    st = oracle.default_settings(ray_bounce_limit=depth)
    noisy, _, _ = oracle.render(osc, cam, st, W, H, 1, 4)
    clean, _, _ = oracle.render(osc, cam, st, W, H, 1, 512)
    g = dn.guides(osc, cam, W, H, 1)
    out = dn.atrous(noisy, g.albedo, g.normal, **dn.DEFAULTS)
    ratio = dn.mse(out, clean) / dn.mse(noisy, clean)
    print("%s: MSE denoised / noisy = %.3f" % (name, ratio))
    assert ratio <= GATES[name]


# ---- the float32 restatement against the same formulas in float64: 96x64, 1 spp of the oracle, 1 .. 10 passes ----
FP64_BOUND = 1e-3         # a quarter of an 8-bit step of display-referred values (the bound test_gpu_temporal.py names)


@pytest.mark.parametrize("sig", [dict(sigma_color=0.5, sigma_normal=0.1, sigma_albedo=0.1), dict(sigma_color=0.8, sigma_normal=0.35, sigma_albedo=0.05)])
@pytest.mark.parametrize("name", ["cornell_box", "uv_texture_test", "suzanne_plane"])
def test_float32_restatement_stays_near_the_float64_filter(name, sig):
    """atrous(dtype=float32), which the GPU is pinned to, against atrous(dtype=float64) on the same inputs after each of 10
    passes (steps 1 .. 512, each chain fed by its own previous pass).  The passes past the image size are part of it: at 96x64
    every tap of steps 128 .. 512 is clamped to the border."""
    _, pos, fwd, depth = SCENES[name]
    Wt, Ht = 96, 64
    osc = oracle.Scene.load_glb(scene_path(name)).build_bvh(20, 8)
    cam = oracle.default_camera(position=pos, forward=fwd)
    noisy, _, _ = oracle.render(osc, cam, oracle.default_settings(ray_bounce_limit=depth), Wt, Ht, 1, 1)
    g = dn.guides(osc, cam, Wt, Ht, 1)
    p32 = dn.atrous_passes(noisy, g.albedo, g.normal, 10, **sig)
    p64 = dn.atrous_passes(noisy, g.albedo, g.normal, 10, dtype=np.float64, **sig)
    errs = []
    for K, (c32, c64) in enumerate(zip(p32, p64), 1):
        assert c32.dtype == np.float32 and c64.dtype == np.float64
        errs.append(float(np.abs(c32 - c64).max()))
    assert len(errs) == 10
    print("%s sigma_color %g: max |fp32 - fp64| after passes 1..10 = %s" % (name, sig["sigma_color"], " ".join("%.2e" % e for e in errs)))
    for K, e in enumerate(errs, 1):
        assert e <= FP64_BOUND, (name, K, e)


def test_float64_argument_leaves_the_float32_restatement_alone():
    """dtype is a pure addition: the float32 result is what atrous() gave before it had the argument (the loop written out here),
    and float64 of 0 passes is the input."""
    rgba, albedo, normal = _random_frame(21, 19, 5)
    out = dn.atrous(rgba, albedo, normal, iterations=2)
    f = np.float32
    c = rgba[..., :3].copy()
    ys, xs = np.arange(21), np.arange(19)
    for i in range(2):
        s = 1 << i
        wsum, csum = np.zeros((21, 19), f), np.zeros((21, 19, 3), f)
        for b in range(5):
            qy = np.clip(ys + (b - 2) * s, 0, 20)
            for a in range(5):
                qx = np.clip(xs + (a - 2) * s, 0, 18)
                cq = c[qy][:, qx]
                e = (dn._sq(c - cq) * (f(s) * (f(1) / (f(0.5) * f(0.5)))) + dn._sq(normal - normal[qy][:, qx]) * (f(1) / (f(0.1) * f(0.1)))) \
                    + dn._sq(albedo - albedo[qy][:, qx]) * (f(1) / (f(0.1) * f(0.1)))
                w = (dn.B3[a] * dn.B3[b]) * np.exp(-e).astype(f)
                wsum = wsum + w
                csum = csum + cq * w[..., None]
        c = (csum / wsum[..., None]).astype(f)
    assert out.dtype == np.float32 and (out[..., :3].view(np.uint32) == c.view(np.uint32)).all()
    out64 = dn.atrous(rgba, albedo, normal, iterations=0, dtype=np.float64)
    assert out64.dtype == np.float64 and (out64 == rgba).all()
