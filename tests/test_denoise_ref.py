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
