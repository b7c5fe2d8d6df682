"""tests/radiance_ref.py (the restatement of drt_renderer_radiance the GPU tests compare with) against the oracle's renderer: fed
with the oracle's own primary rays (kat_getray: the ray and the seed state after Camera::GetRay), one sample of every pixel equals
oracle.render's frame sample bit for bit -- with sunlight on and off, bounce limits 0 / 2 / 8, tone curve and gamma on and off,
alpha cut-outs, and every lobe of the material model."""
import numpy as np
import pytest

import oracle
from tests import radiance_ref as rr
from tests.scenes import SCENES, scene_path

W, H = 24, 16
_cache = {}


def scene(name):
    if name not in _cache:
        _cache[name] = oracle.Scene.load_glb(scene_path(name)).build_bvh(20, 8)
    return _cache[name]


def camera_paths(cam, frame):
    """(org, dir, seed after GetRay) of every pixel in frame `frame`, row-major from y = 0 (RayGen.cuh:65-85)."""
    y, x = np.mgrid[0:H, 0:W]
    x, y = x.ravel().astype(np.uint32), y.ravel().astype(np.uint32)
    uv = np.stack([(x.astype(np.float32) / np.float32(W)) * np.float32(2) - np.float32(1),
                   (y.astype(np.float32) / np.float32(H)) * np.float32(2) - np.float32(1)], axis=1).astype(np.float32)
    r6, seeds = oracle.kat_getray(cam, W, H, uv, ((x + y * np.uint32(W)) * np.uint32(frame)).astype(np.uint32))
    return r6[:, :3].copy(), r6[:, 3:].copy(), seeds


def check(osc, cam, st, frame, what):
    org, dirs, seeds = camera_paths(cam, frame)
    got = np.float32(0) + rr.radiance(osc, org, dirs, seeds, np.full(len(org), cam.exposure, np.float32), st)
    _, ref, _ = oracle.render(osc, cam, st, W, H, frame, 1)
    ref = ref.reshape(-1, 3)
    bad = (got.view(np.uint32) != ref.view(np.uint32)).any(axis=1)
    assert not bad.any(), "%s: %d of %d pixels differ, first %d: %r vs %r" % (what, bad.sum(), len(bad), np.argmax(bad), got[np.argmax(bad)], ref[np.argmax(bad)])


@pytest.mark.parametrize("name", ["cornell_box", "uv_texture_test", "mc_transparency"])
@pytest.mark.parametrize("sun", [0, 1])
@pytest.mark.parametrize("depth", [0, 2, 8])
@pytest.mark.parametrize("frame", [1, 3])
def test_restatement_equals_the_oracle_frame_sample(name, sun, depth, frame):
    _, pos, fwd, _ = SCENES[name]
    cam = oracle.default_camera(position=pos, forward=fwd, exposure=2.5)
    check(scene(name), cam, oracle.default_settings(ray_bounce_limit=depth, enable_sunlight=sun), frame, "%s sun=%d depth=%d" % (name, sun, depth))


def test_restatement_without_tone_curve_and_gamma():
    _, pos, fwd, _ = SCENES["cornell_box"]
    cam = oracle.default_camera(position=pos, forward=fwd)
    check(scene("cornell_box"), cam, oracle.default_settings(ray_bounce_limit=4, enable_sunlight=1, tone_mapping=0, gamma_correction=0), 2, "no tone")


@pytest.mark.parametrize("model", [(1, 0, 2.0), (0, 1, 1.0), (1, 1, 2.5)])
def test_restatement_with_the_emissive_and_mirror_lobes(model):
    osc = scene("emissive_test")
    _, pos, fwd, depth = SCENES["emissive_test"]
    cam = oracle.default_camera(position=pos, forward=fwd)
    osc.material_model = model
    try:
        for sun in (0, 1):
            check(osc, cam, oracle.default_settings(ray_bounce_limit=depth, enable_sunlight=sun), 2, "emissive_test %r sun=%d" % (model, sun))
    finally:
        osc.material_model = (0, 0, 1.0)


@pytest.mark.parametrize("model", [(0, 0, 1.0, 1), (1, 1, 1.5, 1)])
def test_restatement_with_the_dielectric_lobe(model):
    pytest.importorskip("dustraytracer_amd")                       # (the glass scene is built for the product too)
    from tests.test_material_model import _glass_scene
    _, osc = _glass_scene(0)
    cam = oracle.default_camera(position=(0.3, 1.6, 2.8), forward=(-0.1, -0.15, -1.0))
    osc.material_model = model
    for sun in (0, 1):
        check(osc, cam, oracle.default_settings(ray_bounce_limit=7, enable_sunlight=sun), 3, "glass %r sun=%d" % (model, sun))
