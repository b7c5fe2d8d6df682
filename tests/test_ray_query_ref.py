"""CPU checks of the ray-query restatement (tests/ray_query_ref.py) -- the yardstick tests/test_gpu_ray_query.py holds the
kernels to: it agrees with a brute force over all triangles, and on camera rays with what the oracle's renderer draws."""
import ctypes
import os

import numpy as np
import pytest

import oracle
from tests import ray_query_ref as rq
from tests.scenes import ROOT, SCENES, scene_path

BF_SCENES = ["cornell_box", "suzanne_plane", "mc_transparency", "uv_texture_test"]


@pytest.fixture(scope="module")
def scenes():
    return {name: oracle.Scene.load_glb(scene_path(name)).build_bvh(20, 8) for name in BF_SCENES}


def _check_against_brute_force(osc, org, dirs, tmin, tmax, what, boundary_share=200):
    hits = rq.closest(osc, org, dirs, tmin, tmax)
    occ = rq.occluded(osc, org, dirs, tmin, tmax)
    tbf, acc, tpair = rq.brute_force(osc, org, dirs, tmin, tmax)
    n = len(org)
    hit = hits.prim >= 0
    # never a hit that brute force does not accept, and at that hit's t
    r = np.nonzero(hit)[0]
    assert acc[r, hits.prim[r]].all(), what
    assert (tpair[r, hits.prim[r]].view(np.uint32) == hits.t[r].view(np.uint32)).all(), what
    # misses keep t = tmax, u = v = 0
    tmax_b = np.broadcast_to(np.float32(tmax), n).astype(np.float32)
    assert (hits.t[~hit].view(np.uint32) == tmax_b[~hit].view(np.uint32)).all(), what
    assert (hits.u[~hit] == 0).all() and (hits.v[~hit] == 0).all(), what
    # brute force's minimum t, except on rays a slab test at a box boundary sends past the closest triangle
    differ = hits.t.view(np.uint32) != tbf.view(np.uint32)
    assert (hits.t[differ] > tbf[differ]).all() or not differ.any(), what
    assert differ.sum() <= max(2, n // boundary_share), "%s: %d of %d rays miss the closest triangle" % (what, differ.sum(), n)
    # occlusion: only accepted pairs occlude (any accepted pair within (tmin, tmax) -- the tmax test at the boxes can only drop)
    any_acc = acc.any(axis=1)
    assert not (occ & ~any_acc).any(), what
    assert (occ != any_acc).sum() <= max(2, n // boundary_share), what
    return hits, occ


@pytest.mark.parametrize("name", BF_SCENES)
def test_restatement_agrees_with_brute_force(scenes, name):
    osc = scenes[name]
    rng = np.random.default_rng(11)
    n = 1200 if len(osc.tris) < 2000 else 300
    org, dirs = rq.surface_rays(osc, n, rng)
    _check_against_brute_force(osc, org, dirs, np.float32(0), rq.FLT_MAX, name + " surface rays, default interval")
    org, dirs, tmin, tmax = rq.interval_rays(osc, n, rng)
    # (NaN bounds: brute force and traversal agree there by construction, keep finite ones for the minimum-t count)
    fin = np.isfinite(tmin) & ~np.isnan(tmax)
    _check_against_brute_force(osc, org[fin], dirs[fin], tmin[fin], tmax[fin], name + " random intervals")
    org, dirs = rq.axis_rays(osc, n, rng)
    # (a zero direction component with the origin on a flat box's plane: 0 * inf = NaN in the slab test, the box is missed --
    #  a fifth of these origins are copied from vertex coordinates on purpose, so more of them land there)
    _check_against_brute_force(osc, org, dirs, np.float32(0), np.float32(np.inf), name + " axis-aligned", boundary_share=10)


def test_nan_and_negative_tmax_hit_nothing(scenes):
    osc = scenes["cornell_box"]
    rng = np.random.default_rng(3)
    org, dirs = rq.surface_rays(osc, 200, rng)
    for tmax in (np.float32(np.nan), np.float32(-1), np.float32(0)):
        hits = rq.closest(osc, org, dirs, 0, tmax)
        assert (hits.prim == -1).all() and not rq.occluded(osc, org, dirs, 0, tmax).any()
        assert (hits.t.view(np.uint32) == np.float32(tmax).view(np.uint32)).all()


@pytest.mark.parametrize("name", ["cornell_box", "suzanne_plane", "mc_transparency", "uv_texture_test"])
def test_camera_rays_match_the_oracle_images(scenes, name):
    """Hit or miss = pixel black in a zero-bounce render without tone mapping, gamma and sun (a hit leaves light at 0, a miss adds
    the sky); (1 - u - v, u, v) = the barycentric debug view bit for bit (RayGen.cuh:137-169, drt_oracle.c:560-575)."""
    osc = scenes[name]
    _, pos, fwd, _ = SCENES[name]
    W, H = 64, 40
    cam = oracle.default_camera(position=pos, forward=fwd)
    org, dirs = rq.camera_rays(cam, W, H)
    hits = rq.closest(osc, org, dirs, np.float32(0), rq.FLT_MAX)
    s = oracle.default_settings(ray_bounce_limit=0, tone_mapping=0, gamma_correction=0, enable_sunlight=0)
    img, _, _ = oracle.render(osc, cam, s, W, H, 1, 1)
    black = (img[..., :3] == 0).all(axis=-1).ravel()
    hit = hits.prim >= 0
    assert hit.any() and (~hit).any()
    assert (black == hit).all(), "%d pixels disagree" % (black != hit).sum()
    s = oracle.default_settings(render_mode=1, debug_mode=2)
    dbg, _, _ = oracle.render(osc, cam, s, W, H, 1, 1)
    dbg = dbg[..., :3].reshape(-1, 3)[hit]
    one = np.float32(1)
    bary = np.stack([one - hits.u[hit] - hits.v[hit], hits.u[hit], hits.v[hit]], axis=1).astype(np.float32)
    bary = np.float32(0) + bary          # the frame is added to a zeroed sum (RenderKernel.cu:29): a -0 barycentric shows as +0
    assert (dbg.view(np.uint32) == bary.view(np.uint32)).all()
    # occlusion along the same rays = hit (no alpha-rejected-only rays reach past every surface here)
    occ = rq.occluded(osc, org, dirs, np.float32(0), np.float32(np.inf))
    assert (occ == hit).all()


def test_deep_and_large_trees_are_walked_whole():
    """The degenerate chain of the GPU test (a tree deeper than the kernels' LDS stack levels) against brute force."""
    pos, nrm, uv, mat, materials, textures = rq.degenerate_chain()
    tris = np.zeros(len(mat), oracle.TRI_DTYPE)
    a = [np.ascontiguousarray(x, np.float32) for x in (pos.reshape(-1, 3), nrm.reshape(-1, 3), uv.reshape(-1, 2))]
    oracle.lib().o_build_triangles(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, np.ascontiguousarray(mat, np.int32).ctypes.data,
                                   len(mat), tris.ctypes.data)
    osc = oracle.Scene(tris, materials, textures).build_bvh(1, 2)
    assert oracle.tree_depth(osc.nodes) > 32
    rng = np.random.default_rng(2)
    org = np.tile(np.float32([-3.0, 0.0, 0.0]), (300, 1))
    dirs = np.concatenate([np.ones((300, 1), np.float32), rng.normal(scale=0.02, size=(300, 2)).astype(np.float32)], axis=1)
    _check_against_brute_force(osc, org, dirs, np.float32(0), rq.FLT_MAX, "degenerate chain")


def test_ray_query_entry_points_are_exported():
    lib = ctypes.CDLL(os.path.join(ROOT, "dustraytracer_amd", "libdrt_hip.so"))
    for name in ("drt_renderer_trace_rays", "drt_renderer_occluded"):
        assert hasattr(lib, name), name
