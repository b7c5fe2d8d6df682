"""-m gpu: path_pool after the "issue diet"  still renders the oracle's bits where its cuts could go wrong:
the per-batch reciprocal guard on both sides of its bound and on every leaf shape (the unguarded copy of the T loop reads the
same pairs past a lane's leaf as the guarded one), and the sample id -> pixel mapping on odd frames, sample counts and shards.  csrc/pool_index.hpp itself: tests/test_pool_index.py."""
import numpy as np
import pytest

import oracle
from tests.scenes import bits
from tests.test_gpu_parity import _programmatic_pair, _render_both, cameras, compare, make_pair, settings_pair

pytestmark = pytest.mark.gpu
drt = pytest.importorskip("dustraytracer_amd")


@pytest.fixture(scope="module")
def renderer():
    return drt.Renderer(0)


def _quad(a, b, c, d):
    return [[a, b, c], [a, c, d]]


def _cube(lo, hi):
    x0, y0, z0 = lo
    x1, y1, z1 = hi
    p = lambda i, j, k: [(x0, x1)[i], (y0, y1)[j], (z0, z1)[k]]
    return (_quad(p(0, 0, 0), p(0, 1, 0), p(1, 1, 0), p(1, 0, 0)) + _quad(p(0, 0, 1), p(1, 0, 1), p(1, 1, 1), p(0, 1, 1)) +
            _quad(p(0, 0, 0), p(1, 0, 0), p(1, 0, 1), p(0, 0, 1)) + _quad(p(0, 1, 0), p(0, 1, 1), p(1, 1, 1), p(1, 1, 0)) +
            _quad(p(0, 0, 0), p(0, 0, 1), p(0, 1, 1), p(0, 1, 0)) + _quad(p(1, 0, 0), p(1, 1, 0), p(1, 1, 1), p(1, 0, 1)))


def courtyard():
    """34 triangles: a floor and four walls open to the sky, two closed boxes standing in it.  float32 [n, 3, 3]."""
    floor_walls = _cube((-4.0, 0.0, -4.0), (4.0, 5.0, 4.0))
    tris = floor_walls[:6] + floor_walls[8:]            # (without the lid: y = 5)
    tris += _cube((-2.5, 0.0, -2.0), (-0.5, 2.0, 0.0)) + _cube((0.75, 0.0, -1.0), (2.25, 3.0, 0.5))
    return np.float32(tris)


def courtyard_pair(scale_log2, pos=None, leaf=6):
    pos = courtyard() if pos is None else pos
    pos = (pos * np.float32(2.0) ** np.float32(scale_log2)).astype(np.float32)        # (a power of two: exact)
    n = len(pos)
    e1, e2 = pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0]
    with np.errstate(all="ignore"):
        fn = np.cross(e1.astype(np.float64), e2.astype(np.float64))
        fn = np.nan_to_num(fn / np.linalg.norm(fn, axis=1, keepdims=True)).astype(np.float32)
    nrm = np.repeat(fn[:, None, :], 3, axis=1)
    mats = [((0.8, 0.7, 0.6), -1), ((0.3, 0.6, 0.9), -1)]
    mat = (np.arange(n) % 2).astype(np.int32)
    sc, osc = _programmatic_pair(pos, nrm, np.zeros((n, 3, 2), np.float32), mat, mats, [], leaf, 8)
    return sc, osc, pos


CAM_POS, CAM_FWD = (0.2, 2.5, 3.5), (0.05, -0.35, -1.0)
# The scales of the issue are 2^-40, 1, 2^30 and 2^52, camera scaled with the scene (position and focus distance: the primary
# ray is pixel - position, which cancels to nothing at a position of 2^30 with the focus 10 away).  The oracle's image is
# degenerate at both ends: at 2^-40 every |det| is below the test's absolute 1e-6 and at 2^52 every det overflows, so both
# images are sky only.  They stay as cases (the bits still have to match, and at 2^52 no lane is below the bound), and 2^-10
# and 2^36 are added next to them: the smallest and largest scales tried at which the oracle still hits the geometry
# (2^36: primary rays have |det| ~ 2^117, above the guard's 2^100; bounce rays are below the bound, so batches mix).
# 2^40 takes the primary rays' |det| to the top of the float range (~2^125 to overflow), where v_rcp_f32 returns denormals
# and zeros: the scale at which a batch wrongly taken for safe is most likely to show.
SCALES = {-40: False, -10: True, 0: True, 30: True, 36: True, 40: True, 52: False}        # scale -> the oracle's rays hit something


def safe_dir_of(pos):
    """The bound of csrc/pool_index.hpp pool_safe_dir, in double: the largest direction component with 8 D E^2 <= 2^99."""
    with np.errstate(all="ignore"):
        e = np.abs(np.concatenate([pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0]]).astype(np.float32))
    if not np.isfinite(e).all():
        return 0.0
    return float(2.0 ** 96 / float(e.max()) ** 2)


def render_scaled(renderer, sc, osc, k, W=16, H=16, frames=2):
    scale = np.float32(2.0) ** np.float32(k)
    pos = tuple(float(np.float32(c) * scale) for c in CAM_POS)
    cam = drt.Camera(pos)
    cam.m_Forward_dir = np.array(CAM_FWD, np.float32)
    cam.focus_dist = float(np.float32(cam.focus_dist) * scale)
    ocam = oracle.default_camera(position=pos, forward=CAM_FWD, focus_dist=cam.focus_dist)
    s, o = settings_pair(ray_bounce_limit=3)
    ref, _, cnt = oracle.render(osc, ocam, o, W, H, 1, frames, want_counters=True)
    if renderer is None:
        return None, ref, cnt.as_dict()
    renderer.m_RendererSettings = s
    renderer.ResizeBuffer(W, H)
    renderer.resetAccumulationBuffer()
    renderer.RenderBatch(cam, sc, frames)
    return renderer.GetRenderTargetImage(), ref, cnt.as_dict()


@pytest.mark.parametrize("k", sorted(SCALES))
def test_guard_on_both_sides_of_its_bound(renderer, k):
    """The same courtyard and camera at seven scales.  The bound on a safe direction component is 2^96 / E^2: far above every
    direction up to 2^0, 2^30 at 2^30 (primary rays, ~2^33 long, are above it, bounce rays below), 2^18 at 2^36, 2^10 at 2^40 and below every
    direction at 2^52, where every batch keeps the guarded loop."""
    sc, osc, pos = courtyard_pair(k)
    bound = safe_dir_of(pos)
    assert (bound < 0.5) if k == 52 else (bound > 4.0), (k, bound)
    img, ref, counted = render_scaled(renderer, sc, osc, k)
    assert "path_pool<lean,lds-scene>" in renderer.kernelInfo(), renderer.kernelInfo()
    assert np.isfinite(ref).all()
    assert (counted["hits_flat"] > 500) == SCALES[k], (k, counted["hits_flat"])
    compare(img, ref, "courtyard x 2^%d" % k)


def test_a_non_finite_edge_keeps_the_guarded_loop(renderer):
    """One triangle spans the float range: its edge v1 - v0 overflows to infinity, the host finds no bound (0: no lane is safe)
    and the kernel runs the guarded loop on every batch -- the image is still the oracle's.  (One leaf: the builder cannot
    partition a box of infinite extent.)"""
    pos = courtyard()
    big = np.float32(3.0e38)
    pos = np.concatenate([pos, np.float32([[[-big, 6.0, -6.0], [big, 6.0, -6.0], [0.0, 7.0, -6.0]]])])
    sc, osc, pos = courtyard_pair(0, pos, leaf=64)
    assert safe_dir_of(pos) == 0.0 and len(sc.m_BVHNodes) == 1
    img, ref, counted = render_scaled(renderer, sc, osc, 0)
    assert "path_pool" in renderer.kernelInfo(), renderer.kernelInfo()
    assert np.isfinite(ref).all() and counted["hits_flat"] > 500
    compare(img, ref, "courtyard with an infinite edge")


@pytest.mark.parametrize("leaf", [2, 3, 5, 8, 20])
@pytest.mark.parametrize("name", ["cornell_box_gltf", "uv_texture_test"])
def test_unguarded_loop_on_every_leaf_shape(renderer, name, leaf):
    """Leaves of 1, 2, 3, odd and even sizes, in one class or spread over the four T queues: a lane that is through with its
    leaf, or on an odd leaf's last step, tests triangles of the next leaf or the zeroed pad without the guard -- their edges
    are inside the bound too -- and nothing changes.  (The builder's target is an upper
    bound -- a target of 1 it cannot reach on these scenes: cornell's leaves hold 1-2, 1-3, 2-5, 3-8 and 8-18 triangles.)"""
    sc, osc = make_pair(name, leaf=leaf)
    nodes = sc.m_BVHNodes
    sizes = set(nodes["prim_count"][nodes["is_leaf"] != 0].tolist())
    if name == "cornell_box_gltf":
        assert sizes >= {2: {1, 2}, 3: {1, 2, 3}, 5: {3, 4, 5}, 8: {7, 8}, 20: {10, 18}}[leaf], sizes
    cam, ocam = cameras(name)
    s, o = settings_pair(ray_bounce_limit=4)
    renderer.m_RendererSettings = s
    renderer.ResizeBuffer(32, 32)
    renderer.resetAccumulationBuffer()
    renderer.RenderBatch(cam, sc, 2)
    info = renderer.kernelInfo()            # (uv_texture_test has an RGBA texture: the alpha build)
    assert info.startswith("path_pool<lean") and "sun" not in info and "lds-scene" in info, info
    ref, _, _ = oracle.render(osc, ocam, o, 32, 32, 1, 2)
    compare(renderer.GetRenderTargetImage(), ref, "%s, leaves of up to %d" % (name, leaf))


def test_unguarded_loop_on_a_one_leaf_root(renderer):
    """A one-triangle scene (the root is the leaf; the pair's second triangle is the zeroed pad) and a three-triangle one-leaf scene."""
    up = np.tile(np.float32([0, 0, 1]), (3, 1))
    pos = np.float32([[[-1, -1, 0], [1, -1, 0], [0, 1, 0]]])
    sc, osc = _programmatic_pair(pos, up[None], np.zeros((1, 3, 2), np.float32), [0], [((0.8, 0.3, 0.2), -1)], [], 20, 8)
    assert len(sc.m_BVHNodes) == 1
    img, ref = _render_both(renderer, sc, osc, (0.1, 0.0, 2.0), (0, 0, -1), 32, 32, 2, ray_bounce_limit=4)
    compare(img, ref, "one triangle")
    pos3 = np.float32([[[-1, -1, 0], [1, -1, 0], [0, 1, 0]], [[-1, -1, -1], [1, -1, -1], [0, 1, -1]], [[-2, -1, 1], [0, -1, 1], [-1, 1, 1]]])
    sc, osc = _programmatic_pair(pos3, np.repeat(up[None], 3, axis=0), np.zeros((3, 3, 2), np.float32), [0, 0, 0], [((0.8, 0.3, 0.2), -1)], [], 20, 8)
    assert len(sc.m_BVHNodes) == 1
    img, ref = _render_both(renderer, sc, osc, (0.1, 0.0, 3.0), (0, 0, -1), 32, 32, 2, ray_bounce_limit=4)
    compare(img, ref, "three triangles, one leaf")


@pytest.mark.parametrize("name,leaf,kw", [("mc_transparency", 5, dict(ray_bounce_limit=4)), ("mc_transparency", 20, dict(ray_bounce_limit=4)),
                                          ("mc_transparency", 5, dict(ray_bounce_limit=4, enableSunlight=1)),
                                          ("cornell_box_gltf", 3, dict(ray_bounce_limit=4, enableSunlight=1)), ("uv_texture_test", 3, dict(ray_bounce_limit=4, enableSunlight=1))])
def test_alpha_and_sunlight_paths_still_match(renderer, name, leaf, kw):
    """Alpha cut-outs run the unguarded loop too; sunlight builds and the statistics build keep the guarded one.  Production
    build and statistics build, whose counters equal the oracle's.  (mc_transparency under a target of 20 has leaves of ten
    different step counts: all four T queues are in use.)"""
    sc, osc = make_pair(name, leaf=leaf)
    if leaf == 20:
        nodes = sc.m_BVHNodes
        assert len(set(((nodes["prim_count"][nodes["is_leaf"] != 0] + 1) // 2).tolist())) > 4
    cam, ocam = cameras(name)
    s, o = settings_pair(**kw)
    ref, _, cnt = oracle.render(osc, ocam, o, 32, 32, 1, 2, want_counters=True)
    want = cnt.as_dict()
    renderer.m_RendererSettings = s
    renderer.ResizeBuffer(32, 32)
    for counting in (False, True):
        renderer.resetAccumulationBuffer()
        renderer.setCounting(counting)
        try:
            renderer.RenderBatch(cam, sc, 2)
            assert "path_pool" in renderer.kernelInfo(), renderer.kernelInfo()
            compare(renderer.GetRenderTargetImage(), ref, "%s %r counting=%s" % (name, kw, counting))
            if counting:
                got = renderer.getCounters().as_dict()
                for k in ("samples", "rays", "node_visits", "inner_visits", "tri_tests", "hits_textured", "hits_flat", "shadow_rays", "inner_visits_shadow", "tri_tests_shadow"):
                    assert got[k] == want[k], (k, got[k], want[k])
        finally:
            renderer.setCounting(False)


@pytest.fixture(scope="module")
def cornell():
    return make_pair("cornell_box"), cameras("cornell_box")


@pytest.mark.parametrize("spp", [1, 2, 3, 5])
@pytest.mark.parametrize("W,H", [(7, 3), (13, 9), (64, 8), (250, 17)])
def test_sample_id_to_pixel(cornell, W, H, spp):
    """Frames that are no multiple of the 8 x 8 tile (one tile, one tile row, one tile column short), 1-5 frames per launch,
    unsharded and as ranks of a 2- and a 3-way split in 8-row stripes: E's sample id -> (frame, tile, row, stripe) mapping with
    divisors of 1 among n_tiles_all, tiles_x, tiles_y and stripe_rows, against the oracle, and the shards against the rows of
    the unsharded render.  (The cases of the division-free mapping that was measured and not shipped; they hold for
    the mapping as it is.)"""
    (sc, osc), (cam, ocam) = cornell
    s, o = settings_pair(ray_bounce_limit=3)
    ref, _, _ = oracle.render(osc, ocam, o, W, H, 1, spp)
    full = drt.Renderer(0)
    full.m_RendererSettings = s
    full.ResizeBuffer(W, H)
    full.RenderBatch(cam, sc, spp)
    assert "path_pool" in full.kernelInfo(), full.kernelInfo()
    whole = full.GetRenderTargetImage()
    compare(whole, ref, "%dx%d x %d" % (W, H, spp))
    for rank, world in ((0, 2), (1, 2), (2, 3)):
        rows = [y for y in range(H) if (y // 8) % world == rank]
        r = drt.Renderer(0)
        r.m_RendererSettings = s
        r.setShard(8, rank, world)
        r.ResizeBuffer(W, H)
        assert r.getLocalRows() == len(rows)
        if not rows:
            continue
        r.RenderBatch(cam, sc, spp)
        local = r.GetRenderTargetImage()
        assert np.array_equal(bits(local), bits(whole[rows])), (W, H, spp, rank, world)
        assert np.array_equal(bits(local), bits(ref[rows])), (W, H, spp, rank, world)
