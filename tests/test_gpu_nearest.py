"""Nearest-surface queries on the GPU (drt_renderer_nearest, kernel_nearest.hip): every field of every result bit-equal to the
restatement in tests/nearest_ref.py -- over scenes, radii, a tree deeper than the LDS stack, batch shapes, a refitted device copy and
the torch path -- and the renderer's state untouched, and the error codes of include/drt.h."""
import numpy as np
import pytest

import oracle
from tests import nearest_ref as nr
from tests import ray_query_ref as rq
from tests import refit_ref as rf
from tests.scenes import SCENES, scene_path

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ONE_MATERIAL = [((0.8, 0.8, 0.8), -1)]
SINGLE = np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
QUAD = np.float32([[[0, 0, 0], [1, 0, 0], [1, 1, 0]], [[0, 0, 0], [1, 1, 0], [0, 1, 0]]])      # ties on the diagonal
_cache = {}


@pytest.fixture(scope="module")
def renderer():
    return drt.Renderer(0)


def flat_scene(pos):
    n = len(pos)
    nrm = np.tile(np.float32([0, 0, 1]), (n, 3, 1))
    return rq.programmatic_scene(drt, pos, nrm, np.zeros((n, 3, 2), np.float32), np.zeros(n, np.int32), ONE_MATERIAL, [], 20, 8)


def scene_pair(name):
    """(product scene, Geometry of the oracle's scene), both with the editor's tree."""
    if name not in _cache:
        if name in ("single", "quad"):
            sc, osc = flat_scene(SINGLE if name == "single" else QUAD)
        else:
            sc = drt.Scene()
            sc.loadGLTFmodel(scene_path(name))
            b = drt.BVHBuilder()
            b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
            b.buildIterative(sc)
            osc = oracle.Scene.load_glb(scene_path(name)).build_bvh(20, 8)
        _cache[name] = (sc, nr.from_oracle(osc))
    return _cache[name]


def assert_equal(got, ref, what):
    """Bit for bit on every field."""
    assert len(got.d2) == len(ref.d2), what
    for field in nr.Nearest._fields:
        g, r = np.ascontiguousarray(getattr(got, field)), np.ascontiguousarray(getattr(ref, field))
        assert g.shape == r.shape and g.dtype == r.dtype, (what, field, g.shape, r.shape, g.dtype, r.dtype)
        bad = np.nonzero((g.view(np.uint32) != r.view(np.uint32)).reshape(len(g), -1).any(axis=1))[0]
        assert len(bad) == 0, "%s: %s differs on %d of %d points, first %d: %r vs %r" % (what, field, len(bad), len(g), bad[0], g[bad[0]], r[bad[0]])


def assert_all_miss(got, max_dist, what):
    n = len(got.d2)
    assert (got.prim == -1).all(), what
    assert (got.d2.view(np.uint32) == np.full(n, np.float32(max_dist) * np.float32(max_dist), np.float32).view(np.uint32)).all(), what
    for f in (got.point, got.u, got.v, got.side):
        assert (np.ascontiguousarray(f).view(np.uint32) == 0).all(), what


def sweep_points(g, n, seed, nan=True):
    """About n points: on and near surfaces, at vertices and edge midpoints (exact ties), in the scene's box, far outside, and three
    with a NaN coordinate (they visit every node: left out where the restatement would take seconds over that)."""
    rng = np.random.default_rng(seed)
    pts = nr.point_sets(g, n, rng)
    on = nr.surface_points(g, n // 8, rng, offset=0.0)
    bad = np.repeat(pts[:1], 3, axis=0)
    bad[np.arange(3), np.arange(3)] = np.nan
    return np.concatenate([pts, on, bad] if nan else [pts, on]).astype(np.float32)


@pytest.mark.parametrize("name", ["single", "quad", "cornell_box", "suzanne_plane", "cs16_dust"])
def test_scene_sweep_bit_equal_to_the_restatement(renderer, name):
    sc, g = scene_pair(name)
    pts = sweep_points(g, 1800, 11, nan=name != "cs16_dust")
    ref = nr.nearest(g, pts)
    nan = np.isnan(pts).any(axis=1)
    assert (ref.prim[~nan] >= 0).all() and (ref.prim[nan] == -1).all() and (ref.d2 == 0).any()
    assert_equal(renderer.nearest(sc, pts), ref, name + " max_dist inf")
    # a finite radius per point: from a quarter of to twice the distance found, and the distance itself (strict <: a miss)
    rng = np.random.default_rng(5)
    radius = (np.sqrt(ref.d2) * rng.uniform(0.25, 2.0, len(pts)).astype(np.float32)).astype(np.float32)
    radius[::7] = np.sqrt(ref.d2[::7])
    ref_r = nr.nearest(g, pts, radius)
    assert (ref_r.prim >= 0).any() and (ref_r.prim[~nan] < 0).any()
    assert_equal(renderer.nearest(sc, pts, radius), ref_r, name + " per-point radius")
    assert_equal(renderer.nearest(sc, pts, 0.0), nr.nearest(g, pts, 0.0), name + " max_dist 0")
    assert_all_miss(renderer.nearest(sc, pts, 0.0), 0.0, name + " max_dist 0")


def test_quad_diagonal_ties_go_to_the_first_triangle_found(renderer):
    sc, g = scene_pair("quad")
    t = np.linspace(0, 1, 33, dtype=np.float32)
    pts = np.stack([t, t, np.float32(0.5) * np.ones_like(t)], axis=1)
    got, ref = renderer.nearest(sc, pts), nr.nearest(g, pts)
    assert_equal(got, ref, "diagonal")
    assert (got.d2 == 0.25).all() and (got.prim == got.prim[0]).all() and (got.side == 1).all()


def test_an_empty_scene_gives_all_misses(renderer):
    sc = drt.Scene()
    sc.addMaterial(*ONE_MATERIAL[0])
    sc.setGeometry(np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 2), np.float32), np.zeros(0, np.int32))
    drt.BVHBuilder().buildIterative(sc)
    assert len(sc.m_PrimitivesBuffer) == 0
    pts = np.random.default_rng(0).normal(size=(500, 3)).astype(np.float32)
    pts[7, 1] = np.nan
    assert_all_miss(renderer.nearest(sc, pts), np.inf, "empty, inf")
    assert_all_miss(renderer.nearest(sc, pts, 2.5), 2.5, "empty, 2.5")
    assert_equal(renderer.nearest(sc, pts, 2.5), nr.nearest(nr.from_product(sc), pts, 2.5), "empty")


def test_a_tree_deeper_than_the_lds_stack(renderer):
    sc, osc = rq.programmatic_scene(drt, *rq.soup(3000, 5), 2, 8)
    assert sc.bvh_depth > 8                     # levels beyond the 8 in LDS run through the HBM stack
    g = nr.from_oracle(osc)
    rng = np.random.default_rng(3)
    pts = np.concatenate([nr.surface_points(g, 200, rng), nr.box_points(g, 200, rng), nr.box_points(g, 200, rng, 10.0)])
    assert_equal(renderer.nearest(sc, pts), nr.nearest(g, pts), "soup of depth %d" % sc.bvh_depth)
    # a NaN point visits every node: the deepest stack the tree allows
    bad = np.float32([[np.nan, 0, 0]] * 70)
    assert_all_miss(renderer.nearest(sc, bad), np.inf, "NaN points")


@pytest.fixture(scope="module")
def batch():
    sc, g = scene_pair("suzanne_plane")
    pts = sweep_points(g, 1780, 21)[:2000]
    assert len(pts) == 2000
    return sc, pts, nr.nearest(g, pts)


@pytest.mark.parametrize("n", [1, 15, 63, 64, 65, 1000])
def test_small_batches(renderer, batch, n):
    sc, pts, ref = batch
    assert_equal(renderer.nearest(sc, pts[:n]), nr.Nearest(*[f[:n] for f in ref]), "n = %d" % n)
    assert_equal(renderer.nearest(sc, pts[-n:]), nr.Nearest(*[f[-n:] for f in ref]), "last %d" % n)


def _packed(res):
    return torch.cat([res.point, res.d2[:, None], res.prim.view(torch.float32)[:, None], res.u[:, None], res.v[:, None], res.side[:, None]],
                     dim=1).view(torch.int32)


def test_a_batch_beyond_the_grid_a_permutation_and_a_second_run(renderer, batch):
    sc, pts, ref = batch
    tiles = 300                                 # 600 000 points: more than the persistent grid has threads, so lanes are refilled
    assert tiles * len(pts) > torch.cuda.get_device_properties(0).multi_processor_count * 2048
    dev_pts = torch.from_numpy(pts).to(DEV).repeat(tiles, 1)
    got = _packed(renderer.nearest(sc, dev_pts))
    want = np.concatenate([ref.point, ref.d2[:, None], ref.prim.view(np.float32)[:, None], ref.u[:, None], ref.v[:, None], ref.side[:, None]], axis=1)
    want = torch.from_numpy(np.ascontiguousarray(want).view(np.int32)).to(DEV).repeat(tiles, 1)
    bad = (got != want).any(dim=1)
    assert not bad.any(), "%d of %d results differ from the tiled reference, first %d" % (bad.sum(), len(bad), bad.nonzero()[0])
    assert torch.equal(_packed(renderer.nearest(sc, dev_pts)), got)                           # two runs: identical bytes
    perm = torch.from_numpy(np.random.default_rng(2).permutation(len(dev_pts))).to(DEV)
    assert torch.equal(_packed(renderer.nearest(sc, dev_pts[perm])), got[perm])


def _load(name):
    sc = drt.Scene()
    sc.loadGLTFmodel(scene_path(name))
    st = rf.streams(sc.m_PrimitivesBuffer)
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
    b.buildIterative(sc)
    return sc, st


def test_after_a_refit_the_moved_geometry_answers(renderer):
    sc, st = _load("cornell_box")
    moved = (st[0] + np.random.default_rng(1).normal(0, 0.05, st[0].shape)).astype(np.float32)
    host, _ = _load("cornell_box")
    host.refit(moved)                                          # the host scene refitted with the same positions
    g_old, g_new = nr.from_product(sc), nr.from_product(host)
    pts = np.concatenate([sweep_points(g_old, 800, 4), sweep_points(g_new, 800, 5)])
    old, new = nr.nearest(g_old, pts), nr.nearest(g_new, pts)
    assert (old.d2.view(np.uint32) != new.d2.view(np.uint32)).mean() > 0.5
    r = drt.Renderer(0)
    assert_equal(r.nearest(sc, pts), old, "before the refit")
    r.refit(sc, torch.from_numpy(moved).to(DEV))
    assert_equal(r.nearest(sc, pts), new, "after the refit")
    assert_equal(renderer.nearest(sc, pts), old, "a renderer that was not refitted")
    assert_equal(r.nearest(sc, pts), new, "after the other renderer's query")


def test_torch_path_stays_on_the_device_and_orders_with_the_stream(renderer):
    sc, g = scene_pair("cornell_box")
    dev = torch.device(DEV)
    pts = sweep_points(g, 4000, 12)
    ref = nr.nearest(g, pts)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        p = torch.from_numpy(pts).to(dev)
        radius = torch.full((len(pts),), float("inf"), device=dev)
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(2000000)                  # the inputs' producer is still busy when the query is enqueued
        got = renderer.nearest(sc, p * 1.0, radius * 1.0)
        packed = renderer.nearest(sc, torch.cat([p, radius[:, None]], dim=1))
        d2_copy = got.d2.clone()
    assert all(x.device == dev for x in got) and got.prim.dtype == torch.int32 and got.point.shape == (len(pts), 3)
    s.synchronize()
    assert_equal(nr.Nearest(*[x.cpu().numpy() for x in got]), ref, "device tensors")
    assert_equal(nr.Nearest(*[x.cpu().numpy() for x in packed]), ref, "packed [N, 4]")
    assert (d2_copy.cpu().numpy().view(np.uint32) == ref.d2.view(np.uint32)).all()
    assert_equal(renderer.nearest(sc, pts), ref, "numpy")
    assert_equal(renderer.nearest(sc, np.concatenate([pts, np.full((len(pts), 1), 0.75, np.float32)], axis=1)), nr.nearest(g, pts, 0.75), "packed numpy")


def test_queries_leave_the_renderer_alone_and_work_on_a_sharded_one(renderer):
    sc, g = scene_pair("cornell_box")
    _, pos, fwd, depth = SCENES["cornell_box"]
    cam = drt.Camera(pos)
    cam.m_Forward_dir = np.array(fwd, np.float32)
    pts = sweep_points(g, 2000, 6)
    ref = nr.nearest(g, pts)
    images = []
    for with_queries in (False, True):
        r = drt.Renderer(0)
        r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=depth)
        r.ResizeBuffer(96, 64)
        r.Render(cam, sc)
        if with_queries:
            info, frame, accum, n, span = r.kernelInfo(), r.GetRenderTargetImage(), r.GetAccumulationBuffer(), r.getSampleCount(), r.kernelSpanMs()
            assert_equal(r.nearest(sc, pts), ref, "between two renders")
            assert r.kernelInfo() == info and r.getSampleCount() == n and r.kernelSpanMs() == span
            assert r.GetRenderTargetImage().tobytes() == frame.tobytes() and r.GetAccumulationBuffer().tobytes() == accum.tobytes()
        r.Render(cam, sc)
        images.append((r.GetRenderTargetImage(), r.getSampleCount()))
    assert images[0][0].tobytes() == images[1][0].tobytes() and images[0][1] == images[1][1]
    r = drt.Renderer(0)
    r.setShard(8, 1, 2)
    r.ResizeBuffer(96, 64)
    assert_equal(r.nearest(sc, pts), ref, "sharded renderer")


def test_error_paths(renderer):
    sc, g = scene_pair("cornell_box")
    dev = torch.device(DEV)
    pts = torch.zeros((65, 4), dtype=torch.float32, device=dev)
    out = torch.zeros((66, 8), dtype=torch.float32, device=dev)
    L, h = drt._lib, renderer._h
    INV = drt.ERR_INVALID
    assert L.drt_renderer_nearest(h, sc._h, None, out.data_ptr(), 64, None) == INV
    assert L.drt_renderer_nearest(h, sc._h, pts.data_ptr(), None, 64, None) == INV
    assert L.drt_renderer_nearest(None, sc._h, pts.data_ptr(), out.data_ptr(), 64, None) == INV
    assert L.drt_renderer_nearest(h, None, pts.data_ptr(), out.data_ptr(), 64, None) == INV
    assert L.drt_renderer_nearest(h, sc._h, pts.data_ptr() + 4, out.data_ptr(), 64, None) == INV        # misaligned
    assert L.drt_renderer_nearest(h, sc._h, pts.data_ptr(), out.data_ptr() + 8, 64, None) == INV
    host_pts, host_out = np.zeros((64, 4), np.float32), np.zeros((64, 8), np.float32)
    assert L.drt_renderer_nearest(h, sc._h, host_pts.ctypes.data, out.data_ptr(), 64, None) == INV       # host memory
    assert L.drt_renderer_nearest(h, sc._h, pts.data_ptr(), host_out.ctypes.data, 64, None) == INV
    assert L.drt_renderer_nearest(h, sc._h, None, None, 0, None) == drt.OK                               # n == 0: nothing to do
    assert len(renderer.nearest(sc, np.zeros((0, 3), np.float32)).d2) == 0
    torch.cuda.synchronize()
    assert (out == 0).all()                                                                              # nothing was launched
    for bad in (lambda: renderer.nearest(sc, pts.cpu()),                                                 # wrong device
                lambda: renderer.nearest(sc, pts.double()),                                              # wrong dtype
                lambda: renderer.nearest(sc, pts[:, :2]),                                                # wrong shape
                lambda: renderer.nearest(sc, pts[:, :3], pts[:10, 3]),                                   # mismatched counts
                lambda: renderer.nearest(sc, pts[:, :3].cpu().numpy(), pts[:, 3]),                       # numpy mixed with device tensors
                lambda: renderer.nearest(sc, pts, 1.0),                                                  # packed points carry max_dist
                lambda: renderer.nearest(sc, host_pts.astype(np.float64))):
        with pytest.raises(drt.DrtError) as e:
            bad()
        assert e.value.code == INV
    if torch.cuda.device_count() > 1:                                                                    # another device's memory
        other = pts.to("cuda:1")
        assert L.drt_renderer_nearest(h, sc._h, other.data_ptr(), out.data_ptr(), 64, None) == INV
        with pytest.raises(drt.DrtError) as e:
            renderer.nearest(sc, other)
        assert e.value.code == INV
    # a pending asynchronous batch
    r = drt.Renderer(0)
    r.ResizeBuffer(64, 32)
    r.RenderBatchAsync(drt.Camera(SCENES["cornell_box"][1]), sc, 1)
    with pytest.raises(drt.DrtError) as e:
        r.nearest(sc, pts)
    assert e.value.code == INV
    r.Wait()
    r.nearest(sc, pts)
    # a tree deeper than 64 levels: the chain's centroids double per triangle (scaled down so that no area overflows)
    chain = list(rq.degenerate_chain(110))
    chain[0] = (chain[0] * np.float32(2.0 ** -55)).astype(np.float32)
    deep, _ = rq.programmatic_scene(drt, *chain, 1, 2)
    assert deep.bvh_depth > 64
    with pytest.raises(drt.DrtError) as e:
        renderer.nearest(deep, pts)
    assert e.value.code == drt.ERR_UNSUPPORTED
    assert_equal(renderer.nearest(sc, pts[:, :3].cpu().numpy()), nr.nearest(g, pts[:, :3].cpu().numpy()), "after the errors")
