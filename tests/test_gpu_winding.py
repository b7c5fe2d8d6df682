"""Generalised winding numbers on the GPU (drt_renderer_winding_numbers / _winding_inside / _winding_signed_distance,
kernel_winding.hip): every output bit-equal to the restatement in tests/winding_ref.py, the node moments included -- over scenes, beta
in {0, 2, inf}, a tree deeper than the LDS stack, batch shapes, a refitted device copy, the modes and the torch path -- and the
renderer's state untouched, and the error codes of include/drt.h.  (A NaN equals any NaN: the sign of one that arithmetic makes is the
hardware's.)"""
import numpy as np
import pytest

import oracle
from tests import hostile_meshes as hm
from tests import inside_ref as ir
from tests import nearest_ref as nr
from tests import ray_query_ref as rq
from tests import winding_ref as wr
from tests.scenes import SCENES, scene_path

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCENE_NAMES = ["cube", "torus", "open_torus", "cornell_box", "degenerate", "chain"]
BETAS = [0.0, 2.0, np.inf]
_cache, _moments = {}, {}


@pytest.fixture(scope="module")
def renderer():
    return drt.Renderer(0)


def open_torus(seed=17):
    pos = ir.torus()
    keep = np.ones(len(pos), bool)
    keep[np.random.default_rng(seed).choice(len(pos), len(pos) // 10, replace=False)] = False
    return pos[keep]


def scene_pair(name):
    """(product scene, oracle scene) with the same tree: the cube with leaf size 2, the torus and the open torus with 4, cornell_box
    with the editor's tree, the degenerate mesh, ray_query_ref.degenerate_chain(62) with one triangle per leaf (43 levels)."""
    if name not in _cache:
        if name == "cornell_box":
            sc = drt.Scene()
            sc.loadGLTFmodel(scene_path(name))
            b = drt.BVHBuilder()
            b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
            b.buildIterative(sc)
            _cache[name] = (sc, oracle.Scene.load_glb(scene_path(name)).build_bvh(20, 8))
        elif name == "chain":
            chain = list(rq.degenerate_chain(62))                # scaled down so that no product of three lengths overflows
            chain[0] = (chain[0] * np.float32(2.0 ** -31)).astype(np.float32)
            _cache[name] = rq.programmatic_scene(drt, *chain, 1, 2)
        elif name == "degenerate":
            _cache[name] = hm.scene_pair(drt, hm.degenerate())
        else:
            pos, leaf = {"cube": (ir.cube(), 2), "torus": (ir.torus(), 4), "open_torus": (open_torus(), 4)}[name]
            _cache[name] = rq.programmatic_scene(drt, *ir.streams(pos), leaf, 8)
    return _cache[name]


def moments_of(name):
    if name not in _moments:
        _moments[name] = wr.moments(scene_pair(name)[1])
    return _moments[name]


def same(got, ref):
    """Rows in which two arrays hold the same bits, a NaN equal to any NaN."""
    g, r = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert g.shape == r.shape and g.dtype == r.dtype, (g.shape, r.shape, g.dtype, r.dtype)
    eq = g.view(np.uint32) == r.view(np.uint32)
    if g.dtype == np.float32:
        eq |= np.isnan(g) & np.isnan(r)
    return eq.reshape(len(g), -1).all(axis=1)


def assert_same(got, ref, what):
    ok = same(got, ref)
    bad = np.nonzero(~ok)[0]
    assert len(bad) == 0, "%s: %d of %d differ, first %d: %r vs %r" % (what, len(bad), len(ok), bad[0], got[bad[0]], ref[bad[0]])


def assert_fields_same(got, ref, what):
    for field in ref._fields:
        assert_same(getattr(got, field), getattr(ref, field), "%s %s" % (what, field))


def point_set(g, n, seed):
    """About n points for a nearest_ref.Geometry: near and on surfaces, at vertices and edge midpoints (no defined answer, but one
    answer), in the scene's box, in a box four times as large (where whole subtrees are far), and four with a NaN or an infinity."""
    rng = np.random.default_rng(seed)
    pts = np.concatenate([nr.point_sets(g, n // 2, rng), nr.box_points(g, n // 4, rng, 1.2), nr.box_points(g, n // 4, rng, 4.0)])
    bad = np.repeat(pts[:1], 4, axis=0)
    bad[np.arange(3), np.arange(3)] = np.nan
    bad[3, 1] = np.inf
    return np.concatenate([pts[:len(pts) // 2], bad, pts[len(pts) // 2:]]).astype(np.float32)


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_moments_bit_equal_to_the_restatement(renderer, name):
    sc, osc = scene_pair(name)
    got = renderer.debugWindingMoments(sc)
    ref = moments_of(name)[wr.device_order(osc.nodes)]
    assert got.shape == ref.shape and len(ref) == len(osc.nodes)
    assert_same(got, ref, name + " moments")
    assert renderer.debugWindingMoments(sc).tobytes() == got.tobytes()


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_winding_numbers_bit_equal_to_the_restatement(renderer, name):
    sc, osc = scene_pair(name)
    pts = point_set(nr.from_oracle(osc), 480, 13)
    finite = np.isfinite(pts).all(axis=1)
    assert (~finite).sum() == 4
    for beta in BETAS:
        depth, vis = np.zeros(len(pts), np.int64), np.zeros((len(pts), 2), np.int64)
        ref = wr.winding(osc, pts, beta, moments_of(name), visits=vis, depth=depth)
        got = renderer.windingNumbers(sc, pts, beta=beta)
        assert got.dtype == np.float32
        assert_same(got, ref, "%s beta %s" % (name, beta))
        assert np.isnan(got[~finite]).all() and np.isfinite(ref[finite]).all()
        if beta == 0.0:
            assert vis[finite, 0].max() == 1                             # the root's dipole alone
        if beta == np.inf:
            assert (vis[finite, 1] == len(osc.tris)).all()
            if name == "chain":
                assert sc.bvh_depth > 16 and depth.max() > 16            # the levels beyond the 16 in LDS run through the HBM stack
        if beta == 2.0 and name in ("torus", "open_torus"):
            assert 0 < vis[finite, 1].mean() < 0.1 * len(osc.tris)       # the hierarchy at work: a fraction of the triangles
    if name in ("cube", "torus"):
        w = renderer.windingNumbers(sc, pts, beta=np.inf)[finite]
        assert (np.abs(w - 1) < 1e-4).any() and (np.abs(w) < 1e-4).any()
    # packed points: max_dist is ignored; the default beta is 2
    packed = np.concatenate([pts, np.zeros((len(pts), 1), np.float32)], axis=1)
    assert_same(renderer.windingNumbers(sc, packed), wr.winding(osc, pts, 2.0, moments_of(name)), name + " packed")


@pytest.fixture(scope="module")
def batch():
    sc, osc = scene_pair("open_torus")
    pts = point_set(nr.from_oracle(osc), 2400, 21)[:2000]
    assert len(pts) == 2000
    mom = moments_of("open_torus")
    ref = {beta: wr.winding(osc, pts, beta, mom) for beta in (2.0, np.inf)}
    ref["nearest"] = nr.nearest(nr.from_oracle(osc), pts, 0.5)
    return sc, pts, ref


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2000])
def test_batch_sizes(renderer, batch, n):
    sc, pts, ref = batch
    for sl in (slice(0, n), slice(2000 - n, 2000)):
        for beta in (2.0, np.inf):
            assert_same(renderer.windingNumbers(sc, pts[sl], beta=beta), ref[beta][sl], "beta %s %r" % (beta, sl))
        with np.errstate(invalid="ignore"):
            flags = ref[2.0][sl] >= np.float32(0.5)
        assert (renderer.windingInside(sc, pts[sl]) == flags).all()
        want = nr.Nearest(*[f[sl] for f in ref["nearest"]])._replace(side=np.where(flags, np.float32(-1), np.float32(1)).astype(np.float32))
        assert_fields_same(renderer.windingSignedDistance(sc, pts[sl], 0.5), want, "signed %r" % (sl,))


def test_a_batch_beyond_the_grid_a_permutation_and_a_second_run(renderer, batch):
    sc, pts, ref = batch
    tiles = 300                                 # 600 000 points: more than the persistent grid has threads, so lanes are refilled
    assert tiles * len(pts) > torch.cuda.get_device_properties(0).multi_processor_count * 2048
    dev_pts = torch.from_numpy(pts).to(DEV).repeat(tiles, 1)
    perm = torch.from_numpy(np.random.default_rng(2).permutation(len(dev_pts))).to(DEV)
    got = renderer.windingNumbers(sc, dev_pts)
    want = torch.from_numpy(ref[2.0]).to(DEV).repeat(tiles)
    assert got.dtype == torch.float32 and got.device == torch.device(DEV)
    ok = (got.view(torch.int32) == want.view(torch.int32)) | (got.isnan() & want.isnan())
    assert ok.all(), "%d of %d differ from the tiled reference" % ((~ok).sum(), len(ok))
    assert torch.equal(renderer.windingNumbers(sc, dev_pts).view(torch.int32), got.view(torch.int32))          # two runs: identical bytes
    assert torch.equal(renderer.windingNumbers(sc, dev_pts[perm]).view(torch.int32), got[perm].view(torch.int32))
    flags = renderer.windingInside(sc, dev_pts)
    assert flags.dtype == torch.bool and torch.equal(flags, got >= 0.5)
    sd = renderer.windingSignedDistance(sc, dev_pts, 0.5)
    assert torch.equal(sd.side, torch.where(got >= 0.5, -1.0, 1.0).to(torch.float32))
    again = renderer.windingSignedDistance(sc, dev_pts[perm], 0.5)
    assert torch.equal(again.side, sd.side[perm]) and torch.equal(again.prim, sd.prim[perm])


def test_an_empty_scene_answers_zero(renderer):
    sc = drt.Scene()
    sc.addMaterial((0.8, 0.8, 0.8), -1)
    sc.setGeometry(np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 2), np.float32), np.zeros(0, np.int32))
    drt.BVHBuilder().buildIterative(sc)
    pts = np.random.default_rng(0).normal(size=(500, 3)).astype(np.float32)
    pts[7, 1] = np.nan
    for beta in BETAS:
        w = renderer.windingNumbers(sc, pts, beta=beta)
        assert np.isnan(w[7]) and (np.delete(w, 7).view(np.uint32) == 0).all()
    assert not renderer.windingInside(sc, pts).any()
    sd = renderer.windingSignedDistance(sc, pts, 2.5)
    assert_fields_same(sd, nr.nearest(nr.from_product(sc), pts, 2.5)._replace(side=np.ones(500, np.float32)), "empty")


def test_after_a_refit_the_moved_mesh_answers(renderer):
    def load():
        return rq.programmatic_scene(drt, *ir.streams(open_torus()), 4, 8)[0]

    sc, host = load(), load()
    moved = (open_torus() * np.float32([1.25, 0.75, 1.5]) + np.float32([0.125, 0, -0.25])).astype(np.float32)
    host.refit(moved)                                          # the host scene refitted with the same positions
    old, new = ir.product_scene(sc), ir.product_scene(host)
    g_old, g_new = nr.from_product(sc), nr.from_product(host)
    pts = np.concatenate([point_set(g_old, 400, 4), point_set(g_new, 400, 5)])
    m_old, m_new = wr.moments(old), wr.moments(new)
    w_old, w_new = wr.winding(old, pts, 2.0, m_old), wr.winding(new, pts, 2.0, m_new)
    with np.errstate(invalid="ignore"):
        assert ((w_old >= 0.5) != (w_new >= 0.5)).mean() > 0.05
    r = drt.Renderer(0)
    assert_same(r.windingNumbers(sc, pts), w_old, "before the refit")
    assert_same(r.debugWindingMoments(sc), m_old[wr.device_order(old.nodes)], "moments before the refit")
    r.refit(sc, torch.from_numpy(moved).to(DEV))
    assert_same(r.windingNumbers(sc, pts), w_new, "after the refit")
    assert_same(r.debugWindingMoments(sc), m_new[wr.device_order(new.nodes)], "moments after the refit")
    assert_same(r.windingNumbers(sc, pts, beta=np.inf), wr.winding(new, pts, np.inf, m_new), "after the refit, exact")
    assert_fields_same(r.windingSignedDistance(sc, pts), wr.signed_distance(new, pts, g=g_new, mom=m_new), "signed distance after the refit")
    assert_same(renderer.windingNumbers(sc, pts), w_old, "a renderer that was not refitted")
    assert_same(r.windingNumbers(sc, pts), w_new, "after the other renderer's query")


def test_modes_and_the_grid(renderer):
    sc, osc = scene_pair("open_torus")
    mom = moments_of("open_torus")
    g = nr.from_oracle(osc)
    pts = point_set(g, 800, 6)
    w = wr.winding(osc, pts, 2.0, mom)
    near = nr.nearest(g, pts)
    raw = renderer.nearest(sc, pts)
    for thr in (0.5, 0.25, 0.9, -1.0):
        with np.errstate(invalid="ignore"):
            flags = w >= np.float32(thr)
        got = renderer.windingInside(sc, pts, threshold=thr)
        assert got.dtype == np.bool_ and (got == flags).all(), thr
        sd = renderer.windingSignedDistance(sc, pts, threshold=thr)
        assert_fields_same(sd, near._replace(side=np.where(flags, np.float32(-1), np.float32(1)).astype(np.float32)), "threshold %s" % thr)
        for f in ("point", "d2", "prim", "u", "v"):                       # the first seven words are nearest's own output
            assert getattr(sd, f).tobytes() == getattr(raw, f).tobytes(), (thr, f)
    assert (renderer.windingInside(sc, pts) == (renderer.windingNumbers(sc, pts) >= 0.5)).all()
    radius = (np.sqrt(near.d2) * np.random.default_rng(5).uniform(0.25, 2.0, len(pts)).astype(np.float32)).astype(np.float32)
    assert_fields_same(renderer.windingSignedDistance(sc, pts, radius), wr.signed_distance(osc, pts, radius, g=g, mom=mom), "per-point max_dist")
    # the grid: cell centres of the scene's bounds, [Z, Y, X]
    grid = renderer.windingGrid(sc, (5, 4, 3))
    assert grid.device == torch.device(DEV) and grid.dtype == torch.float32 and tuple(grid.shape) == (3, 4, 5)
    lo, hi = np.float32(sc.m_BVHNodes[-1]["bmin"]), np.float32(sc.m_BVHNodes[-1]["bmax"])
    res = (5, 4, 3)
    axes = [float(lo[k]) + (torch.arange(res[k], dtype=torch.float32) + 0.5) * (float(hi[k] - lo[k]) / res[k]) for k in range(3)]
    z, y, x = torch.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    cells = torch.stack([x, y, z], dim=-1).reshape(-1, 3).to(DEV)
    assert torch.equal(grid.reshape(-1).view(torch.int32), renderer.windingNumbers(sc, cells).view(torch.int32))
    assert_same(grid.cpu().numpy().ravel(), wr.winding(osc, cells.cpu().numpy(), 2.0, mom), "grid")
    boxed = renderer.windingGrid(sc, 2, lo=(-0.5, -0.5, -0.5), hi=(1.5, 0.5, 0.5), beta=np.inf).cpu().numpy()
    cells = np.float32([[x, y, z] for z in (-0.25, 0.25) for y in (-0.25, 0.25) for x in (0.0, 1.0)])
    assert boxed.shape == (2, 2, 2)
    assert_same(boxed.ravel(), wr.winding(osc, cells, np.inf, mom), "boxed grid")
    assert (boxed[..., 1] > 0.5).all() and (boxed[..., 0] < 0.5).all()            # x = 1: in the tube; x = 0: in the hole


def test_torch_path_stays_on_the_device_and_orders_with_the_stream(renderer):
    sc, osc = scene_pair("torus")
    mom = moments_of("torus")
    dev = torch.device(DEV)
    pts = point_set(nr.from_oracle(osc), 2400, 12)
    w = wr.winding(osc, pts, 2.0, mom)
    ref = wr.signed_distance(osc, pts, mom=mom)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        p = torch.from_numpy(pts).to(dev)
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(2000000)                  # the inputs' producer is still busy when the queries are enqueued
        got = renderer.windingNumbers(sc, p * 1.0)
        flags = renderer.windingInside(sc, p * 1.0)
        sd = renderer.windingSignedDistance(sc, p * 1.0)
        side_copy = sd.side.clone()
    assert got.device == dev and got.dtype == torch.float32 and flags.dtype == torch.bool and all(x.device == dev for x in sd)
    s.synchronize()
    assert_same(got.cpu().numpy(), w, "device tensors")
    with np.errstate(invalid="ignore"):
        assert (flags.cpu().numpy() == (w >= np.float32(0.5))).all()
    assert_fields_same(nr.Nearest(*[x.cpu().numpy() for x in sd]), ref, "device tensors")
    assert (side_copy.cpu().numpy() == ref.side).all()


def test_queries_leave_the_renderer_alone_and_work_on_a_sharded_one(renderer):
    sc, osc = scene_pair("cornell_box")
    mom = moments_of("cornell_box")
    _, pos, fwd, depth = SCENES["cornell_box"]
    cam = drt.Camera(pos)
    cam.m_Forward_dir = np.array(fwd, np.float32)
    pts = point_set(nr.from_oracle(osc), 800, 6)
    w, sd = wr.winding(osc, pts, 2.0, mom), wr.signed_distance(osc, pts, mom=mom)
    images = []
    for with_queries in (False, True):
        r = drt.Renderer(0)
        r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=depth)
        r.ResizeBuffer(96, 64)
        r.Render(cam, sc)
        if with_queries:
            info, frame, accum, n, span = r.kernelInfo(), r.GetRenderTargetImage(), r.GetAccumulationBuffer(), r.getSampleCount(), r.kernelSpanMs()
            assert_same(r.windingNumbers(sc, pts), w, "between two renders")
            assert_fields_same(r.windingSignedDistance(sc, pts), sd, "between two renders")
            assert r.kernelInfo() == info and r.getSampleCount() == n and r.kernelSpanMs() == span
            assert r.GetRenderTargetImage().tobytes() == frame.tobytes() and r.GetAccumulationBuffer().tobytes() == accum.tobytes()
        r.Render(cam, sc)
        images.append((r.GetRenderTargetImage(), r.getSampleCount()))
    assert images[0][0].tobytes() == images[1][0].tobytes() and images[0][1] == images[1][1]
    r = drt.Renderer(0)
    r.setShard(8, 1, 2)
    r.ResizeBuffer(96, 64)
    assert_same(r.windingNumbers(sc, pts), w, "sharded renderer")
    assert_fields_same(r.windingSignedDistance(sc, pts), sd, "sharded renderer")


def test_error_paths(renderer):
    sc, osc = scene_pair("cornell_box")
    dev = torch.device(DEV)
    pts = torch.zeros((65, 4), dtype=torch.float32, device=dev)
    out = torch.zeros((66, 8), dtype=torch.float32, device=dev)
    L, h = drt._lib, renderer._h
    INV = drt.ERR_INVALID
    host_in, host_out = np.zeros((64, 8), np.float32), np.zeros((64, 8), np.float32)
    calls = {"numbers": (lambda r, s, p, n, beta, o: L.drt_renderer_winding_numbers(r, s, p, n, beta, o, None), 4),
             "inside": (lambda r, s, p, n, beta, o: L.drt_renderer_winding_inside(r, s, p, n, beta, 0.5, o, None), 0),
             "signed_distance": (lambda r, s, p, n, beta, o: L.drt_renderer_winding_signed_distance(r, s, p, n, beta, 0.5, o, None), 16)}
    for what, (fn, align) in calls.items():
        assert fn(h, sc._h, None, 64, 2.0, out.data_ptr()) == INV, what
        assert fn(h, sc._h, pts.data_ptr(), 64, 2.0, None) == INV, what
        assert fn(None, sc._h, pts.data_ptr(), 64, 2.0, out.data_ptr()) == INV, what
        assert fn(h, None, pts.data_ptr(), 64, 2.0, out.data_ptr()) == INV, what
        assert fn(h, sc._h, pts.data_ptr() + 4, 64, 2.0, out.data_ptr()) == INV, what                     # misaligned points
        if align:
            assert fn(h, sc._h, pts.data_ptr(), 64, 2.0, out.data_ptr() + align // 2) == INV, what        # misaligned results
        assert fn(h, sc._h, host_in.ctypes.data, 64, 2.0, out.data_ptr()) == INV, what                    # host memory
        assert fn(h, sc._h, pts.data_ptr(), 64, 2.0, host_out.ctypes.data) == INV, what
        assert fn(h, sc._h, None, 0, 2.0, None) == drt.OK, what                                           # n == 0: nothing to do
        for beta in (-1.0, float("nan"), -float("inf")):
            assert fn(h, sc._h, pts.data_ptr(), 64, beta, out.data_ptr()) == INV, what
            assert b"beta" in L.drt_last_error()
            assert fn(h, sc._h, None, 0, beta, None) == INV, what                                         # also with n == 0
    torch.cuda.synchronize()
    assert (out == 0).all()                                                                               # nothing was launched
    assert L.drt_renderer_winding_inside(h, sc._h, pts.data_ptr(), 64, 2.0, 0.5, out.data_ptr() + 1, None) == drt.OK   # bytes need no alignment
    torch.cuda.synchronize()
    flat = out.view(torch.uint8).view(-1)
    assert flat[0] == 0 and (flat[65:] == 0).all() and (flat[1:65] == flat[1]).all() and flat[1] <= 1     # 64 bytes, one answer each
    assert len(renderer.windingNumbers(sc, np.zeros((0, 3), np.float32))) == 0 and len(renderer.windingInside(sc, np.zeros((0, 3), np.float32))) == 0
    assert len(renderer.windingSignedDistance(sc, np.zeros((0, 3), np.float32)).d2) == 0
    for bad in (lambda: renderer.windingNumbers(sc, pts.cpu()),                                          # wrong device
                lambda: renderer.windingNumbers(sc, pts.double()),                                       # wrong dtype
                lambda: renderer.windingNumbers(sc, pts[:, :2]),                                         # wrong shape
                lambda: renderer.windingNumbers(sc, pts, beta=-0.5),
                lambda: renderer.windingInside(sc, pts, beta=float("nan")),
                lambda: renderer.windingSignedDistance(sc, pts[:, :3], pts[:10, 3]),                     # mismatched counts
                lambda: renderer.windingSignedDistance(sc, pts, 1.0),                                    # packed points carry max_dist
                lambda: renderer.windingSignedDistance(sc, pts, beta="two"),
                lambda: renderer.windingGrid(sc, 0),
                lambda: renderer.windingGrid(sc, 4, beta=-1)):
        with pytest.raises(drt.DrtError) as e:
            bad()
        assert e.value.code == INV
    # a pending asynchronous batch
    r = drt.Renderer(0)
    r.ResizeBuffer(64, 32)
    r.RenderBatchAsync(drt.Camera(SCENES["cornell_box"][1]), sc, 1)
    for call in (lambda: r.windingNumbers(sc, pts), lambda: r.windingInside(sc, pts), lambda: r.windingSignedDistance(sc, pts)):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == INV
    r.Wait()
    r.windingNumbers(sc, pts), r.windingInside(sc, pts), r.windingSignedDistance(sc, pts)
    # a 67-level tree: the chain's centroids double per triangle (scaled down so that no area overflows)
    chain = list(rq.degenerate_chain(110))
    chain[0] = (chain[0] * np.float32(2.0 ** -55)).astype(np.float32)
    deep, _ = rq.programmatic_scene(drt, *chain, 1, 2)
    assert deep.bvh_depth == 67
    for call in (lambda: renderer.windingNumbers(deep, pts), lambda: renderer.windingInside(deep, pts), lambda: renderer.windingSignedDistance(deep, pts)):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == drt.ERR_UNSUPPORTED
    p = pts[:, :3].cpu().numpy()
    assert_same(renderer.windingNumbers(sc, p), wr.winding(osc, p, 2.0, moments_of("cornell_box")), "after the errors")
