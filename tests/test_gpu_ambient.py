"""Ambient occlusion on the GPU (drt_renderer_ambient_occlusion, kernel_ambient.hip; Renderer.ambientOcclusion): every record bit-equal
to the restatement in tests/ambient_ref.py -- over one triangle, the quad, cornell_box, a scene with alpha cut-outs and a tree deeper
than the LDS stack levels; every form of tile (packed, idle lanes, whole, several per point with a partial last one) and point counts
around them; skipped points between live ones, nothing written outside the n records, a second run byte-identical; the tie to
Renderer.occluded; a refitted device copy; the torch path on a side stream and the numpy path; references from traceRays and
sampleSurface; and the error codes of include/drt.h.  tests/test_ambient_ref.py asserts what the restatement is worth."""
import ctypes as C

import numpy as np
import pytest

import oracle
from tests import ambient_ref as ar
from tests import ray_query_ref as rq
from tests import refit_ref as rf
from tests.scenes import SCENES, scene_path

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
SENTINEL = -77
SINGLE = F([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
_cache = {}


@pytest.fixture(scope="module")
def renderer():
    return drt.Renderer(0)


def scene(name):
    """(product scene, oracle scene), made once and left unchanged"""
    if name not in _cache:
        if name == "single":
            _cache[name] = ar.flat_scene(drt, SINGLE)
        elif name == "quad":
            _cache[name] = ar.flat_scene(drt, ar.quad(-1, 1, -1, 1, 0))
        elif name == "room":
            _cache[name] = ar.flat_scene(drt, np.concatenate([ar.box((-1, -1, 0), (1, 1, 2)), ar.box((-0.3, -0.2, 0), (0.2, 0.4, 0.7))]), leaf=4)
        elif name == "chain":
            _cache[name] = rq.programmatic_scene(drt, *rq.degenerate_chain(62), 1, 2)
        else:
            sc = drt.Scene()
            sc.loadGLTFmodel(scene_path(name))
            b = drt.BVHBuilder()
            b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
            b.buildIterative(sc)
            _cache[name] = (sc, oracle.Scene.load_glb(scene_path(name)).build_bvh(20, 8))
    return _cache[name]


def surface_points(osc, n, seed, skip=True):
    """drt_ao_point [n, 8]: points on random triangles with their unit face normals (some flipped), reaches from a fraction of the scene
    to infinity and 0, and -- skipped points between the live ones -- reaches of -1 and NaN."""
    rng = np.random.default_rng(seed)
    p = osc.tris["p"].astype(np.float64)
    k = rng.integers(0, len(p), n)
    b = rng.uniform(0, 1, (n, 2))
    b = np.where(b.sum(axis=1, keepdims=True) > 1, 1 - b, b)
    e1, e2 = p[k, 1] - p[k, 0], p[k, 2] - p[k, 0]
    fn = np.cross(e1, e2)
    fn /= np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-30)
    fn *= np.where(rng.uniform(size=(n, 1)) < 0.3, -1.0, 1.0)
    size = float(np.linalg.norm(p.reshape(-1, 3).max(axis=0) - p.reshape(-1, 3).min(axis=0)))
    pts = np.zeros((n, 8), F)
    pts[:, 0:3] = p[k, 0] + b[:, 0:1] * e1 + b[:, 1:2] * e2
    pts[:, 4:7] = fn
    pts[:, 3] = np.where(rng.uniform(size=n) < 0.5, np.inf, rng.uniform(0.02, 0.6, n) * size)
    pts[:, 7] = 0.001
    kind = rng.integers(0, 12, n)
    pts[kind == 0, 3] = 0
    if skip:
        pts[kind == 1, 3] = -1
        pts[kind == 2, 3] = np.nan
        if n > 8:                                # in any case two skipped points between live ones
            pts[[0, 4, 7, n - 1], 3], pts[5, 3], pts[6, 3] = np.inf, -1, np.nan
    return pts


def restated(osc, pts, samples, seed, first=0):
    return ar.ambient(osc, pts[:, 0:3], pts[:, 4:7], pts[:, 3], pts[:, 7], samples, seed, first)


def run_raw(r, sc, pts, samples, seed, first=0, lead=2, trail=3, flags=0):
    """One call into the middle of a sentinel-filled buffer: the n records as int32 [n, 4], after asserting that the records around them
    are untouched."""
    n = len(pts)
    d_pts = torch.from_numpy(np.ascontiguousarray(pts, F)).to(DEV)
    out = torch.full((lead + n + trail, 4), SENTINEL, dtype=torch.int32, device=DEV)
    params = (C.c_uint32 * 4)(samples, seed, first, flags)
    rc = drt._lib.drt_renderer_ambient_occlusion(r._h, sc._h, d_pts.data_ptr(), n, C.addressof(params), out[lead:].data_ptr(), None)
    assert rc == drt.OK, drt._lib.drt_last_error()
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[:lead] == SENTINEL).all() and (h[lead + n:] == SENTINEL).all()
    return h[lead:lead + n]


def assert_same(got, want, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, "%s: %d of %d records differ, first %d: %r vs %r" % (what, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("name", ["single", "quad", "cornell_box", "mc_transparency", "chain"])
def test_records_are_bit_equal_to_the_restatement(renderer, name):
    sc, osc = scene(name)
    if name == "chain":
        assert sc.bvh_depth > 16                 # more levels than the kernel keeps in LDS
    pts = surface_points(osc, 40, 3)
    if name in ("single", "quad"):               # nothing above a lone face: look at it from points around it as well
        pts[::2, 0:3] += F([0.1, 0.2, -0.7])
    if name == "chain":                          # from in front of the chain, along it: the rays run through many levels
        pts[::2, 0:3], pts[::2, 4:7] = F([-3, 0, 0]), F([1, 0, 0])
    with np.errstate(invalid="ignore"):
        live = pts[:, 3] >= 0
    assert (~live).sum() >= 2 and live[0] and live[-1]
    for samples in (16, 65):
        want = restated(osc, pts, samples, 11, first=5)
        got = run_raw(renderer, sc, pts, samples, 11, first=5)
        assert_same(got, want, "%s S = %d" % (name, samples))
        assert (got[~live] == ar.SKIPPED).all()
        if name not in ("single", "quad"):
            assert 0 < got[live, 0].sum() < samples * live.sum()          # some open, some blocked
        assert_same(run_raw(renderer, sc, pts, samples, 11, first=5), got, "%s S = %d again" % (name, samples))


@pytest.fixture(scope="module")
def room_points():
    sc, osc = scene("room")
    return sc, osc, surface_points(osc, 257, 8)


@pytest.mark.parametrize("samples", [1, 2, 16, 32, 7, 33, 64, 65, 128, 200])
def test_every_form_of_tile(renderer, room_points, samples):
    # packed tiles (1, 2, 16, 32), idle lanes (7, 33), a whole tile (64), atomics with a partial last tile (65, 200) and without (128)
    sc, osc, pts = room_points
    pts = pts[:65]
    want = restated(osc, pts, samples, 2024)
    assert_same(run_raw(renderer, sc, pts, samples, 2024), want, "S = %d" % samples)
    assert 0 < want[want[:, 0] >= 0, 0].sum() < samples * (want[:, 0] >= 0).sum()


@pytest.mark.parametrize("samples", [2, 16, 64, 65])
def test_point_counts_around_the_tiles(renderer, room_points, samples):
    # a record depends on first + its index only, so every shorter batch is a prefix of the longest: in a packed tile the last
    # segments are missing (n = 1, 3, 5 with 4 or 32 points per tile), 63 / 64 / 65 and 257 end in, at and past a workgroup's tiles
    sc, osc, pts = room_points
    want = restated(osc, pts, samples, 7, first=1000)
    for n in (1, 3, 5, 63, 64, 65, 257):
        assert_same(run_raw(renderer, sc, pts[:n], samples, 7, first=1000), want[:n], "S = %d, n = %d" % (samples, n))
    # two halves with `first`, and a permutation point by point
    got = np.concatenate([run_raw(renderer, sc, pts[:100], samples, 7, first=1000), run_raw(renderer, sc, pts[100:], samples, 7, first=1100)])
    assert_same(got, want, "halves")
    for k in (256, 0, 131):
        assert_same(run_raw(renderer, sc, pts[k:k + 1], samples, 7, first=1000 + k), want[k:k + 1], "point %d alone" % k)


def test_open_is_what_occluded_says_of_the_same_rays(renderer):
    sc, osc = scene("cornell_box")
    pts = surface_points(osc, 50, 21, skip=False)
    samples = 33
    o, d, _ = ar.rays(pts[:, 0:3], pts[:, 4:7], pts[:, 7], samples, 4)
    occ = renderer.occluded(sc, np.repeat(o, samples, axis=0), np.ascontiguousarray(d.reshape(-1, 3)), 0.0, np.repeat(pts[:, 3], samples))
    got = run_raw(renderer, sc, pts, samples, 4)
    assert (got[:, 0] == samples - occ.reshape(-1, samples).sum(axis=1)).all()
    assert 0 < got[:, 0].sum() < samples * len(pts)


def test_non_finite_points_and_normals(renderer):
    sc, osc = scene("room")
    pts = surface_points(osc, 24, 5, skip=False)
    pts[:, 3] = np.inf
    pts[1, 0], pts[2, 5], pts[3, 7] = np.nan, np.nan, np.nan          # a NaN in p, in n, in bias
    pts[4, 4:7] = 0                                                     # n = 0: d is the unit-sphere draw itself
    pts[5, 4:7] *= F(1e30)                                              # dot(n + fuzz, n + fuzz) overflows: d = 0
    pts[6, 4:7] = np.inf
    pts[7, 0:3] = np.inf
    for samples in (16, 64, 200):
        want = restated(osc, pts, samples, 6)
        got = run_raw(renderer, sc, pts, samples, 6)
        assert_same(got, want, "S = %d" % samples)
        assert (got[[1, 2, 3], 0] == samples).all()                    # a NaN hits nothing: all open
        assert (got[2, 1:4] == 0).all()                                 # ... and a NaN direction adds 0 to bent


def test_after_a_refit_the_moved_mesh_answers():
    name = "cornell_box"
    sc = drt.Scene()
    sc.loadGLTFmodel(scene_path(name))
    st = rf.streams(sc.m_PrimitivesBuffer)
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
    b.buildIterative(sc)
    osc0 = oracle.Scene.load_glb(scene_path(name))
    mats = [(tuple(m["albedo"]), int(m["albedo_tex"])) for m in osc0.mats[:osc0.n_mats]]
    before = osc0.build_bvh(20, 8)
    moved_pos = (st[0] * F(0.8) + np.random.default_rng(3).normal(0, 0.03, st[0].shape)).astype(F)
    order = sc.triangleOrder()
    moved = oracle.Scene(rf.triangles(moved_pos, st[1], st[2], st[3], order=order), mats, osc0.textures)
    moved.nodes = rf.oracle_tree(rf.nodes(sc.m_BVHNodes, moved_pos[order]))
    ra, rb = drt.Renderer(0), drt.Renderer(0)
    pts = surface_points(before, 40, 13)
    want_before, want_moved = restated(before, pts, 32, 9), restated(moved, pts, 32, 9)
    assert (want_before != want_moved).any()
    assert_same(run_raw(ra, sc, pts, 32, 9), want_before, "before the refit")
    ra.refit(sc, torch.from_numpy(moved_pos).to(DEV))
    assert_same(run_raw(ra, sc, pts, 32, 9), want_moved, "after the refit")
    assert_same(run_raw(rb, sc, pts, 32, 9), want_before, "the second renderer's copy did not move")


def test_the_torch_path_on_a_side_stream_and_the_numpy_path(renderer):
    sc, osc = scene("room")
    pts = surface_points(osc, 96, 17)
    want = restated(osc, pts, 16, 3, first=40)
    shaped = pts.reshape(4, 24, 8)
    dev = torch.device(DEV)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        d_pts = torch.from_numpy(shaped).to(dev)
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(2000000)                  # the inputs' producer is still busy when the query is enqueued
        res = renderer.ambientOcclusion(sc, points=d_pts[..., 0:3] * 1.0, normals=d_pts[..., 4:7] * 1.0, samples=16, max_dist=d_pts[..., 3] * 1.0,
                                        bias=d_pts[..., 7] * 1.0, seed=3, first=40)
        total = res.open.clone()
    assert isinstance(res, drt.AmbientOcclusion) and all(x.device == dev for x in res)
    assert res.open.shape == (4, 24) and res.visibility.shape == (4, 24) and res.bent.shape == (4, 24, 3) and res.sums.shape == (4, 24, 3)
    assert res.open.dtype == torch.int32 and res.sums.dtype == torch.int32 and res.visibility.dtype == torch.float32
    s.synchronize()
    assert (total.cpu().numpy().reshape(-1) == want[:, 0]).all()
    assert (res.sums.cpu().numpy().reshape(-1, 3) == want[:, 1:4]).all()
    # numpy in, numpy out; scalars for max_dist and bias; side = -1 is the flipped normals
    got = renderer.ambientOcclusion(sc, points=pts[:, 0:3].copy(), normals=pts[:, 4:7].copy(), samples=16, max_dist=pts[:, 3].copy(), bias=0.001, seed=3, first=40)
    assert all(isinstance(x, np.ndarray) for x in got) and (got.open == want[:, 0]).all() and (got.sums == want[:, 1:4]).all()
    skipped = want[:, 0] < 0
    assert skipped.any() and np.isnan(got.visibility[skipped]).all() and (got.bent[skipped] == 0).all()
    # (the two convenience fields are float32 quotients of the exact record: a rounding or two of the device's division apart)
    assert np.allclose(got.visibility[~skipped], want[~skipped, 0] / 16.0, rtol=1e-6, atol=0)
    assert np.allclose(got.bent[~skipped], want[~skipped, 1:4] / (65536.0 * np.maximum(want[~skipped, 0], 1))[:, None], rtol=1e-6, atol=1e-9)
    flipped = renderer.ambientOcclusion(sc, points=pts[:, 0:3].copy(), normals=pts[:, 4:7].copy(), samples=16, max_dist=0.8, seed=3, side=-1.0)
    want_flipped = ar.ambient(osc, pts[:, 0:3], -pts[:, 4:7], F(0.8), F(0.001), 16, 3)
    assert (flipped.open == want_flipped[:, 0]).all() and (flipped.sums == want_flipped[:, 1:4]).all()
    per_point = np.where(np.arange(96) % 2 == 0, F(1), F(-1)).astype(F)
    mixed = renderer.ambientOcclusion(sc, points=pts[:, 0:3].copy(), normals=pts[:, 4:7].copy(), samples=16, max_dist=0.8, seed=3, side=per_point)
    assert (mixed.open[::2] == ar.ambient(osc, pts[:, 0:3], pts[:, 4:7], F(0.8), F(0.001), 16, 3)[::2, 0]).all()
    assert (mixed.open[1::2] == want_flipped[1::2, 0]).all()
    empty = renderer.ambientOcclusion(sc, points=pts[:0, 0:3].copy(), normals=pts[:0, 4:7].copy())
    assert empty.open.shape == (0,) and empty.bent.shape == (0, 3)


def test_references_from_trace_rays_with_facing_and_from_sample_surface(renderer):
    sc, osc = scene("cornell_box")
    _, pos, fwd, _ = SCENES["cornell_box"]
    org, dirs = rq.camera_rays(oracle.default_camera(position=pos, forward=fwd), 16, 9)
    org[::7], dirs[::7] = F([100, 100, 100]), F([1, 0, 0])                # some from outside, looking away: misses
    hits = renderer.traceRays(sc, org, dirs)
    assert (hits.prim < 0).any() and (hits.prim >= 0).sum() > 60
    got = renderer.ambientOcclusion(sc, hits, samples=32, max_dist=1.5, seed=8, facing=dirs)
    surf = renderer.surface(sc, hits)
    against = ((surf.normal[:, 0] * dirs[:, 0] + surf.normal[:, 1] * dirs[:, 1]) + surf.normal[:, 2] * dirs[:, 2]) > 0
    nrm = np.where(against[:, None], -surf.normal, surf.normal).astype(F)
    reach = np.where(hits.prim < 0, F(-1), F(1.5)).astype(F)
    want = ar.ambient(osc, surf.position, nrm, reach, F(0.001), 32, 8)
    assert (got.open == want[:, 0]).all() and (got.sums == want[:, 1:4]).all()
    assert (got.open[hits.prim < 0] == -1).all() and against.any() and not against.all()
    # a bake: points drawn by area, their face normals as stored
    smp = renderer.sampleSurface(sc, 48, seed=5)
    baked = renderer.ambientOcclusion(sc, smp, samples=64, seed=1)
    surf = renderer.surface(sc, smp)
    want = ar.ambient(osc, surf.position, surf.normal, F(np.inf), F(0.001), 64, 1)
    assert (baked.open == want[:, 0]).all() and (baked.sums == want[:, 1:4]).all() and baked.open.shape == (48,)
    # device tensors in, device tensors out
    smp_t = renderer.sampleSurface(sc, 48, seed=5, as_torch=True)
    baked_t = renderer.ambientOcclusion(sc, smp_t, samples=64, seed=1)
    assert baked_t.open.is_cuda and (baked_t.open.cpu().numpy() == want[:, 0]).all()


def test_an_empty_scene_is_all_open(renderer):
    sc = drt.Scene()
    sc.addMaterial((0.8, 0.8, 0.8), -1)
    sc.setGeometry(np.zeros((0, 3, 3), F), np.zeros((0, 3, 3), F), np.zeros((0, 3, 2), F), np.zeros(0, np.int32))
    drt.BVHBuilder().buildIterative(sc)
    _, osc = scene("room")
    pts = surface_points(osc, 30, 2)
    for samples in (16, 100):
        got = run_raw(renderer, sc, pts, samples, 1)
        live = pts[:, 3] >= 0
        assert (got[live, 0] == samples).all() and (got[~live] == ar.SKIPPED).all()
        _, d, _ = ar.rays(pts[:, 0:3], pts[:, 4:7], pts[:, 7], samples, 1)
        assert (got[live, 1:4] == ar.bent_terms(d).sum(axis=1)[live]).all()


def test_the_frame_state_is_left_alone():
    sc, osc = scene("cornell_box")
    _, pos, fwd, depth = SCENES["cornell_box"]
    cam = drt.Camera(pos)
    cam.m_Forward_dir = np.array(fwd, F)
    pts = surface_points(osc, 64, 4)
    images = []
    for with_queries in (False, True):
        r = drt.Renderer(0)
        r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=depth)
        r.ResizeBuffer(96, 64)
        r.Render(cam, sc)
        info = r.kernelInfo()
        if with_queries:
            run_raw(r, sc, pts, 16, 1)
            run_raw(r, sc, pts, 100, 1)
            assert r.kernelInfo() == info
        n = r.getSampleCount()
        r.Render(cam, sc)
        images.append((r.GetRenderTargetImage(), n, r.getSampleCount()))
    assert (images[0][0].view(np.uint32) == images[1][0].view(np.uint32)).all()
    assert images[0][1:] == images[1][1:]


def test_error_paths(renderer):
    sc, osc = scene("cornell_box")
    pts = surface_points(osc, 64, 4)
    want = restated(osc, pts, 16, 1)
    d_pts = torch.from_numpy(pts).to(DEV)
    out = torch.full((65, 4), SENTINEL, dtype=torch.int32, device=DEV)
    L, h = drt._lib, renderer._h
    ao = L.drt_renderer_ambient_occlusion

    def params(samples=16, seed=1, first=0, flags=0):
        return (C.c_uint32 * 4)(samples, seed, first, flags)

    ok, none, many, flagged, late = params(), params(samples=0), params(samples=4097), params(flags=2), params(first=2 ** 32 - 63)
    P, O = d_pts.data_ptr(), out.data_ptr()
    for args in ((h, sc._h, None, 64, ok, O), (h, sc._h, P, 64, ok, None), (None, sc._h, P, 64, ok, O), (h, None, P, 64, ok, O),
                 (h, sc._h, P, 64, None, O), (h, sc._h, P + 4, 63, ok, O), (h, sc._h, P, 64, ok, O + 8), (h, sc._h, P, 64, none, O),
                 (h, sc._h, P, 64, many, O), (h, sc._h, P, 64, flagged, O), (h, sc._h, P, 64, late, O), (h, sc._h, pts.ctypes.data, 64, ok, O)):
        assert ao(*args, None) == drt.ERR_INVALID, args
    assert ao(h, sc._h, None, 0, ok, None, None) == drt.OK                        # n == 0: nothing to do
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()                                               # no refused call wrote anything
    # a scene without a BVH
    bare = drt.Scene()
    bare.addMaterial((0.8, 0.8, 0.8), -1)
    bare.setGeometry(SINGLE, np.zeros((1, 3, 3), F), np.zeros((1, 3, 2), F), np.zeros(1, np.int32))
    with pytest.raises(drt.DrtError) as e:
        renderer.ambientOcclusion(bare, points=pts[:, 0:3].copy(), normals=pts[:, 4:7].copy())
    assert e.value.code == drt.ERR_INVALID and "BVH" in str(e.value)
    # wrong device, a mix of numpy and tensors
    for bad in (lambda: renderer.ambientOcclusion(sc, points=d_pts[:, 0:3].cpu(), normals=d_pts[:, 4:7].cpu()),
                lambda: renderer.ambientOcclusion(sc, points=d_pts[:, 0:3], normals=pts[:, 4:7].copy()),
                lambda: renderer.ambientOcclusion(sc, points=d_pts[:, 0:3].double(), normals=d_pts[:, 4:7])):
        with pytest.raises(drt.DrtError) as e:
            bad()
        assert e.value.code == drt.ERR_INVALID
    # a pending asynchronous batch
    _, pos, fwd, _ = SCENES["cornell_box"]
    cam = drt.Camera(pos)
    r = drt.Renderer(0)
    r.ResizeBuffer(64, 32)
    r.RenderBatchAsync(cam, sc, 1)
    with pytest.raises(drt.DrtError) as e:
        r.ambientOcclusion(sc, points=d_pts[:, 0:3], normals=d_pts[:, 4:7])
    assert e.value.code == drt.ERR_INVALID and "pending" in str(e.value)
    r.Wait()
    assert (r.ambientOcclusion(sc, points=d_pts[:, 0:3], normals=d_pts[:, 4:7], samples=16, max_dist=d_pts[:, 3], seed=1).open.cpu().numpy() == want[:, 0]).all()
    # a tree deeper than 64 levels: refused as the traversing queries refuse it
    chain = list(rq.degenerate_chain(110))
    chain[0] = (chain[0] * F(2.0 ** -55)).astype(F)
    deep, _ = rq.programmatic_scene(drt, *chain, 1, 2)
    assert deep.bvh_depth > 64
    with pytest.raises(drt.DrtError) as e:
        renderer.ambientOcclusion(deep, points=pts[:, 0:3].copy(), normals=pts[:, 4:7].copy())
    assert e.value.code == drt.ERR_UNSUPPORTED
    assert_same(run_raw(renderer, sc, pts, 16, 1), want, "after the errors")


def test_the_counting_build_gives_the_same_records(renderer):
    sc, osc = scene("room")
    pts = surface_points(osc, 65, 8)
    want = restated(osc, pts, 33, 2)
    counts = (C.c_uint64 * 2)()
    assert drt._lib.drt_debug_ambient_stats(renderer._h, 1, None) == drt.OK
    try:
        assert_same(run_raw(renderer, sc, pts, 33, 2), want, "counting build")
        assert drt._lib.drt_debug_ambient_stats(renderer._h, 0, C.addressof(counts)) == drt.OK
    finally:
        drt._lib.drt_debug_ambient_stats(renderer._h, 0, None)
    trips, steps = int(counts[0]), int(counts[1])
    assert 0 < steps <= 64 * trips
    assert_same(run_raw(renderer, sc, pts, 33, 2), want, "plain build")
