"""Surface lookups and area-weighted sampling on the GPU (drt_renderer_surface_lookup / _surface_weights / _sample_surface,
kernel_surface.hip; Renderer.surface / surfaceWeights / sampleSurface): every word of every record bit-equal to the restatement in
tests/surface_ref.py -- over one triangle, the quad, cornell_box, the two textured test scenes and a scene with a material of every
kind; references from traceRays and nearest and hostile ones; the tie to the renderer's own guide pass; batch shapes; a refitted device
copy; the scan at its block edges; the torch and the numpy path, a sharded renderer, an empty scene -- nothing written outside the n
records, the renderer's state untouched, and the error codes of include/drt.h.  tests/test_surface_ref.py asserts what the
restatement is worth."""
import numpy as np
import pytest

from tests import ray_query_ref as rq
from tests import surface_ref as sr
from tests.scenes import SCENES, scene_path

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -77.0
F = np.float32
B = drt.SURFACE_SCAN_BLOCK
SINGLE = np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
QUAD = np.float32([[[0, 0, 0], [1, 0, 0], [1, 1, 0]], [[0, 0, 0], [1, 1, 0], [0, 1, 0]]])
SCENE_NAMES = ["single", "quad", "cornell_box", "uv_texture_test", "mc_transparency", "materials"]
_cache = {}


@pytest.fixture(scope="module")
def renderer():
    return drt.Renderer(0)


def flat_scene(pos, leaf=2):
    n = len(pos)
    return sr.product_scene(drt, pos, np.tile(np.float32([0, 0, 1]), (n, 3, 1)), np.zeros((n, 3, 2), F), np.zeros(n, np.int32),
                            [dict(albedo=(0.8, 0.7, 0.6))], [], leaf=leaf)


def scene(name):
    """(product scene, the restatement's view of it), made once and left unchanged"""
    if name not in _cache:
        if name in ("single", "quad"):
            sc = flat_scene(SINGLE if name == "single" else QUAD)
        elif name == "materials":
            sc = sr.product_scene(drt, *sr.every_material(210, 3))
        else:
            sc = drt.Scene()
            sc.loadGLTFmodel(scene_path(name))
            b = drt.BVHBuilder()
            b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
            b.buildIterative(sc)
        _cache[name] = (sc, sr.from_product(sc))
    return _cache[name]


def pack_refs(prim, u, v):
    refs = np.zeros((len(prim), 4), F)
    refs.view(np.int32)[:, 1], refs[:, 2], refs[:, 3] = prim, u, v
    refs[:, 0] = np.arange(len(prim))                                                # t is not read
    return refs


def run_raw(r, sc, prim, u, v, normals=None, lead=2, trail=3):
    """One call into the middle of a sentinel-filled buffer: the n records as uint32 [n, 24], after asserting that the records around
    them are untouched."""
    n = len(prim)
    refs = torch.from_numpy(pack_refs(prim, u, v)).to(DEV)
    nrm = None if normals is None else torch.from_numpy(np.ascontiguousarray(normals, F)).to(DEV)
    out = torch.full((lead + n + trail, 24), SENTINEL, dtype=torch.float32, device=DEV)
    rc = drt._lib.drt_renderer_surface_lookup(r._h, sc._h, refs.data_ptr(), None if nrm is None else nrm.data_ptr(), out[lead:].data_ptr(), n, None)
    assert rc == drt.OK, drt._lib.drt_last_error()
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[:lead] == SENTINEL).all() and (h[lead + n:] == SENTINEL).all()
    return h[lead:lead + n].view(np.uint32)


def records(res):
    """A Surface of the Python interface (numpy) as records uint32 [N, 24]"""
    n = res.material.size
    out = np.zeros((n, 24), np.uint32)
    f = out.view(F)
    f[:, sr.POSITION], f[:, sr.NORMAL], f[:, sr.SHADING] = res.position.reshape(n, 3), res.normal.reshape(n, 3), res.shading.reshape(n, 3)
    f[:, sr.ALBEDO], f[:, sr.EMISSIVE], f[:, sr.UV] = res.albedo.reshape(n, 3), res.emissive.reshape(n, 3), res.uv.reshape(n, 2)
    f[:, sr.ALPHA], f[:, sr.ROUGHNESS], f[:, sr.REFRACTIVE_INDEX] = res.alpha.reshape(n), res.roughness.reshape(n), res.refractive_index.reshape(n)
    i = out.view(np.int32)
    i[:, sr.MATERIAL], i[:, sr.LOAD_INDEX], i[:, sr.TEXTURE] = res.material.reshape(n), res.load_index.reshape(n), res.texture.reshape(n)
    out[:, sr.FLAGS] = res.metallic.reshape(n).astype(np.uint32) | (res.transmission.reshape(n).astype(np.uint32) << 1)
    return out


def query_refs(r, sc, s, n, seed):
    """(prim, u, v) of n rays' closest hits and n points' nearest triangles, as the queries return them (misses included)"""
    rng = np.random.default_rng(seed)
    corners = np.concatenate([s.v0, s.v0 + s.e1, s.v0 + s.e2])
    lo, hi = corners.min(axis=0), corners.max(axis=0)
    size = max(float((hi - lo).max()), 1.0)
    k = rng.integers(0, len(s.v0), n)
    b = rng.uniform(0, 1, (n, 2)).astype(F)
    b = np.where(b.sum(axis=1, keepdims=True) > 1, 1 - b, b).astype(F)
    target = s.v0[k] + b[:, 0:1] * s.e1[k] + b[:, 1:2] * s.e2[k]
    org = (rng.uniform(-1, 2, (n, 3)) * (hi - lo + 0.5) + lo).astype(F)
    d = (target - org).astype(F)
    d[::9] = rng.normal(size=d[::9].shape)                                               # some that may miss
    hits = r.traceRays(sc, org, d)
    pts = (target + rng.normal(size=(n, 3)) * 0.05 * size).astype(F)
    near = r.nearest(sc, pts, 0.1 * size)
    return (np.concatenate([hits.prim, near.prim]), np.concatenate([hits.u, near.u]), np.concatenate([hits.v, near.v])), hits, near


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_lookups_are_bit_equal_to_the_restatement(renderer, name):
    sc, s = scene(name)
    (prim, u, v), hits, near = query_refs(renderer, sc, s, 150, 3)
    assert (prim >= 0).sum() > 100
    hp, hu, hv = sr.hostile_refs(len(s.v0), 120, 8)
    prim, u, v = np.concatenate([prim, hp]), np.concatenate([u, hu]), np.concatenate([v, hv])
    want = sr.lookup(s, prim, u, v)
    assert sr.same(run_raw(renderer, sc, prim, u, v), want)
    assert (want[prim < 0] == sr.MISS).all() and (want[prim >= len(s.v0)] == sr.MISS).all()
    # the Python interface on the queries' results as they stand, numpy in, numpy out
    for res, sl in ((hits, slice(0, 150)), (near, slice(150, 300))):
        got = renderer.surface(sc, res)
        assert isinstance(got, drt.Surface) and got.position.shape == (150, 3) and got.uv.shape == (150, 2) and got.material.dtype == np.int32
        assert got.metallic.dtype == np.bool_ and sr.same(records(got), want[sl])
    # ... and with a caller's normals in load order
    nrm = np.random.default_rng(5).normal(size=(len(s.v0), 3, 3)).astype(F)
    assert sr.same(run_raw(renderer, sc, prim, u, v, normals=nrm), sr.lookup(s, prim, u, v, normals=nrm))
    assert sr.same(records(renderer.surface(sc, prim, u, v, normals=nrm)), sr.lookup(s, prim, u, v, normals=nrm))


@pytest.mark.parametrize("name", ["uv_texture_test", "mc_transparency"])
def test_albedo_and_normal_are_the_guide_pass_s(name):
    sc, s = scene(name)
    _, pos, fwd, _ = SCENES[name]
    cam = drt.Camera(pos)
    cam.m_Forward_dir = np.array(fwd, F)
    r = drt.Renderer(0)
    r.ResizeBuffer(64, 36)
    g = r.renderGuides(cam, sc, 1)
    rays = r.cameraRays(cam, 64, 36, 1)[0]
    h = r.traceRays(sc, np.ascontiguousarray(rays[..., 0:3].reshape(-1, 3)), np.ascontiguousarray(rays[..., 4:7].reshape(-1, 3)))
    surf = r.surface(sc, h)
    gp = g.prim.reshape(-1)
    on = gp >= 0
    assert on.sum() > 200 and (h.prim == gp).all()
    assert (surf.albedo.view(np.uint32)[on] == g.albedo.reshape(-1, 3).view(np.uint32)[on]).all()
    gn = g.normal.reshape(-1, 3)[on]
    sn = surf.normal[on]
    assert ((sn == gn).all(axis=1) | (sn == -gn).all(axis=1)).all()
    assert (surf.material[~on] == -1).all() and (surf.texture[on] >= 0).any()


@pytest.fixture(scope="module")
def batch(renderer):
    """5 140 references on the scene with every material (hostile ones among them) and the restatement's records, made once"""
    sc, s = scene("materials")
    prim, u, v = sr.hostile_refs(len(s.v0), 5140, 21)
    return sc, s, prim, u, v, sr.lookup(s, prim, u, v)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5140])
def test_batch_sizes_permutations_and_repeats(renderer, batch, n):
    sc, s, prim, u, v, want = batch
    for sl in (slice(0, n), slice(5140 - n, 5140)):
        got = run_raw(renderer, sc, prim[sl], u[sl], v[sl])
        assert sr.same(got, want[sl])
        assert run_raw(renderer, sc, prim[sl], u[sl], v[sl]).tobytes() == got.tobytes()           # a second run: the same bytes
    perm = np.random.default_rng(n).permutation(n)
    assert sr.same(run_raw(renderer, sc, prim[:n][perm], u[:n][perm], v[:n][perm]), want[:n][perm])


def test_a_refitted_device_copy(batch):
    sc, s, prim, u, v, want = batch
    ra, rb = drt.Renderer(0), drt.Renderer(0)
    rng = np.random.default_rng(12)
    tris = sc.m_PrimitivesBuffer
    order = s.order
    pos = np.zeros((len(order), 3, 3), F)
    pos[order] = tris["vertex"]["position"]                                                # load order
    pos2 = (pos * F(1.5) + rng.uniform(-0.2, 0.2, pos.shape)).astype(F)
    nrm2 = rng.normal(size=pos.shape).astype(F)
    assert sr.same(run_raw(ra, sc, prim, u, v), want)                                        # before: the host scene
    ra.refit(sc, pos2, nrm2)
    hot = ra.debugReadDeviceScene(sc)[1]
    moved = sr.from_product(sc, hot=hot)
    p = pos2[order]
    assert (moved.v0 == p[:, 0]).all() and (moved.e1 == p[:, 1] - p[:, 0]).all() and (moved.e2 == p[:, 2] - p[:, 0]).all()
    assert sr.same(run_raw(ra, sc, prim, u, v), sr.lookup(moved, prim, u, v))               # position, normal: the device copy; shading: the host's
    assert not sr.same(sr.lookup(moved, prim, u, v), want)
    assert sr.same(run_raw(ra, sc, prim, u, v, normals=nrm2), sr.lookup(moved, prim, u, v, normals=nrm2))
    assert sr.same(run_raw(rb, sc, prim, u, v), want)                                        # the second renderer's copy did not move
    cdf = sr.weights(moved)
    assert [int(x) for x in ra.surfaceWeights(sc)] == cdf and cdf != sr.weights(s)
    assert [int(x) for x in rb.surfaceWeights(sc)] == sr.weights(s)
    smp = ra.sampleSurface(sc, 700, seed=5)
    ref = sr.sample(moved, 5, 0, 700, cdf)
    assert (smp.prim == ref.view(np.int32)[:, 1]).all() and (smp.u == ref[:, 2]).all() and (smp.v == ref[:, 3]).all()
    # the point cloud of the mesh as it stands on the device
    pts = ra.surface(sc, smp).position
    assert sr.same(records(ra.surface(sc, smp)), sr.lookup(moved, smp.prim, smp.u, smp.v)) and pts.shape == (700, 3)


def soup_positions(n, seed):
    rng = np.random.default_rng(seed)
    p = (rng.uniform(-4, 4, (n, 1, 3)) + rng.uniform(-0.5, 0.5, (n, 3, 3)) * rng.uniform(0.01, 1, (n, 1, 1))).astype(F)
    p[2::11, 2] = p[2::11, 1]                                                             # zero-area ones
    return p


@pytest.mark.parametrize("n_tris", [1, B - 1, B, B + 1, 2 * B + 1, B * B + 1])
def test_weights_at_the_scan_s_block_edges(renderer, n_tris):
    """B * B + 1 triangles: the pass over the block totals takes a second trip of its loop."""
    sc = flat_scene(soup_positions(n_tris, n_tris), leaf=8)
    s = sr.from_product(sc)
    want = sr.weights(s)
    got = renderer.surfaceWeights(sc)
    assert got.dtype == np.uint64 and got.shape == (n_tris,) and [int(x) for x in got] == want
    assert want[-1] > 0 and (np.diff(np.array(want, np.float64)) >= 0).all()
    dev = renderer.surfaceWeights(sc, as_torch=True)
    assert dev.dtype == torch.int64 and dev.device == torch.device(DEV) and dev.cpu().numpy().view(np.uint64).tobytes() == got.tobytes()
    smp = renderer.sampleSurface(sc, 300, seed=n_tris)
    ref = sr.sample(s, n_tris, 0, 300, want)
    assert (smp.prim == ref.view(np.int32)[:, 1]).all() and (smp.u == ref[:, 2]).all() and (smp.v == ref[:, 3]).all()


@pytest.mark.parametrize("n", [1, 64, 65, 5140])
def test_samples_are_bit_equal_to_the_restatement(renderer, n):
    sc, s = scene("materials")
    cdf = sr.weights(s)
    for seed in (7, 0xDEADBEEF):
        for first in (0, 2 ** 32 - n):
            want = sr.sample(s, seed, first, n, cdf)
            out = torch.full((2 + n + 3, 4), SENTINEL, dtype=torch.float32, device=DEV)
            assert drt._lib.drt_renderer_sample_surface(renderer._h, sc._h, seed, first, out[2:].data_ptr(), n, None) == drt.OK
            torch.cuda.synchronize()
            h = out.cpu().numpy()
            assert (h[:2] == SENTINEL).all() and (h[2 + n:] == SENTINEL).all() and h[2:2 + n].tobytes() == want.tobytes()
    smp = renderer.sampleSurface(sc, n, seed=7)
    want = sr.sample(s, 7, 0, n, cdf)
    assert isinstance(smp, drt.SurfaceSamples) and smp.prim.dtype == np.int32 and (smp.prim == want.view(np.int32)[:, 1]).all()
    assert (smp.u == want[:, 2]).all() and (smp.v == want[:, 3]).all()
    if n > 1:                                                                              # a batch split in two with first=
        k = n // 3
        a, b = renderer.sampleSurface(sc, k, seed=7), renderer.sampleSurface(sc, n - k, seed=7, first=k)
        for x, y, z in zip(a, b, smp):
            assert (np.concatenate([x, y]) == z).all()
    surf = renderer.surface(sc, smp)
    assert (surf.material >= 0).all() and sr.same(records(surf), sr.lookup(s, smp.prim, smp.u, smp.v))


def test_torch_path_stays_on_the_device_and_orders_with_the_stream(renderer, batch):
    sc, s, prim, u, v, want = batch
    dev = torch.device(DEV)
    st = torch.cuda.Stream(device=dev)
    cdf = sr.weights(s)
    with torch.cuda.stream(st):
        dp, du, dv = torch.from_numpy(prim).to(dev), torch.from_numpy(u).to(dev), torch.from_numpy(v).to(dev)
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(2000000)                  # the inputs' producer is still busy when the lookups are enqueued
        res = renderer.surface(sc, dp + 0, du * 1.0, dv * 1.0)
        shaped = renderer.surface(sc, (dp + 0).reshape(514, 10), (du * 1.0).reshape(514, 10), (dv * 1.0).reshape(514, 10))
        smp = renderer.sampleSurface(sc, 1000, seed=3, as_torch=True)
        cloud = renderer.surface(sc, smp)
        table = renderer.surfaceWeights(sc, as_torch=True)
        copy = res.position.clone()
    assert all(x.device == dev for x in res) and all(x.device == dev for x in smp) and res.material.dtype == torch.int32
    assert res.metallic.dtype == torch.bool and tuple(shaped.position.shape) == (514, 10, 3) and tuple(shaped.alpha.shape) == (514, 10)
    st.synchronize()
    host = lambda r: records(drt.Surface(*(x.cpu().numpy() for x in r)))
    assert sr.same(host(res), want) and sr.same(host(shaped), want) and np.array_equal(copy.cpu().numpy(), want.view(F)[:, sr.POSITION], equal_nan=True)
    ref = sr.sample(s, 3, 0, 1000, cdf)
    assert (smp.prim.cpu().numpy() == ref.view(np.int32)[:, 1]).all() and (smp.u.cpu().numpy() == ref[:, 2]).all()
    assert sr.same(host(cloud), sr.lookup(s, ref.view(np.int32)[:, 1], ref[:, 2], ref[:, 3]))
    assert [int(x) for x in table.cpu().numpy()] == cdf


def test_lookups_leave_the_renderer_alone_and_work_on_a_sharded_one(batch):
    sc, s, prim, u, v, want = batch
    csc, cs = scene("cornell_box")
    _, pos, fwd, depth = SCENES["cornell_box"]
    cam = drt.Camera(pos)
    cam.m_Forward_dir = np.array(fwd, F)
    images = []
    for with_queries in (False, True):
        r = drt.Renderer(0)
        r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=depth)
        r.ResizeBuffer(96, 64)
        r.Render(cam, csc)
        if with_queries:
            info, frame, accum, n, span = r.kernelInfo(), r.GetRenderTargetImage(), r.GetAccumulationBuffer(), r.getSampleCount(), r.kernelSpanMs()
            counters = bytes(r.getCounters())
            smp = r.sampleSurface(csc, 500, seed=1)
            ref = sr.sample(cs, 1, 0, 500)
            assert (smp.prim == ref.view(np.int32)[:, 1]).all()
            assert sr.same(records(r.surface(csc, smp)), sr.lookup(cs, smp.prim, smp.u, smp.v))
            assert [int(x) for x in r.surfaceWeights(csc)] == sr.weights(cs)
            assert r.kernelInfo() == info and r.getSampleCount() == n and r.kernelSpanMs() == span
            assert bytes(r.getCounters()) == counters
            assert r.GetRenderTargetImage().tobytes() == frame.tobytes() and r.GetAccumulationBuffer().tobytes() == accum.tobytes()
        r.Render(cam, csc)
        images.append((r.GetRenderTargetImage(), r.getSampleCount()))
    assert images[0][0].tobytes() == images[1][0].tobytes() and images[0][1] == images[1][1]
    r = drt.Renderer(0)
    r.setShard(8, 1, 2)
    r.ResizeBuffer(96, 64)
    assert sr.same(records(r.surface(sc, prim[:600], u[:600], v[:600])), want[:600])
    smp = r.sampleSurface(sc, 200, seed=9)
    assert (smp.prim == sr.sample(s, 9, 0, 200).view(np.int32)[:, 1]).all()


def test_an_empty_scene_gives_miss_records(renderer, batch):
    sc = drt.Scene()
    sc.addMaterial((0.8, 0.8, 0.8), -1)
    sc.setGeometry(np.zeros((0, 3, 3), F), np.zeros((0, 3, 3), F), np.zeros((0, 3, 2), F), np.zeros(0, np.int32))
    drt.BVHBuilder().buildIterative(sc)
    prim, u, v = batch[2][:300], batch[3][:300], batch[4][:300]
    assert (run_raw(renderer, sc, prim, u, v) == sr.MISS).all()
    smp = renderer.sampleSurface(sc, 70, seed=2)
    assert (smp.prim == -1).all() and not smp.u.any() and not smp.v.any()
    assert renderer.surfaceWeights(sc).shape == (0,)
    assert (renderer.surface(sc, smp).material == -1).all()
    # a mesh without area: a table of zeros, the samples are misses
    flat = flat_scene(np.stack([soup_positions(40, 1)[:, 0]] * 3, axis=1))
    assert not renderer.surfaceWeights(flat).any() and (renderer.sampleSurface(flat, 70, seed=2).prim == -1).all()


def test_error_paths(renderer, batch):
    sc, s, prim, u, v, want = batch
    dev = torch.device(DEV)
    n = 64
    refs = torch.from_numpy(pack_refs(prim[:n + 1], u[:n + 1], v[:n + 1])).to(dev)
    out = torch.full((n + 2, 24), SENTINEL, dtype=torch.float32, device=dev)
    nrm = torch.zeros((len(s.v0), 3, 3), dtype=torch.float32, device=dev)
    table = torch.zeros(len(s.v0), dtype=torch.int64, device=dev)
    host = np.zeros((n + 2, 24), F)
    INV = drt.ERR_INVALID
    R, O, N, T, H = refs.data_ptr(), out.data_ptr(), nrm.data_ptr(), table.data_ptr(), host.ctypes.data
    L = drt._lib
    h = renderer._h
    look = lambda *a: L.drt_renderer_surface_lookup(*a, None)
    for what, args in (("null refs", (h, sc._h, None, None, O, n)), ("null out", (h, sc._h, R, None, None, n)), ("null renderer", (None, sc._h, R, None, O, n)),
                       ("null scene", (h, None, R, None, O, n)), ("misaligned refs", (h, sc._h, R + 4, None, O, n)),
                       ("misaligned out", (h, sc._h, R, None, O + 8, n)), ("misaligned normals", (h, sc._h, R, N + 2, O, n)),
                       ("host refs", (h, sc._h, H, None, O, n)), ("host out", (h, sc._h, R, None, H, n)), ("host normals", (h, sc._h, R, H, O, n)),
                       ("null handles, n = 0", (None, None, R, None, O, 0))):
        assert look(*args) == INV, what
    assert look(h, sc._h, None, None, None, 0) == drt.OK and look(h, sc._h, R, N, O, 0) == drt.OK       # n == 0: nothing to do
    for what, args in (("null out", (h, sc._h, 1, 0, None, n)), ("misaligned out", (h, sc._h, 1, 0, O + 8, n)), ("host out", (h, sc._h, 1, 0, H, n)),
                       ("first + n beyond 2^32", (h, sc._h, 1, 2 ** 32 - n + 1, O, n)), ("null renderer", (None, sc._h, 1, 0, O, n))):
        assert L.drt_renderer_sample_surface(*args, None) == INV, what
    for what, args in (("null table", (h, sc._h, None)), ("misaligned table", (h, sc._h, T + 8)), ("host table", (h, sc._h, H)),
                       ("null scene", (h, None, T))):
        assert L.drt_renderer_surface_weights(*args, None) == INV, what
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and not table.any()                                                    # nothing was launched
    # one reference and one record further on are aligned too
    assert look(h, sc._h, R + 16, N, O + 96, n) == drt.OK
    torch.cuda.synchronize()
    assert (out[0] == SENTINEL).all() and (out[n + 1] == SENTINEL).all() and sr.same(out[1:n + 1].cpu().numpy(), sr.lookup(s, prim[1:n + 1], u[1:n + 1], v[1:n + 1], normals=np.zeros((len(s.v0), 3, 3), F)))
    empty = renderer.surface(sc, prim[:0], u[:0], v[:0])
    assert empty.position.shape == (0, 3) and empty.material.shape == (0,) and renderer.sampleSurface(sc, 0).prim.shape == (0,)
    dp, du = refs.view(torch.int32)[:, 1].contiguous(), refs[:, 2].contiguous()
    for bad in (lambda: renderer.surface(sc, dp.cpu(), du, du),                                           # wrong device
                lambda: renderer.surface(sc, dp, du.double(), du), lambda: renderer.surface(sc, dp.long(), du, du),
                lambda: renderer.surface(sc, dp, du[:5], du), lambda: renderer.surface(sc, dp, du.cpu().numpy(), du),
                lambda: renderer.surface(sc, dp, du, du, normals=nrm[:5]), lambda: renderer.surface(sc, dp, du, du, normals=nrm.double()),
                lambda: renderer.surface(sc, dp, du, du, normals="host"), lambda: renderer.surface(sc, 5)):
        with pytest.raises(drt.DrtError) as e:
            bad()
        assert e.value.code == INV
    # a scene without a BVH
    bare = drt.Scene()
    bare.addMaterial((0.8, 0.8, 0.8), -1)
    bare.setGeometry(SINGLE, np.zeros((1, 3, 3), F), np.zeros((1, 3, 2), F), np.zeros(1, np.int32))
    for call in (lambda: renderer.surface(bare, dp, du, du), lambda: renderer.sampleSurface(bare, 4), lambda: renderer.surfaceWeights(bare)):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == INV
    # a pending asynchronous batch
    r = drt.Renderer(0)
    r.ResizeBuffer(64, 32)
    r.RenderBatchAsync(drt.Camera(SCENES["cornell_box"][1]), sc, 1)
    for call in (lambda: r.surface(sc, dp, du, du), lambda: r.sampleSurface(sc, 4), lambda: r.surfaceWeights(sc)):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == INV
    r.Wait()
    r.surface(sc, dp, du, du), r.sampleSurface(sc, 4), r.surfaceWeights(sc)
    # a tree deeper than 64 levels: refused by the queries that traverse, not by a lookup
    chain = list(rq.degenerate_chain(110))
    chain[0] = (chain[0] * np.float32(2.0 ** -55)).astype(F)
    deep, _ = rq.programmatic_scene(drt, *chain, 1, 2)
    assert deep.bvh_depth > 64
    with pytest.raises(drt.DrtError) as e:
        renderer.traceRays(deep, np.zeros((1, 3), F), np.float32([[0, 0, 1]]))
    assert e.value.code == drt.ERR_UNSUPPORTED
    ds = sr.from_product(deep)
    k = np.arange(110, dtype=np.int32)
    third = np.full(110, 0.25, F)
    assert sr.same(records(renderer.surface(deep, k, third, third)), sr.lookup(ds, k, third, third))
    assert [int(x) for x in renderer.surfaceWeights(deep)] == sr.weights(ds)
    assert sr.same(run_raw(renderer, sc, prim, u, v), want)                                               # after the errors
