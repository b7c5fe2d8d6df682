"""Triangle distance queries on the GPU (drt_renderer_triangle_distance, kernel_tri_distance.hip; Renderer.triangleDistance /
withinDistance / meshDistance): every field of every record bit-equal to the restatement in tests/tri_distance_ref.py -- over one
triangle, the quad, a soup, cornell_box and a tree deeper than the LDS stack, both modes, queries from a point to a triangle across the
whole scene, invalid and zero-area ones, max_dist infinite, per query, 0 and NaN, batch shapes, a refitted device copy, the torch and
the numpy path -- nothing written outside the n records, the renderer's state untouched, and the error codes of include/drt.h.
tests/test_tri_distance_ref.py asserts what the restatement is worth."""
import numpy as np
import pytest

from tests import nearest_ref as nr
from tests import ray_query_ref as rq
from tests import tri_distance_ref as td
from tests import tri_overlap_ref as tv
from tests.scenes import SCENES
from tests.test_gpu_tri_overlap import DEV, ONE_MATERIAL, SCENE_NAMES, _load, flat_scene, scene_pair, sweep_queries

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
_refs = {}


@pytest.fixture(scope="module")
def renderer():
    return drt.Renderer(0)


def same(got, want):
    """Records [N, 12] equal word for word; a NaN d2 (the miss record of a NaN max_dist) equals a NaN d2."""
    got, want = np.ascontiguousarray(got, np.float32).reshape(-1, 12), np.ascontiguousarray(want, np.float32).reshape(-1, 12)
    eq = got.view(np.uint32) == want.view(np.uint32)
    eq[:, 3] |= np.isnan(got[:, 3]) & np.isnan(want[:, 3])
    return got.shape == want.shape and bool(eq.all())


def raw(r, sc, tris, max_dist, out, n, mode, stream=None):
    """The entry point itself on device tensors (or None) or addresses: the status code."""
    ptr = lambda x: x.data_ptr() if torch.is_tensor(x) else x
    return drt._lib.drt_renderer_triangle_distance(r._h, sc._h, ptr(tris), ptr(max_dist), ptr(out), n, mode, stream)


def run_raw(r, sc, q, max_dist=None, mode=td.NEAREST, lead=2, trail=3):
    """One call into the middle of a sentinel-filled buffer: the n records, after asserting that the records around them are untouched."""
    n = len(q)
    t = torch.from_numpy(tv.pack(q)).to(DEV)
    md = None if max_dist is None else torch.from_numpy(np.array(np.broadcast_to(np.float32(max_dist), n))).to(DEV)
    out = torch.full((lead + n + trail, 12), SENTINEL, dtype=torch.float32, device=DEV)
    assert raw(r, sc, t, md, out[lead:], n, mode) == drt.OK
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[:lead] == SENTINEL).all() and (h[lead + n:] == SENTINEL).all()
    return h[lead:lead + n]


def fields(res):
    """A TriNearest of the Python interface as records."""
    return td.records(td.TriNear(res.point_q, res.d2, res.point_t, res.prim, res.u, res.v, res.feature))


def case(name):
    """(scene, Geometry, queries, per-query max_dist, and the restatement's records for [infinite, per query] x [NEAREST, ANY]), made
    once per scene and left unchanged."""
    if name not in _refs:
        sc, g = scene_pair(name)
        q = sweep_queries(g, 90, 11, whole=1) if name == "soup" else sweep_queries(g, 150, 11)
        rng = np.random.default_rng(3)
        lo, hi = nr.bounds(g)
        md = (rng.uniform(0, 1, len(q)) ** 2 * 0.3 * float((hi - lo).max())).astype(np.float32)
        md[::7], md[3::11], md[5::17] = 0, np.nan, np.inf
        depth = np.zeros(len(q), np.int64)
        want = {(None, td.NEAREST): td.records(td.distance(g, q, depth=depth)), (None, td.ANY): td.records(td.distance(g, q, mode=td.ANY)),
                ("md", td.NEAREST): td.records(td.distance(g, q, md)), ("md", td.ANY): td.records(td.distance(g, q, md, td.ANY))}
        _refs[name] = (sc, g, q, md, want, depth)
    return _refs[name]


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_both_modes_are_bit_equal_to_the_restatement(renderer, name):
    sc, g, q, md, want, depth = case(name)
    n = len(q)
    near = want[(None, td.NEAREST)]
    prim = near.view(np.int32)[:, 7]
    # infinite: all but the invalid ones (and on the chain those whose fourth powers overflow: a NaN never wins)
    assert (name == "chain" or (prim[:-4] >= 0).all()) and (prim >= 0).any() and (prim[-4:] == -1).all() and np.isinf(near[-4:, 3]).all()
    assert name != "chain" or depth.max() > 8                                                         # entries held in the HBM levels
    feature = near.view(np.int32)[:, 10]
    assert (feature[prim >= 0] >= 16).any() and (near[feature >= 16, 3] == 0).all()                   # touching: d2 = 0
    limited = want[("md", td.NEAREST)].view(np.int32)[:, 7]
    assert (limited >= 0).any() and (limited[prim >= 0] == -1).any()
    for (which, mode), ref in want.items():
        assert same(run_raw(renderer, sc, q, None if which is None else md, mode), ref), (name, which, mode)
    # the Python interface: numpy in, numpy out; [N, 3, 3] and the packed [N, 12] are the same query, the pad words are ignored
    got = renderer.triangleDistance(sc, q)
    assert isinstance(got, drt.TriNearest) and got.prim.dtype == np.int32 and got.feature.dtype == np.int32 and got.point_q.shape == (n, 3)
    assert same(fields(got), near)
    packed = tv.pack(q)
    packed[:, 9:] = np.nan
    assert same(fields(renderer.triangleDistance(sc, packed, md)), want[("md", td.NEAREST)])
    scalar = np.float32(md[1])
    assert same(fields(renderer.triangleDistance(sc, q, float(scalar))), td.records(td.distance(g, q, scalar)))
    # the boolean: mode ANY with prim >= 0; a query within the distance is within it in both modes
    within = renderer.withinDistance(sc, q, md)
    assert within.dtype == np.bool_ and within.shape == (n,) and (within == (want[("md", td.ANY)].view(np.int32)[:, 7] >= 0)).all()
    assert (within == (limited >= 0)).all()
    # the nearest pair of the batch, ties to the smallest query index
    best = renderer.meshDistance(sc, q[:-4][prim[:-4] >= 0][::-1])
    d2 = near[:-4][prim[:-4] >= 0][::-1, 3]
    assert isinstance(best, drt.MeshDistance) and best.d2 == d2.min() and best.query == int(np.nonzero(d2 == d2.min())[0][0])


def test_hand_cases_on_one_triangle(renderer):
    """tests/test_tri_distance_ref.py's cases against the triangle (0, 0, 0), (4, 0, 0), (0, 4, 0): the deciding candidate and d2."""
    sc, _ = flat_scene(np.float32([[[0, 0, 0], [4, 0, 0], [0, 4, 0]]]))
    g = nr.from_product(sc)
    from tests.test_tri_distance_ref import HAND_CASES
    q = np.float32([c[0] for c in HAND_CASES])
    got = renderer.triangleDistance(sc, q)
    assert same(fields(got), td.records(td.distance(g, q)))
    assert got.d2.tolist() == [c[1] for c in HAND_CASES] and got.feature.tolist() == [c[2] for c in HAND_CASES]
    assert renderer.withinDistance(sc, q, 1.5).tolist() == [c[1] < 2.25 for c in HAND_CASES]


@pytest.fixture(scope="module")
def batch():
    """257 queries on cornell_box with per-query distances and the restatement's records in both modes."""
    sc, g = scene_pair("cornell_box")
    q = sweep_queries(g, 260, 21)[-257:]
    assert len(q) == 257
    md = (np.random.default_rng(8).uniform(0, 1, 257) ** 2 * 0.25).astype(np.float32)
    md[::5] = np.inf
    near, first = td.records(td.distance(g, q, md)), td.records(td.distance(g, q, md, td.ANY))
    prim = near.view(np.int32)[:, 7]
    assert (prim >= 0).sum() > 50 and (prim == -1).sum() > 50 and (near.view(np.uint32) != first.view(np.uint32)).any()
    return sc, g, q, md, near, first


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(renderer, batch, n):
    sc, g, q, md, near, first = batch
    for sl in (slice(0, n), slice(257 - n, 257)):
        assert same(run_raw(renderer, sc, q[sl], md[sl]), near[sl])
        assert same(run_raw(renderer, sc, q[sl], md[sl], td.ANY), first[sl])


def test_about_5000_queries_a_permutation_and_a_second_run(renderer, batch):
    """20 x 257 = 5140 queries: the claim crosses shards, and waves refill lanes from more than one of them."""
    sc, g, q, md, near, first = batch
    tiles = 20
    dev_q = torch.from_numpy(q).to(DEV).repeat(tiles, 1, 1)
    dev_md = torch.from_numpy(md).to(DEV).repeat(tiles)
    want = np.tile(near, (tiles, 1))
    res = renderer.triangleDistance(sc, dev_q, dev_md)
    assert all(torch.is_tensor(x) and x.device == torch.device(DEV) for x in res) and res.prim.dtype == torch.int32
    host = lambda r: fields(drt.TriNearest(*(x.cpu().numpy() for x in r)))
    first_run = host(res)
    assert same(first_run, want)
    assert host(renderer.triangleDistance(sc, dev_q, dev_md)).tobytes() == first_run.tobytes()         # two runs: identical bytes
    perm = np.random.default_rng(2).permutation(len(dev_q))
    dev_perm = torch.from_numpy(perm).to(DEV)
    assert same(host(renderer.triangleDistance(sc, dev_q[dev_perm], dev_md[dev_perm])), want[perm])
    within = renderer.withinDistance(sc, dev_q[dev_perm], dev_md[dev_perm])
    assert within.dtype == torch.bool and (within.cpu().numpy() == np.tile(first.view(np.int32)[:, 7] >= 0, tiles)[perm]).all()


def test_mesh_distance_takes_the_smallest_query_index_of_a_tie(renderer, batch):
    sc, g, q, md, near, first = batch
    far = near.view(np.int32)[:, 7] >= 0
    far &= near[:, 3] > 0
    i = int(np.nonzero(far)[0][np.argmin(near[far, 3])])                       # the nearest query that does not touch
    apart = np.nonzero(far)[0]
    mesh = np.concatenate([q[apart[apart != i]][:40], q[i:i + 1], q[apart[apart != i]][40:60], q[i:i + 1]])   # the same triangle twice
    mmd = np.concatenate([md[apart[apart != i]][:40], md[i:i + 1], md[apart[apart != i]][40:60], md[i:i + 1]])
    ref = td.distance(g, mesh, mmd)
    assert ref.d2[40] == ref.d2[61] == ref.d2.min() and (ref.d2 == ref.d2.min()).sum() == 2
    got = renderer.meshDistance(sc, mesh, mmd)
    assert got.query == 40 and got.d2 == ref.d2[40] and got.prim == ref.prim[40] and got.feature == ref.feature[40]
    assert (got.point_q == ref.point_q[40]).all() and (got.point_t == ref.point_t[40]).all()
    dev = renderer.meshDistance(sc, torch.from_numpy(mesh[::-1].copy()).to(DEV), torch.from_numpy(mmd[::-1].copy()).to(DEV))
    assert all(torch.is_tensor(x) and x.device == torch.device(DEV) for x in dev)
    assert int(dev.query) == 0 and float(dev.d2) == ref.d2[40] and int(dev.prim) == ref.prim[40] and dev.query.dtype == torch.int32
    # nothing within the distance, and an empty batch
    for miss in (renderer.meshDistance(sc, mesh, np.float32(0.5 * np.sqrt(ref.d2.min()))), renderer.meshDistance(sc, np.zeros((0, 3, 3), np.float32))):
        assert miss.query == -1 and miss.prim == -1 and np.isinf(miss.d2) and not miss.point_q.any() and miss.feature == 0
    # touching meshes: d2 = 0 at the first touching query
    touch = renderer.meshDistance(sc, q)
    t = np.nonzero((near.view(np.int32)[:, 7] >= 0) & (near[:, 3] == 0))[0]
    assert touch.d2 == 0 and touch.query == t[0] and touch.feature >= 16


def test_after_a_refit_the_moved_mesh_answers(renderer):
    sc, st = _load("cornell_box")
    moved = (st[0] + np.random.default_rng(1).normal(0, 0.05, st[0].shape)).astype(np.float32)
    host, _ = _load("cornell_box")
    host.refit(moved)                                          # the host scene refitted with the same positions
    g_old, g_new = nr.from_product(sc), nr.from_product(host)
    q = np.concatenate([sweep_queries(g_old, 60, 4, whole=1), sweep_queries(g_new, 60, 5, whole=1)])
    old, new = td.records(td.distance(g_old, q)), td.records(td.distance(g_new, q))
    assert (old.view(np.uint32) != new.view(np.uint32)).any(axis=1).mean() > 0.3
    r = drt.Renderer(0)
    assert same(fields(r.triangleDistance(sc, q)), old)
    r.refit(sc, torch.from_numpy(moved).to(DEV))
    assert same(fields(r.triangleDistance(sc, q)), new)
    assert (r.withinDistance(sc, q, 0.1) == (td.distance(g_new, q, 0.1, td.ANY).prim >= 0)).all()
    assert same(fields(renderer.triangleDistance(sc, q)), old)   # a renderer that was not refitted


def test_torch_path_stays_on_the_device_and_orders_with_the_stream(renderer, batch):
    sc, g, q, md, near, first = batch
    dev = torch.device(DEV)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        dq = torch.from_numpy(q).to(dev)
        dmd = torch.from_numpy(md).to(dev)
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(2000000)                  # the inputs' producer is still busy when the queries are enqueued
        res = renderer.triangleDistance(sc, dq * 1.0, dmd * 1.0)
        packed = renderer.triangleDistance(sc, torch.from_numpy(tv.pack(q)).to(dev) * 1.0, dmd * 1.0)
        within = renderer.withinDistance(sc, dq * 1.0, dmd * 1.0)
        d2_copy = res.d2.clone()
    assert all(x.device == dev for x in res) and within.device == dev and within.dtype == torch.bool
    assert res.d2.dtype == torch.float32 and res.prim.dtype == torch.int32 and tuple(res.point_t.shape) == (257, 3)
    s.synchronize()
    host = lambda r: fields(drt.TriNearest(*(x.cpu().numpy() for x in r)))
    assert same(host(res), near) and same(host(packed), near) and (d2_copy.cpu().numpy() == near[:, 3]).all()
    assert (within.cpu().numpy() == (first.view(np.int32)[:, 7] >= 0)).all()


def test_queries_leave_the_renderer_alone_and_work_on_a_sharded_one(renderer, batch):
    sc, g, q, md, near, first = batch
    _, pos, fwd, depth = SCENES["cornell_box"]
    cam = drt.Camera(pos)
    cam.m_Forward_dir = np.array(fwd, np.float32)
    images = []
    for with_queries in (False, True):
        r = drt.Renderer(0)
        r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=depth)
        r.ResizeBuffer(96, 64)
        r.Render(cam, sc)
        if with_queries:
            info, frame, accum, n, span = r.kernelInfo(), r.GetRenderTargetImage(), r.GetAccumulationBuffer(), r.getSampleCount(), r.kernelSpanMs()
            counters = bytes(r.getCounters())
            assert same(fields(r.triangleDistance(sc, q, md)), near)
            assert (r.withinDistance(sc, q, md) == (first.view(np.int32)[:, 7] >= 0)).all()
            assert r.kernelInfo() == info and r.getSampleCount() == n and r.kernelSpanMs() == span
            assert bytes(r.getCounters()) == counters
            assert r.GetRenderTargetImage().tobytes() == frame.tobytes() and r.GetAccumulationBuffer().tobytes() == accum.tobytes()
        r.Render(cam, sc)
        images.append((r.GetRenderTargetImage(), r.getSampleCount()))
    assert images[0][0].tobytes() == images[1][0].tobytes() and images[0][1] == images[1][1]
    r = drt.Renderer(0)
    r.setShard(8, 1, 2)
    r.ResizeBuffer(96, 64)
    assert same(fields(r.triangleDistance(sc, q, md)), near)
    assert (r.withinDistance(sc, q, md) == (first.view(np.int32)[:, 7] >= 0)).all()


def test_an_empty_scene_gives_the_miss_record(renderer, batch):
    sc = drt.Scene()
    sc.addMaterial(*ONE_MATERIAL[0])
    sc.setGeometry(np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 2), np.float32), np.zeros(0, np.int32))
    drt.BVHBuilder().buildIterative(sc)
    q, md = batch[2], batch[3]
    miss = np.zeros((len(q), 12), np.float32)
    miss[:, 3], miss.view(np.int32)[:, 7] = md * md, -1
    for mode in (td.NEAREST, td.ANY):
        assert same(run_raw(renderer, sc, q, md, mode), miss)
    assert not renderer.withinDistance(sc, q, 1e30).any() and renderer.meshDistance(sc, q).prim == -1


def test_error_paths(renderer, batch):
    sc, g, ref_q, ref_md, near, first = batch
    dev = torch.device(DEV)
    n = 64
    tris = torch.zeros((n + 1, 12), dtype=torch.float32, device=dev)
    tris[:, 3], tris[:, 7] = 1, 1                                                # (0, 0, 0), (1, 0, 0), (0, 1, 0)
    md = torch.ones(n + 1, dtype=torch.float32, device=dev)
    out = torch.full((n + 2, 12), SENTINEL, dtype=torch.float32, device=dev)
    host = np.zeros((n + 2, 12), np.float32)
    INV = drt.ERR_INVALID
    B, M, O, H = tris.data_ptr(), md.data_ptr(), out.data_ptr(), host.ctypes.data
    L = drt._lib
    fn = lambda r, s, *a: L.drt_renderer_triangle_distance(r, s, *a, None)
    h = renderer._h
    for what, args in (("null tris", (h, sc._h, None, M, O, n, 0)), ("null out", (h, sc._h, B, M, None, n, 0)),
                       ("null renderer", (None, sc._h, B, M, O, n, 0)), ("null scene", (h, None, B, M, O, n, 1)),
                       ("mode 2", (h, sc._h, B, M, O, n, 2)), ("mode -1", (h, sc._h, B, M, O, n, -1)), ("mode 2, n = 0", (h, sc._h, B, M, O, 0, 2)),
                       ("mode 2, null tris", (h, sc._h, None, M, O, n, 2)),
                       ("misaligned tris", (h, sc._h, B + 4, M, O, n, 0)), ("misaligned out", (h, sc._h, B, M, O + 8, n, 0)),
                       ("misaligned max_dist", (h, sc._h, B, M + 2, O, n, 0)),
                       ("host tris", (h, sc._h, H, M, O, n, 0)), ("host max_dist", (h, sc._h, B, H, O, n, 1)), ("host out", (h, sc._h, B, M, H, n, 0)),
                       ("null handles, n = 0", (None, None, B, M, O, 0, 0))):
        assert fn(*args) == INV, what
        if what.startswith("mode"):
            assert b"mode" in L.drt_last_error(), what                                                    # checked first after the handles
    for mode in (0, 1):
        assert fn(h, sc._h, None, None, None, 0, mode) == drt.OK                                          # n == 0: nothing to do
        assert fn(h, sc._h, B, M, O, 0, mode) == drt.OK
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()                                                                         # nothing was launched
    # tris and out need 16-byte alignment, max_dist 4: one triangle, one record and one word further on
    assert fn(h, sc._h, B + 48, M + 4, O + 48, n, 0) == drt.OK
    torch.cuda.synchronize()
    assert (out[0] == SENTINEL).all() and (out[n + 1] == SENTINEL).all() and not (out[1:n + 1, 3] == SENTINEL).any()
    empty = renderer.triangleDistance(sc, np.zeros((0, 3, 3), np.float32))
    assert empty.d2.shape == (0,) and empty.point_q.shape == (0, 3) and renderer.withinDistance(sc, np.zeros((0, 12), np.float32), 1.0).shape == (0,)
    for bad in (lambda: renderer.triangleDistance(sc, tris.cpu()),                                        # wrong device
                lambda: renderer.triangleDistance(sc, tris.double()),                                     # wrong dtype
                lambda: renderer.triangleDistance(sc, tris[:, :9]),                                       # [N, 9] is neither form
                lambda: renderer.triangleDistance(sc, tris, md[:5]),                                      # one distance per triangle
                lambda: renderer.triangleDistance(sc, tris, md.cpu().numpy()),                            # mix of numpy and torch
                lambda: renderer.triangleDistance(sc, tris, md.double()),
                lambda: renderer.triangleDistance(sc, tris, "far"),
                lambda: renderer.withinDistance(sc, host.astype(np.float64), 1.0),
                lambda: renderer.meshDistance(sc, tris[:, :11])):
        with pytest.raises(drt.DrtError) as e:
            bad()
        assert e.value.code == INV
    # a pending asynchronous batch
    r = drt.Renderer(0)
    r.ResizeBuffer(64, 32)
    r.RenderBatchAsync(drt.Camera(SCENES["cornell_box"][1]), sc, 1)
    for call in (lambda: r.triangleDistance(sc, tris), lambda: r.withinDistance(sc, tris, 1.0), lambda: r.meshDistance(sc, tris)):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == INV
    assert raw(r, sc, tris, md, out, n, 0) == INV
    r.Wait()
    r.triangleDistance(sc, tris), r.withinDistance(sc, tris, 1.0)
    # a tree deeper than 64 levels: the chain's centroids double per triangle (scaled down so that no area overflows)
    chain = list(rq.degenerate_chain(110))
    chain[0] = (chain[0] * np.float32(2.0 ** -55)).astype(np.float32)
    deep, _ = rq.programmatic_scene(drt, *chain, 1, 2)
    assert deep.bvh_depth > 64
    for call in (lambda: renderer.triangleDistance(deep, tris), lambda: renderer.withinDistance(deep, tris, 1.0)):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == drt.ERR_UNSUPPORTED
    assert same(fields(renderer.triangleDistance(sc, ref_q, ref_md)), near)                               # after the errors
