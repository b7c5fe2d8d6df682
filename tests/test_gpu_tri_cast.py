"""Triangle casts on the GPU (drt_renderer_triangle_cast, kernel_tri_cast.hip; Renderer.triangleCast / castsAny / meshCast): every
word of every record bit-equal to the restatement in tests/tri_cast_ref.py -- over one triangle, the quad, a soup, cornell_box and a
tree deeper than the LDS stack, both modes, query triangles from a point to a triangle across the whole scene moving toward, away from
and along the surfaces, invalid and zero-area ones, d = 0, tmax a scalar, per cast, 0, NaN and infinite, batch shapes, a refitted device
copy, the torch and the numpy path -- nothing written outside the n records, the renderer's state untouched, and the error codes of
include/drt.h.  tests/test_tri_cast_ref.py asserts what the restatement is worth."""
import numpy as np
import pytest

from tests import nearest_ref as nr
from tests import ray_query_ref as rq
from tests import tri_cast_ref as tc
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
    """Records [N, 12] equal word for word.  In the float fields a NaN equals a NaN: the miss record of a NaN tmax, and the point, u and
    v of a contact whose third powers overflowed (the chain's largest triangles: inf / inf) -- which NaN an invalid operation gives is
    the processor's choice, not the rule's (drt.h says so)."""
    got, want = np.ascontiguousarray(got, np.float32).reshape(-1, 12), np.ascontiguousarray(want, np.float32).reshape(-1, 12)
    eq = got.view(np.uint32) == want.view(np.uint32)
    floats = [0, 1, 2, 3, 4, 5, 6, 8, 9]
    eq[:, floats] |= np.isnan(got[:, floats]) & np.isnan(want[:, floats])
    return got.shape == want.shape and bool(eq.all())


def motions_of(d, tmax, n):
    m = np.zeros((n, 4), np.float32)
    m[:, 0:3], m[:, 3] = d, tmax
    return m


def raw(r, sc, tris, motions, out, n, mode, stream=None):
    """The entry point itself on device tensors (or None) or addresses: the status code."""
    ptr = lambda x: x.data_ptr() if torch.is_tensor(x) else x
    return drt._lib.drt_renderer_triangle_cast(r._h, sc._h, ptr(tris), ptr(motions), ptr(out), n, mode, stream)


def run_raw(r, sc, q, d, tmax, mode=tc.FIRST, lead=2, trail=3):
    """One call into the middle of a sentinel-filled buffer: the n records, after asserting that the records around them are untouched."""
    n = len(q)
    t = torch.from_numpy(tv.pack(q)).to(DEV)
    m = torch.from_numpy(motions_of(d, tmax, n)).to(DEV)
    out = torch.full((lead + n + trail, 12), SENTINEL, dtype=torch.float32, device=DEV)
    assert raw(r, sc, t, m, out[lead:], n, mode) == drt.OK
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[:lead] == SENTINEL).all() and (h[lead + n:] == SENTINEL).all()
    return h[lead:lead + n]


def fields(res):
    """A TriHits of the Python interface as records."""
    return tc.records(tc.TriHits(res.point, res.t, res.normal, res.prim, res.u, res.v, res.feature))


def directions(g, q, seed):
    """One direction per query: toward a point of the surface, away from one, along an edge of the mesh, and a few zeros; lengths of
    0.2 to 2 times the distance to that point (or the extent)."""
    rng = np.random.default_rng(seed)
    n = len(q)
    lo, hi = nr.bounds(g)
    extent = np.float32((hi - lo).max())
    with np.errstate(invalid="ignore"):
        toward = nr.surface_points(g, n, rng, 0.0).astype(np.float32) - q.mean(axis=1)
    k = rng.integers(0, len(g.v0), n)
    along = g.e1[k] / np.maximum(np.linalg.norm(g.e1[k], axis=1, keepdims=True), np.float32(1e-30)) * extent
    kind = np.arange(n) % 3
    d = np.where(kind[:, None] == 0, toward, np.where(kind[:, None] == 1, -toward, along)) * rng.uniform(0.2, 2, (n, 1))
    d = np.nan_to_num(d, nan=1.0, posinf=1.0, neginf=-1.0).astype(np.float32)       # (the invalid queries: any direction)
    d[5::19] = 0
    d[7::23, 1] = 0                                                                 # an axis the motion does not use: inv_d is infinite
    return d


def case(name):
    """(scene, Geometry, queries, directions, per-cast tmax, and the restatement's records for [tmax 1, per cast] x [FIRST, ANY]), made
    once per scene and left unchanged."""
    if name not in _refs:
        sc, g = scene_pair(name)
        q = sweep_queries(g, 90, 11, whole=0) if name == "soup" else sweep_queries(g, 150, 11)   # (a triangle across the soup visits every node: slow in numpy)
        d = directions(g, q, 5)
        if name == "chain":
            # triangle i of the chain lies in the plane x = 2^i: small triangles that start in front of the first planes and cross them
            # all, so that the far children wait on the stack beyond the LDS levels
            q[:6] = np.float32([(0.25, 0.01, 0.01), (0.25, 0.03, 0.01), (0.25, 0.01, 0.03)])
            d[:6] = np.float32([(2.0 ** e, 0, 0) for e in (30, 20, 12, 8, 4, 1)])
        rng = np.random.default_rng(3)
        tmax = (rng.uniform(0, 1.5, len(q)) ** 2).astype(np.float32)
        tmax[::7], tmax[3::11], tmax[5::17], tmax[6::29] = 0, np.nan, np.inf, -1
        depth = np.zeros(len(q), np.int64)
        want = {("one", tc.FIRST): tc.records(tc.cast(g, q, d, 1.0, depth=depth)), ("one", tc.ANY): tc.records(tc.cast(g, q, d, 1.0, tc.ANY)),
                ("per", tc.FIRST): tc.records(tc.cast(g, q, d, tmax)), ("per", tc.ANY): tc.records(tc.cast(g, q, d, tmax, tc.ANY))}
        _refs[name] = (sc, g, q, d, tmax, want, depth)
    return _refs[name]


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_both_modes_are_bit_equal_to_the_restatement(renderer, name):
    sc, g, q, d, tmax, want, depth = case(name)
    n = len(q)
    first = want[("one", tc.FIRST)]
    prim, feature = first.view(np.int32)[:, 7], first.view(np.int32)[:, 10]
    assert (prim >= 0).any() and (prim[-4:] == -1).all() and (first[-4:, 3] == 1).all() and (feature[-4:] == -1).all()   # the invalid ones
    assert name != "chain" or depth.max() > 8                                                         # entries held in the HBM levels
    assert (feature >= 16).any() and (first[feature >= 16, 3] == 0).all()                             # start overlaps: t = 0
    assert name == "single" or ((feature >= 0) & (feature < 16) & (first[:, 3] > 0)).any()            # contacts on the way
    limited = want[("per", tc.FIRST)].view(np.int32)[:, 7]
    assert (limited >= 0).any() and (limited[prim >= 0] == -1).any()
    for (which, mode), ref in want.items():
        assert same(run_raw(renderer, sc, q, d, 1.0 if which == "one" else tmax, mode), ref), (name, which, mode)
    # the Python interface: numpy in, numpy out; [N, 3, 3] and the packed [N, 12] are the same query, the pad words are ignored
    got = renderer.triangleCast(sc, q, d)
    assert isinstance(got, drt.TriHits) and got.prim.dtype == np.int32 and got.feature.dtype == np.int32 and got.point.shape == (n, 3)
    assert same(fields(got), first)
    packed = tv.pack(q)
    packed[:, 9:] = np.nan
    assert same(fields(renderer.triangleCast(sc, packed, d, tmax)), want[("per", tc.FIRST)])
    # one direction for the whole batch, and a scalar tmax
    assert same(fields(renderer.triangleCast(sc, q, d[1], 0.75)), tc.records(tc.cast(g, q, d[1], 0.75)))
    # the boolean: mode ANY with prim >= 0; a cast that touches before tmax does so in both modes
    hits = renderer.castsAny(sc, q, d, tmax)
    assert hits.dtype == np.bool_ and hits.shape == (n,) and (hits == (want[("per", tc.ANY)].view(np.int32)[:, 7] >= 0)).all()
    assert (hits == (limited >= 0)).all()


def test_hand_cases_on_one_triangle(renderer):
    """tests/test_tri_cast_ref.py's cases against the triangle (0, 0, 0), (4, 0, 0), (0, 4, 0): t, the deciding candidate, the normal."""
    sc, _ = flat_scene(np.float32([[[0, 0, 0], [4, 0, 0], [0, 4, 0]]]))
    g = nr.from_product(sc)
    from tests.test_tri_cast_ref import HAND_CASES
    q, d, tmax = np.float32([c[0] for c in HAND_CASES]), np.float32([c[1] for c in HAND_CASES]), np.float32([c[2] for c in HAND_CASES])
    got = renderer.triangleCast(sc, q, d, tmax)
    assert same(fields(got), tc.records(tc.cast(g, q, d, tmax)))
    assert got.t.tolist() == [c[3] for c in HAND_CASES] and got.prim.tolist() == [c[4] for c in HAND_CASES]
    assert got.feature.tolist() == [c[5] for c in HAND_CASES] and (got.normal == np.float32([c[6] for c in HAND_CASES])).all()
    assert renderer.castsAny(sc, q, d, tmax).tolist() == [c[4] >= 0 for c in HAND_CASES]


@pytest.fixture(scope="module")
def batch():
    """257 casts on cornell_box with per-cast tmax and the restatement's records in both modes."""
    sc, g = scene_pair("cornell_box")
    q = sweep_queries(g, 260, 21)[-257:]
    assert len(q) == 257
    d = directions(g, q, 9)
    tmax = (np.random.default_rng(8).uniform(0, 1.4, 257) ** 2).astype(np.float32)
    tmax[::5] = np.inf
    first, any_ = tc.records(tc.cast(g, q, d, tmax)), tc.records(tc.cast(g, q, d, tmax, tc.ANY))
    prim = first.view(np.int32)[:, 7]
    assert (prim >= 0).sum() > 50 and (prim == -1).sum() > 50 and (first.view(np.uint32) != any_.view(np.uint32)).any()
    return sc, g, q, d, tmax, first, any_


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(renderer, batch, n):
    sc, g, q, d, tmax, first, any_ = batch
    for sl in (slice(0, n), slice(257 - n, 257)):
        assert same(run_raw(renderer, sc, q[sl], d[sl], tmax[sl]), first[sl])
        assert same(run_raw(renderer, sc, q[sl], d[sl], tmax[sl], tc.ANY), any_[sl])


def test_about_5000_casts_a_permutation_and_a_second_run(renderer, batch):
    """20 x 257 = 5140 casts: the claim crosses shards, and waves refill lanes from more than one of them."""
    sc, g, q, d, tmax, first, any_ = batch
    tiles = 20
    dev_q = torch.from_numpy(q).to(DEV).repeat(tiles, 1, 1)
    dev_d = torch.from_numpy(d).to(DEV).repeat(tiles, 1)
    dev_t = torch.from_numpy(tmax).to(DEV).repeat(tiles)
    want = np.tile(first, (tiles, 1))
    res = renderer.triangleCast(sc, dev_q, dev_d, dev_t)
    assert all(torch.is_tensor(x) and x.device == torch.device(DEV) for x in res) and res.prim.dtype == torch.int32
    host = lambda r: fields(drt.TriHits(*(x.cpu().numpy() for x in r)))
    first_run = host(res)
    assert same(first_run, want)
    assert host(renderer.triangleCast(sc, dev_q, dev_d, dev_t)).tobytes() == first_run.tobytes()         # two runs: identical bytes
    perm = np.random.default_rng(2).permutation(len(dev_q))
    dev_perm = torch.from_numpy(perm).to(DEV)
    assert same(host(renderer.triangleCast(sc, dev_q[dev_perm], dev_d[dev_perm], dev_t[dev_perm])), want[perm])
    hits = renderer.castsAny(sc, dev_q[dev_perm], dev_d[dev_perm], dev_t[dev_perm])
    assert hits.dtype == torch.bool and (hits.cpu().numpy() == np.tile(any_.view(np.int32)[:, 7] >= 0, tiles)[perm]).all()


def test_mesh_cast_takes_the_smallest_query_index_of_a_tie(renderer, batch):
    sc, g, q, d, tmax, first, any_ = batch
    one = d[0]                                                                 # a mesh moves as one: the same direction for all
    ref_all = tc.cast(g, q, one, 1.0)
    later = (ref_all.prim >= 0) & (ref_all.t > 0)
    i = int(np.nonzero(later)[0][np.argmin(ref_all.t[later])])                 # the earliest contact that is no start overlap
    others = np.nonzero(later)[0]
    others = others[others != i]
    assert len(others) >= 12
    mesh = np.concatenate([q[others[:8]], q[i:i + 1], q[others[8:12]], q[i:i + 1]])   # the same cast twice
    ref = tc.cast(g, mesh, one, 1.0)
    assert ref.t[8] == ref.t[13] == ref.t.min() and (ref.t == ref.t.min()).sum() == 2
    got = renderer.meshCast(sc, mesh, one, 1.0)
    assert isinstance(got, drt.MeshHit) and got.query == 8 and got.t == ref.t[8] and got.prim == ref.prim[8] and got.feature == ref.feature[8]
    assert (got.point == ref.point[8]).all() and (got.normal == ref.normal[8]).all()
    dev = renderer.meshCast(sc, torch.from_numpy(mesh[::-1].copy()).to(DEV), torch.from_numpy(one).to(DEV), 1.0)
    assert all(torch.is_tensor(x) and x.device == torch.device(DEV) for x in dev)
    assert int(dev.query) == 0 and float(dev.t) == ref.t[8] and int(dev.prim) == ref.prim[8] and dev.query.dtype == torch.int32
    # nothing before tmax, and an empty batch
    for miss in (renderer.meshCast(sc, mesh, one, np.float32(0.5) * ref.t.min()), renderer.meshCast(sc, np.zeros((0, 3, 3), np.float32), one)):
        assert miss.query == -1 and miss.prim == -1 and np.isinf(miss.t) and not miss.point.any() and not miss.normal.any() and miss.feature == -1
    # a mesh that touches at the start: t = 0 at the first such query
    touch = renderer.meshCast(sc, q, one, 1.0)
    t = np.nonzero((ref_all.prim >= 0) & (ref_all.t == 0))[0]
    assert touch.t == 0 and touch.query == t[0] and touch.feature >= 16


def test_after_a_refit_the_moved_mesh_answers(renderer):
    sc, st = _load("cornell_box")
    moved = (st[0] + np.random.default_rng(1).normal(0, 0.05, st[0].shape)).astype(np.float32)
    host, _ = _load("cornell_box")
    host.refit(moved)                                          # the host scene refitted with the same positions
    g_old, g_new = nr.from_product(sc), nr.from_product(host)
    q = np.concatenate([sweep_queries(g_old, 60, 4, whole=1), sweep_queries(g_new, 60, 5, whole=1)])
    d = directions(g_old, q, 6)
    old, new = tc.records(tc.cast(g_old, q, d, 1.0)), tc.records(tc.cast(g_new, q, d, 1.0))
    assert (old.view(np.uint32) != new.view(np.uint32)).any(axis=1).mean() > 0.3
    r = drt.Renderer(0)
    assert same(fields(r.triangleCast(sc, q, d)), old)
    r.refit(sc, torch.from_numpy(moved).to(DEV))
    assert same(fields(r.triangleCast(sc, q, d)), new)
    assert (r.castsAny(sc, q, d, 0.5) == (tc.cast(g_new, q, d, 0.5, tc.ANY).prim >= 0)).all()
    assert same(fields(renderer.triangleCast(sc, q, d)), old)   # a renderer that was not refitted


def test_torch_path_stays_on_the_device_and_orders_with_the_stream(renderer, batch):
    sc, g, q, d, tmax, first, any_ = batch
    dev = torch.device(DEV)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        dq, dd, dt = torch.from_numpy(q).to(dev), torch.from_numpy(d).to(dev), torch.from_numpy(tmax).to(dev)
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(2000000)                  # the inputs' producer is still busy when the casts are enqueued
        res = renderer.triangleCast(sc, dq * 1.0, dd * 1.0, dt * 1.0)
        packed = renderer.triangleCast(sc, torch.from_numpy(tv.pack(q)).to(dev) * 1.0, dd * 1.0, dt * 1.0)
        hits = renderer.castsAny(sc, dq * 1.0, dd * 1.0, dt * 1.0)
        t_copy = res.t.clone()
    assert all(x.device == dev for x in res) and hits.device == dev and hits.dtype == torch.bool
    assert res.t.dtype == torch.float32 and res.prim.dtype == torch.int32 and tuple(res.normal.shape) == (257, 3)
    s.synchronize()
    host = lambda r: fields(drt.TriHits(*(x.cpu().numpy() for x in r)))
    assert same(host(res), first) and same(host(packed), first) and (t_copy.cpu().numpy() == first[:, 3]).all()
    assert (hits.cpu().numpy() == (any_.view(np.int32)[:, 7] >= 0)).all()


def test_casts_leave_the_renderer_alone_and_work_on_a_sharded_one(renderer, batch):
    sc, g, q, d, tmax, first, any_ = batch
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
            assert same(fields(r.triangleCast(sc, q, d, tmax)), first)
            assert (r.castsAny(sc, q, d, tmax) == (any_.view(np.int32)[:, 7] >= 0)).all()
            assert r.kernelInfo() == info and r.getSampleCount() == n and r.kernelSpanMs() == span
            assert bytes(r.getCounters()) == counters
            assert r.GetRenderTargetImage().tobytes() == frame.tobytes() and r.GetAccumulationBuffer().tobytes() == accum.tobytes()
        r.Render(cam, sc)
        images.append((r.GetRenderTargetImage(), r.getSampleCount()))
    assert images[0][0].tobytes() == images[1][0].tobytes() and images[0][1] == images[1][1]
    r = drt.Renderer(0)
    r.setShard(8, 1, 2)
    r.ResizeBuffer(96, 64)
    assert same(fields(r.triangleCast(sc, q, d, tmax)), first)
    assert (r.castsAny(sc, q, d, tmax) == (any_.view(np.int32)[:, 7] >= 0)).all()


def test_an_empty_scene_gives_the_miss_record(renderer, batch):
    sc = drt.Scene()
    sc.addMaterial(*ONE_MATERIAL[0])
    sc.setGeometry(np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 2), np.float32), np.zeros(0, np.int32))
    drt.BVHBuilder().buildIterative(sc)
    q, d, tmax = batch[2], batch[3], batch[4]
    miss = np.zeros((len(q), 12), np.float32)
    miss[:, 3], miss.view(np.int32)[:, 7], miss.view(np.int32)[:, 10] = tmax, -1, -1
    for mode in (tc.FIRST, tc.ANY):
        assert same(run_raw(renderer, sc, q, d, tmax, mode), miss)
    assert not renderer.castsAny(sc, q, d, 1e30).any() and renderer.meshCast(sc, q, d[0]).prim == -1


def test_error_paths(renderer, batch):
    sc, g, ref_q, ref_d, ref_tmax, first, any_ = batch
    dev = torch.device(DEV)
    n = 64
    tris = torch.zeros((n + 1, 12), dtype=torch.float32, device=dev)
    tris[:, 3], tris[:, 7] = 1, 1                                                # (0, 0, 0), (1, 0, 0), (0, 1, 0)
    mo = torch.ones((n + 1, 4), dtype=torch.float32, device=dev)
    dirs = mo[:, 0:3].contiguous()
    out = torch.full((n + 2, 12), SENTINEL, dtype=torch.float32, device=dev)
    host = np.zeros((n + 2, 12), np.float32)
    INV = drt.ERR_INVALID
    B, M, O, H = tris.data_ptr(), mo.data_ptr(), out.data_ptr(), host.ctypes.data
    L = drt._lib
    fn = lambda r, s, *a: L.drt_renderer_triangle_cast(r, s, *a, None)
    h = renderer._h
    for what, args in (("null tris", (h, sc._h, None, M, O, n, 0)), ("null motions", (h, sc._h, B, None, O, n, 0)), ("null out", (h, sc._h, B, M, None, n, 0)),
                       ("null renderer", (None, sc._h, B, M, O, n, 0)), ("null scene", (h, None, B, M, O, n, 1)),
                       ("mode 2", (h, sc._h, B, M, O, n, 2)), ("mode -1", (h, sc._h, B, M, O, n, -1)), ("mode 2, n = 0", (h, sc._h, B, M, O, 0, 2)),
                       ("mode 2, null tris", (h, sc._h, None, M, O, n, 2)),
                       ("misaligned tris", (h, sc._h, B + 4, M, O, n, 0)), ("misaligned out", (h, sc._h, B, M, O + 8, n, 0)),
                       ("misaligned motions", (h, sc._h, B, M + 8, O, n, 0)),
                       ("host tris", (h, sc._h, H, M, O, n, 0)), ("host motions", (h, sc._h, B, H, O, n, 1)), ("host out", (h, sc._h, B, M, H, n, 0)),
                       ("null handles, n = 0", (None, None, B, M, O, 0, 0))):
        assert fn(*args) == INV, what
        if what.startswith("mode"):
            assert b"mode" in L.drt_last_error(), what                                                    # checked first after the handles
    for mode in (0, 1):
        assert fn(h, sc._h, None, None, None, 0, mode) == drt.OK                                          # n == 0: nothing to do
        assert fn(h, sc._h, B, M, O, 0, mode) == drt.OK
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()                                                                         # nothing was launched
    # all three need 16-byte alignment: one triangle, one motion and one record further on
    assert fn(h, sc._h, B + 48, M + 16, O + 48, n, 0) == drt.OK
    torch.cuda.synchronize()
    assert (out[0] == SENTINEL).all() and (out[n + 1] == SENTINEL).all() and not (out[1:n + 1, 3] == SENTINEL).any()
    empty = renderer.triangleCast(sc, np.zeros((0, 3, 3), np.float32), np.float32([0, 0, 1]))
    assert empty.t.shape == (0,) and empty.point.shape == (0, 3) and renderer.castsAny(sc, np.zeros((0, 12), np.float32), np.float32([0, 0, 1])).shape == (0,)
    tm = torch.ones(n + 1, dtype=torch.float32, device=dev)
    for bad in (lambda: renderer.triangleCast(sc, tris.cpu(), dirs),                                      # wrong device
                lambda: renderer.triangleCast(sc, tris.double(), dirs),                                   # wrong dtype
                lambda: renderer.triangleCast(sc, tris[:, :9], dirs),                                     # [N, 9] is neither form
                lambda: renderer.triangleCast(sc, tris, dirs[:5]),                                        # one direction per triangle, or one
                lambda: renderer.triangleCast(sc, tris, dirs.cpu().numpy()),                              # mix of numpy and torch
                lambda: renderer.triangleCast(sc, tris, dirs.double()),
                lambda: renderer.triangleCast(sc, tris, 1.0),
                lambda: renderer.triangleCast(sc, tris, dirs, tm[:5]),                                    # one tmax per triangle, or a scalar
                lambda: renderer.triangleCast(sc, tris, dirs, tm.double()),
                lambda: renderer.triangleCast(sc, tris, dirs, "far"),
                lambda: renderer.castsAny(sc, host.astype(np.float64), np.float32([0, 0, 1])),
                lambda: renderer.meshCast(sc, tris[:, :11], dirs[0])):
        with pytest.raises(drt.DrtError) as e:
            bad()
        assert e.value.code == INV
    # a pending asynchronous batch
    r = drt.Renderer(0)
    r.ResizeBuffer(64, 32)
    r.RenderBatchAsync(drt.Camera(SCENES["cornell_box"][1]), sc, 1)
    for call in (lambda: r.triangleCast(sc, tris, dirs), lambda: r.castsAny(sc, tris, dirs), lambda: r.meshCast(sc, tris, dirs[0])):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == INV
    assert raw(r, sc, tris, mo, out, n, 0) == INV
    r.Wait()
    r.triangleCast(sc, tris, dirs), r.castsAny(sc, tris, dirs)
    # a tree deeper than 64 levels: the chain's centroids double per triangle (scaled down so that no area overflows)
    chain = list(rq.degenerate_chain(110))
    chain[0] = (chain[0] * np.float32(2.0 ** -55)).astype(np.float32)
    deep, _ = rq.programmatic_scene(drt, *chain, 1, 2)
    assert deep.bvh_depth > 64
    for call in (lambda: renderer.triangleCast(deep, tris, dirs), lambda: renderer.castsAny(deep, tris, dirs)):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == drt.ERR_UNSUPPORTED
    assert same(fields(renderer.triangleCast(sc, ref_q, ref_d, ref_tmax)), first)                         # after the errors
