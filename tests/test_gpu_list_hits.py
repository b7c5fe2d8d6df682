"""Ordered hit lists on the GPU (drt_renderer_list_hits, kernel_list_hits.hip; Renderer.firstHits / listHits): every slot of every
segment bit-equal to the restatement in tests/hits_ref.py, miss-filled slots included -- over scenes with ties, inserts in the
middle, evictions, a cut-out material and a tree deeper than the LDS stack, capacities, batch shapes, a refitted device copy and the
torch path -- nothing written outside the segments, the renderer's state untouched, and the error codes of include/drt.h.
tests/test_list_hits_ref.py asserts what these inputs contain."""
import numpy as np
import pytest

import oracle
from tests import hits_ref as hr
from tests import inside_ref as ir
from tests import ray_query_ref as rq
from tests.scenes import SCENES, scene_path

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FIELDS = ("t", "prim", "u", "v")
SENTINEL = -7.5
_scenes, _refs = {}, {}


@pytest.fixture(scope="module")
def renderer():
    return drt.Renderer(0)


def scene_pair(name):
    """(product scene, oracle scene) with the same tree, as tests/hits_ref.py describes them."""
    if name not in _scenes:
        if name == "cornell_box":
            sc = drt.Scene()
            sc.loadGLTFmodel(scene_path(name))
            b = drt.BVHBuilder()
            b.m_TargetLeafPrimitivesCount, b.m_BinCount = hr.CORNELL_TREE
            b.buildIterative(sc)
            _scenes[name] = (sc, hr.oracle_scene(name))
        else:
            make, leaf, bins = hr.GEOMETRY[name]
            _scenes[name] = rq.programmatic_scene(drt, *make(), leaf, bins)
    return _scenes[name]


def reference(name):
    """(org, dirs, tmin, tmax, n_plain, records, totals) of the scene's ray set: one traversal of the restatement, shared."""
    if name not in _refs:
        _, osc = scene_pair(name)
        org, dirs, tmin, tmax, n_plain = hr.ray_set(name, osc)
        rec = hr.records(osc, org, dirs, tmin, tmax)
        _refs[name] = (org, dirs, tmin, tmax, n_plain, rec, hr.ranks(len(org), rec)[2])
    return _refs[name]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_slots_equal(got, ref, what):
    """Bit for bit on t, prim, u, v of two tuples of arrays (any shape, the same number of slots)."""
    for f in FIELDS:
        g, r = np.ascontiguousarray(getattr(got, f)).reshape(-1), np.ascontiguousarray(getattr(ref, f)).reshape(-1)
        assert g.shape == r.shape and g.dtype == r.dtype, (what, f, g.shape, r.shape, g.dtype, r.dtype)
        bad = np.nonzero(bits(g) != bits(r))[0]
        assert len(bad) == 0, "%s: %s differs in %d of %d slots, first %d: %r vs %r" % (what, f, len(bad), len(g), bad[0], g[bad[0]], r[bad[0]])


def packed_rays(org, dirs, tmin, tmax):
    n = len(org)
    tmin, tmax = np.broadcast_to(np.float32(tmin), n), np.broadcast_to(np.float32(tmax), n)
    return np.ascontiguousarray(np.concatenate([org, tmin[:, None], dirs, tmax[:, None]], axis=1), np.float32)


def raw_list_hits(r, sc, rays, offsets, hits, capacity, counts, n, stream=None):
    """The entry point itself on device tensors (or None): the status code."""
    ptr = lambda x: None if x is None else x.data_ptr()
    return drt._lib.drt_renderer_list_hits(r._h, sc._h, ptr(rays), ptr(offsets), ptr(hits), capacity, ptr(counts), n, stream)


def slots_of(hits):
    """A [m, 4] float32 host array of drt_hit records as hits_ref.Slots."""
    hits = np.ascontiguousarray(hits)
    return hr.Slots(hits[:, 0].copy(), hits.view(np.int32)[:, 1].copy(), hits[:, 2].copy(), hits[:, 3].copy())


@pytest.mark.parametrize("name", hr.SCENE_NAMES)
def test_every_mode_is_bit_equal_to_the_restatement(renderer, name):
    sc, osc = scene_pair(name)
    org, dirs, tmin, tmax, n_plain, rec, totals = reference(name)
    n, top = len(org), int(totals.max())
    crossed = renderer.crossings(sc, org, dirs, tmin, tmax).count
    assert (crossed == totals).all()
    whole = renderer.listHits(sc, org, dirs, tmin, tmax)
    assert isinstance(whole, drt.HitList) and whole.splits.dtype == np.int32 and whole.prim.dtype == np.int32
    assert (whole.splits == np.concatenate([[0], np.cumsum(totals)])).all()
    assert_slots_equal(whole, hr.list_hits(osc, org, dirs, tmin, tmax, totals, rec)[0], name + " listHits")
    nan_ray = np.isnan(org).any(axis=1) | np.isnan(dirs).any(axis=1) | np.isnan(tmin) | np.isnan(tmax)
    assert nan_ray[n_plain:].all() and nan_ray.sum() >= 6
    for k in (1, 2, 3, 8):
        got = renderer.firstHits(sc, org, dirs, tmin, tmax, k=k)
        assert isinstance(got, drt.FirstHits) and got.t.shape == (n, k) and got.count.dtype == np.int32 and got.prim.dtype == np.int32
        ref, _ = hr.list_hits(osc, org, dirs, tmin, tmax, k, rec)
        assert_slots_equal(got, ref, "%s firstHits k = %d" % (name, k))
        assert (got.count == totals).all() and (got.count.view(np.uint32) == crossed).all()
        assert not got.count[nan_ray].any() and (got.prim[nan_ray] == -1).all()                # NaN rays list nothing
        # the prefix property on the device's own output: a row is the first min(k, count) records of listHits
        j = np.arange(k)[None, :]
        stored = j < np.minimum(k, got.count)[:, None]
        idx = (whole.splits[:-1, None] + j)[stored]
        for f in FIELDS:
            assert (bits(getattr(got, f)[stored]) == bits(getattr(whole, f)[idx])).all(), (name, k, f)
        assert (got.prim[~stored] == -1).all() and (bits(got.t[~stored]) == bits(np.broadcast_to(tmax[:, None], (n, k))[~stored])).all()
    # the raw entry point with ragged capacities 0 .. max total + 2, zeros included
    rng = np.random.default_rng(3)
    caps = rng.integers(0, top + 3, n)
    caps[rng.integers(0, n, n // 8)] = 0
    assert (caps == 0).sum() >= n // 16 and caps.max() == top + 2 and (caps < totals).any() and (caps > totals).any()
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(caps)]).astype(np.int32)).to(DEV)
    rays = torch.from_numpy(packed_rays(org, dirs, tmin, tmax)).to(DEV)
    hits = torch.full((int(caps.sum()), 4), SENTINEL, dtype=torch.float32, device=DEV)
    counts = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    assert raw_list_hits(renderer, sc, rays, offsets, hits, len(hits), counts, n) == drt.OK
    torch.cuda.synchronize()
    assert_slots_equal(slots_of(hits.cpu().numpy()), hr.list_hits(osc, org, dirs, tmin, tmax, caps, rec)[0], name + " ragged capacities")
    assert (counts.cpu().numpy() == totals).all()
    # a pure count, and hits without counts
    counts.fill_(-1)
    assert raw_list_hits(renderer, sc, rays, offsets, None, 0, counts, n) == drt.OK
    again = torch.full_like(hits, SENTINEL)
    assert raw_list_hits(renderer, sc, rays, offsets, again, len(again), None, n) == drt.OK
    torch.cuda.synchronize()
    assert (counts.cpu().numpy() == totals).all() and torch.equal(again.view(torch.int32), hits.view(torch.int32))
    # packed rays, and the default interval (0, +inf)
    assert_slots_equal(renderer.firstHits(sc, packed_rays(org, dirs, tmin, tmax), k=3), hr.list_hits(osc, org, dirs, tmin, tmax, 3, rec)[0], name + " packed")
    m = 300
    ref, ref_totals = hr.list_hits(osc, org[:m], dirs[:m], 0.0, np.inf, 2)
    got = renderer.firstHits(sc, org[:m], dirs[:m], k=2)
    assert_slots_equal(got, ref, name + " default interval")
    assert (got.count == ref_totals).all()
    whole = renderer.listHits(sc, org[:m], dirs[:m])
    assert_slots_equal(whole, hr.list_hits(osc, org[:m], dirs[:m], 0.0, np.inf, ref_totals)[0], name + " default interval, listHits")


@pytest.fixture(scope="module")
def batch():
    """2 000 rays on the torus and their table at k = 6 (no ray passes through more), the reference made 1 000 rays at a time."""
    sc, osc = scene_pair("torus")
    rng = np.random.default_rng(21)
    org, dirs = rq.surface_rays(osc, 1300, rng)
    o2, d2 = rq.box_rays(osc, 700, rng)
    org, dirs = np.concatenate([org, o2]), np.concatenate([dirs, d2])
    k = 6
    parts = [hr.list_hits(osc, org[s:s + 1000], dirs[s:s + 1000], 0.0, np.inf, k) for s in (0, 1000)]
    table = hr.Slots(*[np.concatenate([p[0][i].reshape(-1, k) for p in parts]) for i in range(4)])
    totals = np.concatenate([p[1] for p in parts])
    assert totals.max() <= k and totals.max() >= 3 and (totals == 0).any()
    return sc, packed_rays(org, dirs, 0.0, np.inf), k, table, totals


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2000])
def test_batch_sizes(renderer, batch, n):
    sc, rays, k, table, totals = batch
    for sl in (slice(0, n), slice(2000 - n, 2000)):
        got = renderer.firstHits(sc, rays[sl], k=k)
        assert_slots_equal(got, hr.Slots(*[f[sl] for f in table]), "firstHits %r" % (sl,))
        assert (got.count == totals[sl]).all()
        whole = renderer.listHits(sc, rays[sl])
        stored = np.arange(k)[None, :] < totals[sl][:, None]
        assert (whole.splits == np.concatenate([[0], np.cumsum(totals[sl])])).all()
        assert_slots_equal(whole, hr.Slots(*[f[sl][stored] for f in table]), "listHits %r" % (sl,))


def _records(res):
    """FirstHits / HitList device tensors as one int32 tensor [..., 4]."""
    return torch.stack([res.t.view(torch.int32), res.prim, res.u.view(torch.int32), res.v.view(torch.int32)], dim=-1)


def test_a_batch_beyond_the_grid_a_permutation_and_a_second_run(renderer, batch):
    sc, rays, k6, table, totals = batch
    tiles, k = 300, 4                           # 600 000 rays: more than the persistent grid has threads, so lanes are refilled
    assert tiles * len(rays) > torch.cuda.get_device_properties(0).multi_processor_count * 2048
    dev_rays = torch.from_numpy(rays).to(DEV).repeat(tiles, 1)
    want = np.stack([bits(getattr(table, f)[:, :k]).view(np.int32) for f in FIELDS], axis=-1)
    # (a row of the k = 6 table cut to 4 is the list at capacity 4: slots beyond the total hold the miss record in both)
    want = torch.from_numpy(np.ascontiguousarray(want)).to(DEV).repeat(tiles, 1, 1)
    res = renderer.firstHits(sc, dev_rays, k=k)
    got = _records(res)
    bad = (got != want).any(dim=2).any(dim=1)
    assert not bad.any(), "%d of %d rows differ from the tiled reference, first %d" % (bad.sum(), len(bad), bad.nonzero()[0])
    assert res.count.dtype == torch.int32 and torch.equal(res.count, torch.from_numpy(totals.view(np.int32)).to(DEV).repeat(tiles))
    assert torch.equal(_records(renderer.firstHits(sc, dev_rays, k=k)), got)                                 # two runs: identical bytes
    perm = torch.from_numpy(np.random.default_rng(2).permutation(len(dev_rays))).to(DEV)
    shuffled = renderer.firstHits(sc, dev_rays[perm], k=k)
    assert torch.equal(_records(shuffled), got[perm]) and torch.equal(shuffled.count, res.count[perm])


def test_nothing_outside_the_segments_is_written(renderer, batch):
    sc, rays, k6, table, totals = batch
    _, osc = scene_pair("torus")
    n = 600
    org, dirs = rays[:n, 0:3], rays[:n, 4:7]
    rec = hr.records(osc, org, dirs, 0.0, np.inf)
    dev_rays = torch.from_numpy(rays[:n]).to(DEV)
    rng = np.random.default_rng(9)
    caps = rng.integers(0, 7, n)
    lead, trail = 7, 9
    off = lead + np.concatenate([[0], np.cumsum(caps)])
    offsets = torch.from_numpy(off.astype(np.int32)).to(DEV)
    sentinel_bits = np.float32(SENTINEL).view(np.uint32)

    def run(offsets, size, capacity):
        hits = torch.full((size, 4), SENTINEL, dtype=torch.float32, device=DEV)
        counts = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        assert raw_list_hits(renderer, sc, dev_rays, offsets, hits, capacity, counts, n) == drt.OK
        torch.cuda.synchronize()
        assert (counts.cpu().numpy() == totals[:n]).all()                       # the totals, whatever the capacities
        return hits.cpu().numpy()

    # records before offsets[0] and from offsets[n] on are untouched
    size = int(off[-1]) + trail
    h = run(offsets, size, size)
    assert (bits(h[:lead]) == sentinel_bits).all() and (bits(h[off[-1]:]) == sentinel_bits).all()
    assert_slots_equal(slots_of(h[lead:off[-1]]), hr.list_hits(osc, org, dirs, 0.0, np.inf, caps, rec)[0], "offset segments")
    # a capacity stated smaller than the last offsets, ending inside a segment: the records at and beyond it are untouched (the
    # tensor is as large as the unclamped offsets need, so nothing can leave the allocation)
    i = int(np.nonzero((caps >= 2) & (np.arange(n) > n // 2))[0][0])
    stated = int(off[i]) + 1
    h = run(offsets, size, stated)
    assert (bits(h[stated:]) == sentinel_bits).all() and (bits(h[:lead]) == sentinel_bits).all()
    clamped = np.clip(np.minimum(caps, stated - off[:-1]), 0, None)
    assert clamped[i] == 1 and not clamped[i + 1:].any() and (clamped[:i] == caps[:i]).all()
    assert_slots_equal(slots_of(h[lead:stated]), hr.list_hits(osc, org, dirs, 0.0, np.inf, clamped, rec)[0], "stated capacity")
    # decreasing pairs of offsets give capacity 0: even rays own four slots each in blocks that descend through the array, so
    # offsets[i + 1] < offsets[i] for every odd ray, and no two segments overlap
    b = 8 * (n // 2 - np.arange(n // 2 + 1))
    down = np.empty(n + 1, np.int64)
    down[0::2], down[1::2] = b, b[:-1] + 4
    assert down[-1] == 0 and (down[2::2] < down[1::2]).all()
    size = int(down.max()) + 8
    h = run(torch.from_numpy(down.astype(np.int32)).to(DEV), size, size)
    even = np.where(np.arange(n) % 2 == 0, 4, 0)
    ref = hr.list_hits(osc, org, dirs, 0.0, np.inf, even, rec)[0]
    owned = (down[0:n:2, None] + np.arange(4)[None, :]).reshape(-1)
    assert_slots_equal(slots_of(h[owned]), ref, "descending blocks")
    rest = np.ones(size, bool)
    rest[owned] = False
    assert (bits(h[rest]) == sentinel_bits).all()


def test_after_a_refit_the_moved_mesh_answers(renderer):
    def load():
        return rq.programmatic_scene(drt, *ir.streams(ir.torus()), 4, 8)[0]

    sc, host = load(), load()
    moved = (ir.torus() * np.float32([1.25, 0.75, 1.5]) + np.float32([0.125, 0, -0.25])).astype(np.float32)
    host.refit(moved)                                          # the host scene refitted with the same positions
    old, new = ir.product_scene(sc), ir.product_scene(host)
    rng = np.random.default_rng(4)
    o1, d1 = rq.surface_rays(old, 400, rng)
    o2, d2 = rq.surface_rays(new, 400, rng)
    org, dirs = np.concatenate([o1, o2]), np.concatenate([d1, d2])
    ref_old, tot_old = hr.list_hits(old, org, dirs, 0.0, np.inf, 3)
    ref_new, tot_new = hr.list_hits(new, org, dirs, 0.0, np.inf, 3)
    assert (tot_old != tot_new).mean() > 0.05
    r = drt.Renderer(0)
    got = r.firstHits(sc, org, dirs, k=3)
    assert_slots_equal(got, ref_old, "before the refit")
    r.refit(sc, torch.from_numpy(moved).to(DEV))
    got = r.firstHits(sc, org, dirs, k=3)
    assert_slots_equal(got, ref_new, "after the refit")
    assert (got.count == tot_new).all()
    whole = r.listHits(sc, org, dirs)
    assert (whole.splits == np.concatenate([[0], np.cumsum(tot_new)])).all()
    assert_slots_equal(whole, hr.list_hits(new, org, dirs, 0.0, np.inf, tot_new)[0], "listHits after the refit")
    got = renderer.firstHits(sc, org, dirs, k=3)
    assert_slots_equal(got, ref_old, "a renderer that was not refitted")
    assert (got.count == tot_old).all()
    assert_slots_equal(r.firstHits(sc, org, dirs, k=3), ref_new, "after the other renderer's query")


def test_torch_path_stays_on_the_device_and_orders_with_the_stream(renderer):
    sc, osc = scene_pair("torus")
    dev = torch.device(DEV)
    org, dirs = rq.surface_rays(osc, 1500, np.random.default_rng(12))
    rec = hr.records(osc, org, dirs, 0.0, np.inf)
    totals = hr.ranks(len(org), rec)[2]
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        o = torch.from_numpy(org).to(dev)
        d = torch.from_numpy(dirs).to(dev)
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(2000000)                  # the inputs' producer is still busy when the queries are enqueued
        first = renderer.firstHits(sc, o * 1.0, d * 1.0, k=2)
        whole = renderer.listHits(sc, o * 1.0, d * 1.0)
        t_copy = first.t.clone()
    assert all(x.device == dev for x in first) and all(x.device == dev for x in whole)
    assert first.t.dtype == torch.float32 and first.prim.dtype == torch.int32 and first.count.dtype == torch.int32 and tuple(first.t.shape) == (1500, 2)
    assert whole.splits.dtype == torch.int32 and whole.prim.dtype == torch.int32 and tuple(whole.splits.shape) == (1501,)
    s.synchronize()
    ref = hr.list_hits(osc, org, dirs, 0.0, np.inf, 2, rec)[0]
    assert_slots_equal(hr.Slots(*[getattr(first, f).cpu().numpy() for f in FIELDS]), ref, "device tensors, firstHits")
    assert (bits(t_copy.cpu().numpy().reshape(-1)) == bits(ref.t)).all() and (first.count.cpu().numpy() == totals).all()
    assert (whole.splits.cpu().numpy() == np.concatenate([[0], np.cumsum(totals)])).all()
    assert_slots_equal(hr.Slots(*[getattr(whole, f).cpu().numpy() for f in FIELDS]), hr.list_hits(osc, org, dirs, 0.0, np.inf, totals, rec)[0], "device tensors, listHits")


def test_queries_leave_the_renderer_alone_and_work_on_a_sharded_one(renderer):
    sc, osc = scene_pair("cornell_box")
    org, dirs, tmin, tmax, n_plain, rec, totals = reference("cornell_box")
    _, pos, fwd, depth = SCENES["cornell_box"]
    cam = drt.Camera(pos)
    cam.m_Forward_dir = np.array(fwd, np.float32)
    ref = hr.list_hits(osc, org, dirs, tmin, tmax, 3, rec)[0]
    ref_all = hr.list_hits(osc, org, dirs, tmin, tmax, totals, rec)[0]
    images = []
    for with_queries in (False, True):
        r = drt.Renderer(0)
        r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=depth)
        r.ResizeBuffer(96, 64)
        r.Render(cam, sc)
        if with_queries:
            info, frame, accum, n, span = r.kernelInfo(), r.GetRenderTargetImage(), r.GetAccumulationBuffer(), r.getSampleCount(), r.kernelSpanMs()
            assert_slots_equal(r.firstHits(sc, org, dirs, tmin, tmax, k=3), ref, "between two renders")
            assert_slots_equal(r.listHits(sc, org, dirs, tmin, tmax), ref_all, "between two renders")
            assert r.kernelInfo() == info and r.getSampleCount() == n and r.kernelSpanMs() == span
            assert r.GetRenderTargetImage().tobytes() == frame.tobytes() and r.GetAccumulationBuffer().tobytes() == accum.tobytes()
        r.Render(cam, sc)
        images.append((r.GetRenderTargetImage(), r.getSampleCount()))
    assert images[0][0].tobytes() == images[1][0].tobytes() and images[0][1] == images[1][1]
    r = drt.Renderer(0)
    r.setShard(8, 1, 2)
    r.ResizeBuffer(96, 64)
    got = r.firstHits(sc, org, dirs, tmin, tmax, k=3)
    assert_slots_equal(got, ref, "sharded renderer")
    assert (got.count == totals).all()
    assert_slots_equal(r.listHits(sc, org, dirs, tmin, tmax), ref_all, "sharded renderer")


def test_an_empty_scene_lists_nothing(renderer):
    sc = drt.Scene()
    sc.addMaterial((0.8, 0.8, 0.8), -1)
    sc.setGeometry(np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 2), np.float32), np.zeros(0, np.int32))
    drt.BVHBuilder().buildIterative(sc)
    org = np.random.default_rng(0).normal(size=(500, 3)).astype(np.float32)
    org[7, 1] = np.nan
    dirs = np.tile(ir.DIRS[0], (500, 1))
    tmax = np.random.default_rng(1).uniform(1, 9, 500).astype(np.float32)
    got = renderer.firstHits(sc, org, dirs, 0.0, tmax, k=3)
    assert not got.count.any() and (got.prim == -1).all() and not got.u.any() and not got.v.any()
    assert (bits(got.t) == bits(np.repeat(tmax[:, None], 3, axis=1))).all()                 # the ray's own tmax word
    whole = renderer.listHits(sc, org, dirs, 0.0, tmax)
    assert whole.splits.shape == (501,) and not whole.splits.any() and all(len(getattr(whole, f)) == 0 for f in FIELDS)
    assert whole.t.dtype == np.float32 and whole.prim.dtype == np.int32


def test_error_paths(renderer):
    sc, osc = scene_pair("cornell_box")
    dev = torch.device(DEV)
    n = 64
    rays = torch.zeros((n + 1, 8), dtype=torch.float32, device=dev)
    rays[:, 4] = 1
    offsets = (torch.arange(n + 2, dtype=torch.int32, device=dev) * 2)
    hits = torch.full((2 * n + 8, 4), SENTINEL, dtype=torch.float32, device=dev)
    counts = torch.full((n + 1,), -1, dtype=torch.int32, device=dev)
    host = np.zeros((2 * n + 8, 8), np.float32)
    L, h = drt._lib, renderer._h
    INV = drt.ERR_INVALID
    cap = 2 * n
    R, O, H, C = rays.data_ptr(), offsets.data_ptr(), hits.data_ptr(), counts.data_ptr()
    for what, args in (("null rays", (h, sc._h, None, O, H, cap, C, n)), ("null offsets", (h, sc._h, R, None, H, cap, C, n)),
                       ("null renderer", (None, sc._h, R, O, H, cap, C, n)), ("null scene", (h, None, R, O, H, cap, C, n)),
                       ("both outputs null", (h, sc._h, R, O, None, 0, None, n)), ("null hits with a capacity", (h, sc._h, R, O, None, cap, C, n)),
                       ("hits without a capacity", (h, sc._h, R, O, H, 0, C, n)),
                       ("misaligned rays", (h, sc._h, R + 4, O, H, cap, C, n)), ("misaligned hits", (h, sc._h, R, O, H + 8, cap, C, n)),
                       ("misaligned offsets", (h, sc._h, R, O + 2, H, cap, C, n)), ("misaligned counts", (h, sc._h, R, O, H, cap, C + 1, n)),
                       ("host rays", (h, sc._h, host.ctypes.data, O, H, cap, C, n)), ("host offsets", (h, sc._h, R, host.ctypes.data, H, cap, C, n)),
                       ("host hits", (h, sc._h, R, O, host.ctypes.data, cap, C, n)), ("host counts", (h, sc._h, R, O, H, cap, host.ctypes.data, n)),
                       ("null handles, n = 0", (None, None, R, O, H, cap, C, 0))):
        assert L.drt_renderer_list_hits(*args, None) == INV, what
    assert L.drt_renderer_list_hits(h, sc._h, None, None, None, 0, None, 0, None) == drt.OK                 # n == 0: nothing to do
    assert L.drt_renderer_list_hits(h, sc._h, R, O, H, cap, C, 0, None) == drt.OK
    torch.cuda.synchronize()
    assert (hits == SENTINEL).all() and (counts == -1).all()                                               # nothing was launched
    # offsets and counts need 4-byte alignment only, hits 16: one record and one word further on
    assert L.drt_renderer_list_hits(h, sc._h, R, O + 4, H + 16, cap + 2, C + 4, n, None) == drt.OK
    torch.cuda.synchronize()
    assert (hits[0] == SENTINEL).all() and (hits[1 + 2 + 2 * n:] == SENTINEL).all() and not (hits[1 + 2:1 + 2 + 2 * n] == SENTINEL).any()
    assert counts[0] == -1 and (counts[1:] >= 0).all()
    assert len(renderer.firstHits(sc, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)).count) == 0
    assert renderer.firstHits(sc, np.zeros((0, 8), np.float32), k=5).t.shape == (0, 5)
    none = renderer.listHits(sc, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    assert none.splits.tolist() == [0] and len(none.t) == 0
    for bad in (lambda: renderer.firstHits(sc, rays, k=0),
                lambda: renderer.firstHits(sc, rays, k=-3),
                lambda: renderer.firstHits(sc, rays.cpu()),                                              # wrong device
                lambda: renderer.firstHits(sc, rays.double()),                                           # wrong dtype
                lambda: renderer.firstHits(sc, rays[:, :5]),                                             # wrong shape
                lambda: renderer.firstHits(sc, rays[:, :3], rays[:10, 4:7]),                             # mismatched counts
                lambda: renderer.firstHits(sc, rays[:, :3].cpu().numpy(), rays[:, 4:7]),                 # numpy mixed with device tensors
                lambda: renderer.firstHits(sc, rays, tmax=1.0),                                          # packed rays carry their interval
                lambda: renderer.listHits(sc, rays.cpu()),
                lambda: renderer.listHits(sc, rays.double()),
                lambda: renderer.listHits(sc, rays[:, :5]),
                lambda: renderer.listHits(sc, rays[:, :3].cpu().numpy(), rays[:, 4:7]),
                lambda: renderer.listHits(sc, rays, tmin=0.5),
                lambda: renderer.listHits(sc, host.astype(np.float64))):
        with pytest.raises(drt.DrtError) as e:
            bad()
        assert e.value.code == INV
    # a pending asynchronous batch
    r = drt.Renderer(0)
    r.ResizeBuffer(64, 32)
    r.RenderBatchAsync(drt.Camera(SCENES["cornell_box"][1]), sc, 1)
    for call in (lambda: r.firstHits(sc, rays), lambda: r.listHits(sc, rays)):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == INV
    assert raw_list_hits(r, sc, rays, offsets, hits, cap, counts, n) == INV
    r.Wait()
    r.firstHits(sc, rays), r.listHits(sc, rays)
    # a 67-level tree: the chain's centroids double per triangle (scaled down so that no area overflows)
    chain = list(rq.degenerate_chain(110))
    chain[0] = (chain[0] * np.float32(2.0 ** -55)).astype(np.float32)
    deep, _ = rq.programmatic_scene(drt, *chain, 1, 2)
    assert deep.bvh_depth == 67
    for call in (lambda: renderer.firstHits(deep, rays), lambda: renderer.listHits(deep, rays)):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == drt.ERR_UNSUPPORTED
    org, dirs, tmin, tmax, n_plain, rec, totals = reference("cornell_box")
    assert_slots_equal(renderer.firstHits(sc, org, dirs, tmin, tmax, k=2), hr.list_hits(osc, org, dirs, tmin, tmax, 2, rec)[0], "after the errors")
