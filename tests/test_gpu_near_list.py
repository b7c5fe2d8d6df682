"""Nearest-triangle lists on the GPU (drt_renderer_nearest_list, kernel_near_list.hip; Renderer.kNearest / withinRadius): every slot of
every segment, every surf word and every count bit-equal to the restatement in tests/near_list_ref.py, miss-filled slots included --
over scenes with ties, inserts in the middle, evictions and a tree deeper than the LDS stack, both modes, capacities, radii, batch
shapes, a refitted device copy and the torch path -- nothing written outside the segments, the renderer's state untouched, and the
error codes of include/drt.h.  tests/test_near_list_ref.py asserts what the restatement does on inputs like these."""
import numpy as np
import pytest

import oracle
from tests import near_list_ref as nl
from tests import nearest_ref as nr
from tests import ray_query_ref as rq
from tests import refit_ref as rf
from tests.scenes import SCENES, scene_path

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -7.5
ONE_MATERIAL = [((0.8, 0.8, 0.8), -1)]
SINGLE = np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
QUAD = np.float32([[[0, 0, 0], [1, 0, 0], [1, 1, 0]], [[0, 0, 0], [1, 1, 0], [0, 1, 0]]])      # ties on the diagonal
SCENE_NAMES = ["single", "quad", "soup", "chain", "cornell_box"]
_cache = {}


@pytest.fixture(scope="module")
def renderer():
    return drt.Renderer(0)


def flat_scene(pos):
    n = len(pos)
    nrm = np.tile(np.float32([0, 0, 1]), (n, 3, 1))
    return rq.programmatic_scene(drt, pos, nrm, np.zeros((n, 3, 2), np.float32), np.zeros(n, np.int32), ONE_MATERIAL, [], 20, 8)


def scene_pair(name):
    """(product scene, Geometry of the oracle's scene) with the same tree: one triangle, the quad, the soup of 3000 triangles with two
    per leaf, the chain whose 43 levels outgrow the 8 stack levels in LDS, cornell_box with the editor's tree."""
    if name not in _cache:
        if name in ("single", "quad"):
            sc, osc = flat_scene(SINGLE if name == "single" else QUAD)
        elif name == "soup":
            sc, osc = rq.programmatic_scene(drt, *rq.soup(3000, 5), 2, 8)
            assert sc.bvh_depth > 8
        elif name == "chain":
            sc, osc = rq.programmatic_scene(drt, *rq.degenerate_chain(), 1, 2)
            assert sc.bvh_depth == 43
        else:
            sc = drt.Scene()
            sc.loadGLTFmodel(scene_path(name))
            b = drt.BVHBuilder()
            b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
            b.buildIterative(sc)
            osc = oracle.Scene.load_glb(scene_path(name)).build_bvh(20, 8)
        _cache[name] = (sc, nr.from_oracle(osc))
    return _cache[name]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_slots_equal(got, ref, what):
    """Bit for bit on d2, prim, u, v, point and side of two Slots with the same number of slots (a NaN r2 is `some NaN`)."""
    nan = np.isnan(ref.d2)
    assert np.isnan(np.ascontiguousarray(got.d2).reshape(-1)[nan]).all(), what
    for f in nl.Slots._fields:
        g, r = np.ascontiguousarray(getattr(got, f)), np.ascontiguousarray(getattr(ref, f))
        g = g.reshape(r.shape) if g.size == r.size else g
        assert g.shape == r.shape and g.dtype == r.dtype, (what, f, g.shape, r.shape, g.dtype, r.dtype)
        diff = (bits(g) != bits(r)).reshape(len(r), g[0].size if len(r) else 1).any(axis=1)     # (an empty list: no slots)
        if f == "d2":
            diff &= ~nan
        bad = np.nonzero(diff)[0]
        assert len(bad) == 0, "%s: %s differs in %d of %d slots, first %d: %r vs %r" % (what, f, len(bad), len(r), bad[0], g[bad[0]], r[bad[0]])


def flat(res):
    """KNearest / NearList (numpy) as near_list_ref.Slots, slot after slot."""
    return nl.Slots(res.d2.reshape(-1), res.prim.reshape(-1), res.u.reshape(-1), res.v.reshape(-1), res.point.reshape(-1, 3), res.side.reshape(-1))


def slots_of(near, surf):
    """[m, 4] float32 host arrays of drt_near and drt_near_surf records as near_list_ref.Slots."""
    near, surf = np.ascontiguousarray(near), np.ascontiguousarray(surf)
    return nl.Slots(near[:, 0].copy(), near.view(np.int32)[:, 1].copy(), near[:, 2].copy(), near[:, 3].copy(), surf[:, 0:3].copy(), surf[:, 3].copy())


def packed_points(pts, radius):
    return np.ascontiguousarray(np.concatenate([pts, np.broadcast_to(np.float32(radius), len(pts))[:, None]], axis=1), np.float32)


def raw(r, sc, points, offsets, near, surf, capacity, counts, n, mode, stream=None):
    """The entry point itself on device tensors (or None): the status code."""
    ptr = lambda x: None if x is None else x.data_ptr()
    return drt._lib.drt_renderer_nearest_list(r._h, sc._h, ptr(points), ptr(offsets), ptr(near), ptr(surf), capacity, ptr(counts), n, mode, stream)


def run_raw(r, sc, pts4, offsets, size, capacity, mode, with_surf=True, with_counts=True):
    """One call on sentinel-filled buffers of `size` records: (near, surf, counts) as host arrays (None where not given)."""
    n = len(pts4)
    points = torch.from_numpy(pts4).to(DEV)
    off = torch.from_numpy(np.asarray(offsets).astype(np.int32)).to(DEV)
    near = torch.full((size, 4), SENTINEL, dtype=torch.float32, device=DEV)
    surf = torch.full((size, 4), SENTINEL, dtype=torch.float32, device=DEV) if with_surf else None
    counts = torch.full((n,), -1, dtype=torch.int32, device=DEV) if with_counts else None
    assert raw(r, sc, points, off, near, surf, capacity, counts, n, mode) == drt.OK
    torch.cuda.synchronize()
    host = lambda x: None if x is None else x.cpu().numpy()
    return host(near), host(surf), host(counts)


def sweep_points(g, n, seed, far=True):
    """About n points: near surfaces, at vertices and edge midpoints (exact ties), in the scene's box, far outside, and three with a
    NaN coordinate."""
    rng = np.random.default_rng(seed)
    q = max(n // 4, 1)
    parts = [nr.surface_points(g, q, rng), nr.tie_points(g, q, rng), nr.box_points(g, q, rng)] + ([nr.box_points(g, q, rng, 10.0)] if far else [])
    pts = np.concatenate(parts).astype(np.float32)
    bad = np.repeat(pts[:1], 3, axis=0)
    bad[np.arange(3), np.arange(3)] = np.nan
    return np.concatenate([pts, bad]).astype(np.float32)


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_both_modes_are_bit_equal_to_the_restatement(renderer, name):
    sc, g = scene_pair(name)
    pts = sweep_points(g, 240, 11, far=name != "chain")
    n = len(pts)
    lo, hi = nr.bounds(g)
    extent = float((hi - lo).max())
    rng = np.random.default_rng(5)
    scalar = {"soup": 0.06, "chain": 0.5}.get(name, 0.15) * extent                # (the soup's lists stay short enough for the restatement)
    per_point = (rng.uniform(0, 2 * scalar, n)).astype(np.float32)
    per_point[::9], per_point[4::31] = 0, np.nan                                  # nothing within 0; a NaN radius lists nothing
    # mode K through kNearest: k = 1, 2, 4, 8 at an infinite and a per-point radius, k = 4 at a scalar one
    for radius, ks, what in ((np.inf, (1, 2, 4, 8), "inf"), (per_point, (1, 2, 4, 8), "per point"), (scalar, (4,), "scalar")):
        for k in ks:
            got = renderer.kNearest(sc, pts, k=k, max_dist=radius)
            assert isinstance(got, drt.KNearest) and got.d2.shape == (n, k) and got.point.shape == (n, k, 3) and got.side.shape == (n, k)
            assert got.prim.dtype == np.int32 and got.count.dtype == np.int32
            ref, counts = nl.near_list(g, pts, radius, k, nl.K)
            assert_slots_equal(flat(got), ref, "%s kNearest k = %d, radius %s" % (name, k, what))
            assert (got.count.view(np.uint32) == counts).all()
    nan = np.isnan(pts).any(axis=1)
    assert not got.count[nan].any() and (got.prim[nan] == -1).all()             # a NaN point lists nothing
    assert_slots_equal(flat(renderer.kNearest(sc, packed_points(pts, per_point), k=2)), nl.near_list(g, pts, per_point, 2, nl.K)[0], name + " packed")
    # mode GATHER through withinRadius: a count with capacity 0, then the fill
    for radius, what in ((scalar, "scalar"), (per_point, "per point")) + (((np.inf, "inf"),) if name != "soup" else ()):
        _, totals = nl.near_list(g, pts, radius, 0, nl.GATHER)
        ref, _ = nl.near_list(g, pts, radius, totals, nl.GATHER)
        whole = renderer.withinRadius(sc, pts, radius)
        assert isinstance(whole, drt.NearList) and whole.splits.dtype == np.int32 and whole.prim.dtype == np.int32
        assert (whole.splits == np.concatenate([[0], np.cumsum(totals.astype(np.int64))])).all(), what
        assert_slots_equal(flat(whole), ref, "%s withinRadius, radius %s" % (name, what))
        assert (whole.prim >= 0).all()
        # a kNearest row whose count is below k is the point's whole list
        for k in (2, 8):
            rows = renderer.kNearest(sc, pts, k=k, max_dist=radius)
            short = np.nonzero(totals < k)[0]
            assert (rows.count[short] == totals[short]).all()
            for f in nl.Slots._fields:
                a, b = getattr(rows, f), getattr(whole, f)
                for i in short[:40]:
                    assert (bits(a[i, :totals[i]]) == bits(b[whole.splits[i]:whole.splits[i + 1]])).all(), (name, what, k, f, i)
    # the raw entry point in both modes with ragged capacities, zeros included, at the per-point radius
    _, totals = nl.near_list(g, pts, per_point, 0, nl.GATHER)
    top = int(totals.max())
    caps = rng.integers(0, top + 3, n)
    caps[rng.integers(0, n, n // 8)] = 0
    assert (caps == 0).sum() >= n // 16 and (caps > totals).any() and ((caps < totals).any() or top <= 1)
    offsets = np.concatenate([[0], np.cumsum(caps)])
    pts4 = packed_points(pts, per_point)
    for mode in (nl.GATHER, nl.K):
        ref, ref_counts = nl.near_list(g, pts, per_point, caps, mode)
        near, surf, counts = run_raw(renderer, sc, pts4, offsets, int(caps.sum()), int(caps.sum()), mode)
        assert_slots_equal(slots_of(near, surf), ref, "%s ragged capacities, mode %d" % (name, mode))
        assert (counts.view(np.uint32) == ref_counts).all()
        # surf NULL, and counts NULL: the other outputs are the same bytes
        near2, _, counts2 = run_raw(renderer, sc, pts4, offsets, int(caps.sum()), int(caps.sum()), mode, with_surf=False)
        near3, surf3, _ = run_raw(renderer, sc, pts4, offsets, int(caps.sum()), int(caps.sum()), mode, with_counts=False)
        assert near2.tobytes() == near.tobytes() and (counts2 == counts).all() and near3.tobytes() == near.tobytes() and surf3.tobytes() == surf.tobytes()
    # a pure count: capacity 0 and no near.  GATHER counts every listed triangle, K counts 0 and visits nothing
    points, off = torch.from_numpy(pts4).to(DEV), torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    for mode, want in ((nl.GATHER, totals), (nl.K, np.zeros(n, np.uint32))):
        counts = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        assert raw(renderer, sc, points, off, None, None, 0, counts, n, mode) == drt.OK
        torch.cuda.synchronize()
        assert (counts.cpu().numpy().view(np.uint32) == want).all(), mode


def test_quad_diagonal_ties_are_ordered_by_prim(renderer):
    sc, g = scene_pair("quad")
    t = np.linspace(0, 1, 33, dtype=np.float32)
    pts = np.stack([t, t, np.float32(0.5) * np.ones_like(t)], axis=1)
    two = renderer.kNearest(sc, pts, k=2)
    assert (two.d2 == 0.25).all() and (two.prim == [0, 1]).all() and (two.count == 2).all() and (two.side == 1).all()
    one = renderer.kNearest(sc, pts, k=1)
    assert (one.prim == 0).all() and (one.d2 == 0.25).all()                     # the smaller prim, whatever nearest() found first
    assert (bits(one.d2[:, 0]) == bits(renderer.nearest(sc, pts).d2)).all()
    assert_slots_equal(flat(two), nl.near_list(g, pts, np.inf, 2, nl.K)[0], "diagonal")
    whole = renderer.withinRadius(sc, pts, 0.75)
    assert whole.splits.tolist() == list(range(0, 67, 2)) and (whole.prim.reshape(-1, 2) == [0, 1]).all()


@pytest.fixture(scope="module")
def batch():
    """257 points on cornell_box with a per-point radius, their table at k = 4 and their lists within the radius."""
    sc, g = scene_pair("cornell_box")
    pts = sweep_points(g, 260, 21)[:257]
    assert len(pts) == 257
    lo, hi = nr.bounds(g)
    radius = np.random.default_rng(8).uniform(0.05, 0.4, len(pts)).astype(np.float32) * np.float32((hi - lo).max())
    table, stored = nl.near_list(g, pts, radius, 4, nl.K)
    _, totals = nl.near_list(g, pts, radius, 0, nl.GATHER)
    lists, _ = nl.near_list(g, pts, radius, totals, nl.GATHER)
    assert totals.max() > 4 and (totals == 0).any() and (totals < 4).any()
    return sc, g, pts, radius, table, stored, lists, totals


def take(s, idx):
    return nl.Slots(*[f[idx] for f in s])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(renderer, batch, n):
    sc, g, pts, radius, table, stored, lists, totals = batch
    base = np.concatenate([[0], np.cumsum(totals.astype(np.int64))])
    for sl in (slice(0, n), slice(257 - n, 257)):
        got = renderer.kNearest(sc, pts[sl], k=4, max_dist=radius[sl])
        assert_slots_equal(flat(got), take(table, slice(4 * sl.start, 4 * sl.stop)), "kNearest %r" % (sl,))
        assert (got.count.view(np.uint32) == stored[sl]).all()
        whole = renderer.withinRadius(sc, pts[sl], radius[sl])
        assert (whole.splits == base[sl.start:sl.stop + 1] - base[sl.start]).all()
        assert_slots_equal(flat(whole), take(lists, slice(base[sl.start], base[sl.stop])), "withinRadius %r" % (sl,))


def _records(res):
    """KNearest device tensors as one int32 tensor [n, k, 8]."""
    return torch.cat([torch.stack([res.d2, res.prim.view(torch.float32), res.u, res.v, res.side], dim=-1), res.point], dim=-1).view(torch.int32)


def test_a_batch_beyond_the_grid_a_permutation_and_a_second_run(renderer, batch):
    sc, g, pts, radius, table, stored, lists, totals = batch
    tiles, k = 2400, 4                          # 616 800 points: more than the persistent grid has threads, so lanes are refilled
    assert tiles * len(pts) > torch.cuda.get_device_properties(0).multi_processor_count * 2048
    dev_pts = torch.from_numpy(packed_points(pts, radius)).to(DEV).repeat(tiles, 1)
    want = np.concatenate([table.d2[:, None], table.prim.view(np.float32)[:, None], table.u[:, None], table.v[:, None], table.side[:, None],
                           table.point], axis=1).reshape(len(pts), k, 8)
    want = torch.from_numpy(np.ascontiguousarray(want).view(np.int32)).to(DEV).repeat(tiles, 1, 1)
    res = renderer.kNearest(sc, dev_pts, k=k)
    got = _records(res)
    bad = (got != want).any(dim=2).any(dim=1)
    assert not bad.any(), "%d of %d rows differ from the tiled reference, first %d" % (bad.sum(), len(bad), bad.nonzero()[0])
    assert res.count.dtype == torch.int32 and torch.equal(res.count, torch.from_numpy(stored.view(np.int32)).to(DEV).repeat(tiles))
    assert torch.equal(_records(renderer.kNearest(sc, dev_pts, k=k)), got)                                  # two runs: identical bytes
    perm = torch.from_numpy(np.random.default_rng(2).permutation(len(dev_pts))).to(DEV)
    shuffled = renderer.kNearest(sc, dev_pts[perm], k=k)
    assert torch.equal(_records(shuffled), got[perm]) and torch.equal(shuffled.count, res.count[perm])
    # mode GATHER over the same batch: the CSR of every tile is the reference's
    whole = renderer.withinRadius(sc, dev_pts[:, :3], dev_pts[:, 3].contiguous())
    per_tile = int(totals.sum())
    assert int(whole.splits[-1]) == tiles * per_tile
    ref = torch.from_numpy(np.ascontiguousarray(np.stack([lists.d2, lists.prim.view(np.float32), lists.u, lists.v, lists.side], axis=1)).view(np.int32)).to(DEV)
    rec = torch.stack([whole.d2, whole.prim.view(torch.float32), whole.u, whole.v, whole.side], dim=1).view(torch.int32).reshape(tiles, per_tile, 5)
    assert (rec == ref[None]).all() and (whole.point.reshape(tiles, per_tile, 3).view(torch.int32) == torch.from_numpy(lists.point).to(DEV).view(torch.int32)[None]).all()
    again = renderer.withinRadius(sc, dev_pts[:, :3], dev_pts[:, 3].contiguous())
    assert torch.equal(again.splits, whole.splits) and torch.equal(again.d2.view(torch.int32), whole.d2.view(torch.int32)) and torch.equal(again.prim, whole.prim)


@pytest.mark.parametrize("mode", [nl.GATHER, nl.K])
def test_nothing_outside_the_segments_is_written(renderer, batch, mode):
    sc, g, pts, radius, table, stored, lists, totals = batch
    n = len(pts)
    pts4 = packed_points(pts, radius)
    rng = np.random.default_rng(9)
    caps = rng.integers(0, 7, n)
    lead, trail = 7, 9
    off = lead + np.concatenate([[0], np.cumsum(caps)])
    sentinel_bits = np.float32(SENTINEL).view(np.uint32)

    def untouched(a, b, rows):
        return (bits(a[rows]) == sentinel_bits).all() and (bits(b[rows]) == sentinel_bits).all()

    # records before offsets[0] and from offsets[n] on are untouched, in near and in surf
    size = int(off[-1]) + trail
    near, surf, counts = run_raw(renderer, sc, pts4, off, size, size, mode)
    assert untouched(near, surf, slice(0, lead)) and untouched(near, surf, slice(int(off[-1]), None))
    ref, ref_counts = nl.near_list(g, pts, radius, caps, mode)
    assert_slots_equal(slots_of(near[lead:off[-1]], surf[lead:off[-1]]), ref, "offset segments")
    assert (counts.view(np.uint32) == ref_counts).all()
    # a capacity stated smaller than the last offsets, ending inside a segment: the records at and beyond it are untouched (the
    # tensors are as large as the unclamped offsets need, so nothing can leave the allocation)
    i = int(np.nonzero((caps >= 2) & (np.arange(n) > n // 2))[0][0])
    stated = int(off[i]) + 1
    near, surf, counts = run_raw(renderer, sc, pts4, off, size, stated, mode)
    assert untouched(near, surf, slice(stated, None)) and untouched(near, surf, slice(0, lead))
    clamped = nl.caps_of(off, stated)
    assert clamped[i] == 1 and not clamped[i + 1:].any() and (clamped[:i] == caps[:i]).all()
    ref, ref_counts = nl.near_list(g, pts, radius, clamped, mode)
    assert_slots_equal(slots_of(near[lead:stated], surf[lead:stated]), ref, "stated capacity")
    assert (counts.view(np.uint32) == ref_counts).all()
    # decreasing pairs of offsets give capacity 0: even points own four slots each in blocks that descend through the array, so
    # offsets[i + 1] < offsets[i] for every odd point, and no two segments overlap
    m = n - 1                                   # an even number of points
    b = 8 * (m // 2 - np.arange(m // 2 + 1))
    down = np.empty(m + 1, np.int64)
    down[0::2], down[1::2] = b, b[:-1] + 4
    assert down[-1] == 0 and (down[2::2] < down[1::2]).all()
    size = int(down.max()) + 8
    near, surf, counts = run_raw(renderer, sc, pts4[:m], down, size, size, mode)
    even = np.where(np.arange(m) % 2 == 0, 4, 0)
    assert (nl.caps_of(down, size) == even).all()
    owned = (down[0:m:2, None] + np.arange(4)[None, :]).reshape(-1)
    assert_slots_equal(slots_of(near[owned], surf[owned]), nl.near_list(g, pts[:m], radius[:m], even, mode)[0], "descending blocks")
    rest = np.ones(size, bool)
    rest[owned] = False
    assert untouched(near, surf, rest)


def _load(name):
    sc = drt.Scene()
    sc.loadGLTFmodel(scene_path(name))
    st = rf.streams(sc.m_PrimitivesBuffer)
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
    b.buildIterative(sc)
    return sc, st


def test_after_a_refit_the_moved_mesh_answers(renderer):
    sc, st = _load("cornell_box")
    moved = (st[0] + np.random.default_rng(1).normal(0, 0.05, st[0].shape)).astype(np.float32)
    host, _ = _load("cornell_box")
    host.refit(moved)                                          # the host scene refitted with the same positions
    g_old, g_new = nr.from_product(sc), nr.from_product(host)
    pts = np.concatenate([sweep_points(g_old, 160, 4), sweep_points(g_new, 160, 5)])
    radius = 0.6
    old, old_counts = nl.near_list(g_old, pts, radius, 3, nl.K)
    new, new_counts = nl.near_list(g_new, pts, radius, 3, nl.K)
    assert (bits(old.d2) != bits(new.d2)).mean() > 0.1
    r = drt.Renderer(0)
    assert_slots_equal(flat(r.kNearest(sc, pts, k=3, max_dist=radius)), old, "before the refit")
    r.refit(sc, torch.from_numpy(moved).to(DEV))
    got = r.kNearest(sc, pts, k=3, max_dist=radius)
    assert_slots_equal(flat(got), new, "after the refit")
    assert (got.count.view(np.uint32) == new_counts).all()
    _, totals = nl.near_list(g_new, pts, radius, 0, nl.GATHER)
    whole = r.withinRadius(sc, pts, radius)
    assert (whole.splits == np.concatenate([[0], np.cumsum(totals.astype(np.int64))])).all()
    assert_slots_equal(flat(whole), nl.near_list(g_new, pts, radius, totals, nl.GATHER)[0], "withinRadius after the refit")
    got = renderer.kNearest(sc, pts, k=3, max_dist=radius)
    assert_slots_equal(flat(got), old, "a renderer that was not refitted")
    assert (got.count.view(np.uint32) == old_counts).all()
    assert_slots_equal(flat(r.kNearest(sc, pts, k=3, max_dist=radius)), new, "after the other renderer's query")


def test_torch_path_stays_on_the_device_and_orders_with_the_stream(renderer, batch):
    sc, g, pts, radius, table, stored, lists, totals = batch
    dev = torch.device(DEV)
    n = len(pts)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        p = torch.from_numpy(pts).to(dev)
        rad = torch.from_numpy(radius).to(dev)
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(2000000)                  # the inputs' producer is still busy when the queries are enqueued
        rows = renderer.kNearest(sc, p * 1.0, k=4, max_dist=rad * 1.0)
        whole = renderer.withinRadius(sc, p * 1.0, rad * 1.0)
        packed = renderer.kNearest(sc, torch.cat([p, rad[:, None]], dim=1), k=4)
        d2_copy = rows.d2.clone()
    assert all(x.device == dev for x in rows) and all(x.device == dev for x in whole)
    assert rows.d2.dtype == torch.float32 and rows.prim.dtype == torch.int32 and rows.count.dtype == torch.int32
    assert tuple(rows.d2.shape) == (n, 4) and tuple(rows.point.shape) == (n, 4, 3) and tuple(rows.side.shape) == (n, 4)
    assert whole.splits.dtype == torch.int32 and whole.prim.dtype == torch.int32 and tuple(whole.splits.shape) == (n + 1,)
    s.synchronize()
    host = lambda res: flat(type(res)(*[x.cpu().numpy() for x in res]))
    assert_slots_equal(host(rows), table, "device tensors, kNearest")
    assert_slots_equal(host(packed), table, "packed [N, 4]")
    assert (bits(d2_copy.cpu().numpy().reshape(-1)) == bits(table.d2)).all() and (rows.count.cpu().numpy().view(np.uint32) == stored).all()
    assert (whole.splits.cpu().numpy() == np.concatenate([[0], np.cumsum(totals.astype(np.int64))])).all()
    assert_slots_equal(host(whole), lists, "device tensors, withinRadius")


def test_queries_leave_the_renderer_alone_and_work_on_a_sharded_one(renderer, batch):
    sc, g, pts, radius, table, stored, lists, totals = batch
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
            assert_slots_equal(flat(r.kNearest(sc, pts, k=4, max_dist=radius)), table, "between two renders")
            assert_slots_equal(flat(r.withinRadius(sc, pts, radius)), lists, "between two renders")
            assert r.kernelInfo() == info and r.getSampleCount() == n and r.kernelSpanMs() == span
            assert r.GetRenderTargetImage().tobytes() == frame.tobytes() and r.GetAccumulationBuffer().tobytes() == accum.tobytes()
        r.Render(cam, sc)
        images.append((r.GetRenderTargetImage(), r.getSampleCount()))
    assert images[0][0].tobytes() == images[1][0].tobytes() and images[0][1] == images[1][1]
    r = drt.Renderer(0)
    r.setShard(8, 1, 2)
    r.ResizeBuffer(96, 64)
    got = r.kNearest(sc, pts, k=4, max_dist=radius)
    assert_slots_equal(flat(got), table, "sharded renderer")
    assert (got.count.view(np.uint32) == stored).all()
    assert_slots_equal(flat(r.withinRadius(sc, pts, radius)), lists, "sharded renderer")


def test_an_empty_scene_lists_nothing(renderer):
    sc = drt.Scene()
    sc.addMaterial(*ONE_MATERIAL[0])
    sc.setGeometry(np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 2), np.float32), np.zeros(0, np.int32))
    drt.BVHBuilder().buildIterative(sc)
    pts = np.random.default_rng(0).normal(size=(500, 3)).astype(np.float32)
    pts[7, 1] = np.nan
    radius = np.random.default_rng(1).uniform(1, 9, 500).astype(np.float32)
    got = renderer.kNearest(sc, pts, k=3, max_dist=radius)
    assert not got.count.any() and (got.prim == -1).all()
    for f in (got.u, got.v, got.point, got.side):
        assert (bits(f) == 0).all()
    assert (bits(got.d2) == bits(np.repeat((radius * radius)[:, None], 3, axis=1))).all()    # the point's own product
    assert_slots_equal(flat(got), nl.near_list(nr.from_product(sc), pts, radius, 3, nl.K)[0], "empty")
    whole = renderer.withinRadius(sc, pts, radius)
    assert whole.splits.shape == (501,) and not whole.splits.any() and all(len(getattr(whole, f)) == 0 for f in nl.Slots._fields)
    assert whole.d2.dtype == np.float32 and whole.prim.dtype == np.int32 and whole.point.shape == (0, 3)


def test_error_paths(renderer, batch):
    sc, g, ref_pts, radius, table, stored, lists, totals = batch
    dev = torch.device(DEV)
    n = 64
    pts = torch.zeros((n + 1, 4), dtype=torch.float32, device=dev)
    pts[:, 3] = 1
    offsets = (torch.arange(n + 2, dtype=torch.int32, device=dev) * 2)
    near = torch.full((2 * n + 8, 4), SENTINEL, dtype=torch.float32, device=dev)
    surf = torch.full((2 * n + 8, 4), SENTINEL, dtype=torch.float32, device=dev)
    counts = torch.full((n + 1,), -1, dtype=torch.int32, device=dev)
    host = np.zeros((2 * n + 8, 8), np.float32)
    L, h = drt._lib, renderer._h
    INV = drt.ERR_INVALID
    cap = 2 * n
    P, O, N, S, C = pts.data_ptr(), offsets.data_ptr(), near.data_ptr(), surf.data_ptr(), counts.data_ptr()
    for what, args in (("null points", (h, sc._h, None, O, N, S, cap, C, n, 1)), ("null offsets", (h, sc._h, P, None, N, S, cap, C, n, 1)),
                       ("null renderer", (None, sc._h, P, O, N, S, cap, C, n, 1)), ("null scene", (h, None, P, O, N, S, cap, C, n, 0)),
                       ("mode 2", (h, sc._h, P, O, N, S, cap, C, n, 2)), ("mode -1", (h, sc._h, P, O, N, S, cap, C, n, -1)),
                       ("mode 2, n = 0", (h, sc._h, P, O, N, S, cap, C, 0, 2)), ("mode 2, null points", (h, sc._h, None, O, N, S, cap, C, n, 2)),
                       ("both outputs null", (h, sc._h, P, O, None, None, 0, None, n, 0)), ("null near with a capacity", (h, sc._h, P, O, None, S, cap, C, n, 1)),
                       ("near without a capacity", (h, sc._h, P, O, N, S, 0, C, n, 0)),
                       ("misaligned points", (h, sc._h, P + 4, O, N, S, cap, C, n, 1)), ("misaligned near", (h, sc._h, P, O, N + 8, S, cap, C, n, 1)),
                       ("misaligned surf", (h, sc._h, P, O, N, S + 8, cap, C, n, 1)),
                       ("misaligned offsets", (h, sc._h, P, O + 2, N, S, cap, C, n, 0)), ("misaligned counts", (h, sc._h, P, O, N, S, cap, C + 1, n, 0)),
                       ("host points", (h, sc._h, host.ctypes.data, O, N, S, cap, C, n, 1)), ("host offsets", (h, sc._h, P, host.ctypes.data, N, S, cap, C, n, 1)),
                       ("host near", (h, sc._h, P, O, host.ctypes.data, S, cap, C, n, 1)), ("host surf", (h, sc._h, P, O, N, host.ctypes.data, cap, C, n, 1)),
                       ("host counts", (h, sc._h, P, O, N, S, cap, host.ctypes.data, n, 0)),
                       ("null handles, n = 0", (None, None, P, O, N, S, cap, C, 0, 1))):
        assert L.drt_renderer_nearest_list(*args, None) == INV, what
        if what.startswith("mode"):
            assert b"mode" in L.drt_last_error(), what                                                    # checked first after the handles
    for mode in (0, 1):
        assert L.drt_renderer_nearest_list(h, sc._h, None, None, None, None, 0, None, 0, mode, None) == drt.OK   # n == 0: nothing to do
        assert L.drt_renderer_nearest_list(h, sc._h, P, O, N, S, cap, C, 0, mode, None) == drt.OK
    torch.cuda.synchronize()
    assert (near == SENTINEL).all() and (surf == SENTINEL).all() and (counts == -1).all()                  # nothing was launched
    # offsets and counts need 4-byte alignment only, near and surf 16: one record and one word further on
    assert L.drt_renderer_nearest_list(h, sc._h, P, O + 4, N + 16, S + 16, cap + 2, C + 4, n, 1, None) == drt.OK
    torch.cuda.synchronize()
    for buf in (near, surf):
        assert (buf[0] == SENTINEL).all() and (buf[1 + 2 + 2 * n:] == SENTINEL).all() and not (buf[1 + 2:1 + 2 + 2 * n] == SENTINEL).any()
    assert counts[0] == -1 and (counts[1:] >= 0).all()
    assert len(renderer.kNearest(sc, np.zeros((0, 3), np.float32)).count) == 0
    assert renderer.kNearest(sc, np.zeros((0, 4), np.float32), k=5).point.shape == (0, 5, 3)
    none = renderer.withinRadius(sc, np.zeros((0, 3), np.float32), 1.0)
    assert none.splits.tolist() == [0] and len(none.d2) == 0
    for bad in (lambda: renderer.kNearest(sc, pts, k=0),
                lambda: renderer.kNearest(sc, pts, k=-3),
                lambda: renderer.kNearest(sc, pts.cpu()),                                                # wrong device
                lambda: renderer.kNearest(sc, pts.double()),                                             # wrong dtype
                lambda: renderer.kNearest(sc, pts[:, :2]),                                               # wrong shape
                lambda: renderer.kNearest(sc, pts[:, :3], max_dist=pts[:10, 3]),                         # mismatched counts
                lambda: renderer.kNearest(sc, pts[:, :3].cpu().numpy(), max_dist=pts[:, 3]),             # numpy mixed with device tensors
                lambda: renderer.kNearest(sc, pts, max_dist=1.0),                                        # packed points carry max_dist
                lambda: renderer.withinRadius(sc, pts.cpu(), 1.0),
                lambda: renderer.withinRadius(sc, pts.double(), 1.0),
                lambda: renderer.withinRadius(sc, pts[:, :2], 1.0),
                lambda: renderer.withinRadius(sc, pts[:, :3], pts[:10, 3]),
                lambda: renderer.withinRadius(sc, pts, 1.0),
                lambda: renderer.withinRadius(sc, host[:, :3].astype(np.float64), 1.0)):
        with pytest.raises(drt.DrtError) as e:
            bad()
        assert e.value.code == INV
    # a pending asynchronous batch
    r = drt.Renderer(0)
    r.ResizeBuffer(64, 32)
    r.RenderBatchAsync(drt.Camera(SCENES["cornell_box"][1]), sc, 1)
    for call in (lambda: r.kNearest(sc, pts), lambda: r.withinRadius(sc, pts[:, :3], 1.0)):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == INV
    assert raw(r, sc, pts, offsets, near, surf, cap, counts, n, 1) == INV
    r.Wait()
    r.kNearest(sc, pts), r.withinRadius(sc, pts[:, :3], 1.0)
    # a tree deeper than 64 levels: the chain's centroids double per triangle (scaled down so that no area overflows)
    chain = list(rq.degenerate_chain(110))
    chain[0] = (chain[0] * np.float32(2.0 ** -55)).astype(np.float32)
    deep, _ = rq.programmatic_scene(drt, *chain, 1, 2)
    assert deep.bvh_depth > 64
    for call in (lambda: renderer.kNearest(deep, pts), lambda: renderer.withinRadius(deep, pts[:, :3], 1.0)):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == drt.ERR_UNSUPPORTED
    assert_slots_equal(flat(renderer.kNearest(sc, ref_pts, k=4, max_dist=radius)), table, "after the errors")
