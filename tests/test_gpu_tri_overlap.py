"""Triangle overlap queries on the GPU (drt_renderer_overlap_triangles, kernel_tri_overlap.hip; Renderer.overlapTriangles / intersectsAny /
selfIntersections): every slot of every segment and every count bit-equal to the restatement in tests/tri_overlap_ref.py, -1-filled
slots included -- over one triangle, the quad, a soup, cornell_box and a tree deeper than the LDS stack, both modes, queries from a point
to a triangle across the whole scene, invalid and zero-area ones, capacities, batch shapes, a refitted device copy, the torch and the
numpy path -- nothing written outside the segments, the renderer's state untouched, and the error codes of include/drt.h.
tests/test_tri_overlap_ref.py asserts what the restatement does.

On the builder's trees a query's triangles arrive in ascending index, so here every insert is an append: the whole-scene queries at
capacities 0 to 9 exercise truncation and the -1 fill, not the insert before a stored record or the eviction.  Those run in
tests/test_tri_overlap_ref.py, over a tree with exchanged children, which the public interface cannot hand to the GPU."""
import numpy as np
import pytest

import oracle
from tests import nearest_ref as nr
from tests import ray_query_ref as rq
from tests import refit_ref as rf
from tests import tri_overlap_ref as tv
from tests.scenes import SCENES, scene_path
from tests.tri_overlap_scenes import CROSSING_PAIRS, CROSSING_QUADS, TETRAHEDRON

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -77
ONE_MATERIAL = [((0.8, 0.8, 0.8), -1)]
SINGLE = np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
QUAD = np.float32([[[0, 0, 0], [1, 0, 0], [1, 1, 0]], [[0, 0, 0], [1, 1, 0], [0, 1, 0]]])
SCENE_NAMES = ["single", "quad", "soup", "chain", "cornell_box"]
# The chain's triangle i lies in the plane x = 2^i and is 0.8 * 2^i across, so a triangle across the whole scene overflows the test's
# fourth powers and lists nothing.  These long thin ones start at x = 0.5 and reach x = 2^28 and 2^24, where every product is finite:
# they cut the 29 and 25 smallest triangles, and their stacks outgrow the 16 levels in LDS (27 and 25 entries), so records that were
# held in the HBM levels are listed.
SPEARS = np.float32([[(0.5, 0, 0), (2.0 ** e, 0, 0), (2.0 ** e, 2.0 ** (e - 2), 2.0 ** (e - 3))] for e in (28, 24)])
_cache = {}


@pytest.fixture(scope="module")
def renderer():
    return drt.Renderer(0)


def flat_scene(pos):
    n = len(pos)
    nrm = np.tile(np.float32([0, 0, 1]), (n, 3, 1))
    return rq.programmatic_scene(drt, pos, nrm, np.zeros((n, 3, 2), np.float32), np.zeros(n, np.int32), ONE_MATERIAL, [], 20, 8)


def scene_pair(name):
    """(product scene, Geometry of the oracle's scene) with the same tree, as tests/test_gpu_overlap.py builds them: one triangle, the
    quad, the soup of 3000 triangles with two per leaf, the chain whose 43 levels outgrow the 16 stack levels in LDS, cornell_box with
    the editor's tree."""
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


def sweep_queries(g, n, seed, whole=2):
    """About n queries [N, 3, 3]: small random triangles centred near surfaces, on vertices and edge midpoints and in the scene's box,
    of size U^3 * 0.3 * extent; some of the scene's own triangles; `whole` triangles across the whole scene; a segment and a point
    (zero area) on the surface; and four invalid ones with a NaN or an infinity in them."""
    rng = np.random.default_rng(seed)
    k = max(n // 3, 1)
    lo, hi = nr.bounds(g)
    extent = np.float32((hi - lo).max())
    center = np.concatenate([nr.surface_points(g, k, rng), nr.tie_points(g, k, rng), nr.box_points(g, k, rng)]).astype(np.float32)
    m = len(center)
    size = (rng.uniform(0, 1, (m, 1, 1)) ** 3 * np.float32(0.3) * extent).astype(np.float32)
    q = (center[:, None, :] + rng.uniform(-1, 1, (m, 3, 3)).astype(np.float32) * size).astype(np.float32)
    q[::9, 2] = q[::9, 1]                                                       # segments
    q[4::13, 1] = q[4::13, 0]
    q[4::13, 2] = q[4::13, 0]                                                   # points
    own = tv.scene_triangles(g)[rng.choice(len(g.v0), min(max(n // 8, 1), len(g.v0)), replace=False)]
    mid = (lo + hi) / 2
    big = np.stack([np.stack([lo - (hi - lo), mid + np.float32([0, 1, 0]) * 2 * extent, hi + (hi - lo)]),
                    np.stack([np.float32([lo[0] - extent, mid[1], mid[2] - extent]), np.float32([hi[0] + extent, mid[1], mid[2] - extent]),
                              np.float32([mid[0], mid[1], hi[2] + 2 * extent])])])[:whole].astype(np.float32)
    bad = np.repeat(own[:1], 4, axis=0)
    bad[0, 0, 1], bad[1, 1, 0], bad[2, 2, 2], bad[3, 1, 1] = np.nan, np.inf, -np.inf, np.nan
    return np.concatenate([q, own, big, bad]).astype(np.float32)


def raw(r, sc, tris, offsets, prims, capacity, counts, n, mode, stream=None):
    """The entry point itself on device tensors (or None): the status code."""
    ptr = lambda x: None if x is None else x.data_ptr()
    return drt._lib.drt_renderer_overlap_triangles(r._h, sc._h, ptr(tris), ptr(offsets), ptr(prims), capacity, ptr(counts), n, mode, stream)


def run_raw(r, sc, q, offsets, size, capacity, mode=tv.LIST, with_prims=True, with_counts=True):
    """One call on sentinel-filled buffers of `size` records: (prims, counts) as host arrays (None where not given)."""
    n = len(q)
    t = torch.from_numpy(tv.pack(q)).to(DEV)
    off = None if offsets is None else torch.from_numpy(np.asarray(offsets).astype(np.int32)).to(DEV)
    prims = torch.full((size,), SENTINEL, dtype=torch.int32, device=DEV) if with_prims else None
    counts = torch.full((n,), -1, dtype=torch.int32, device=DEV) if with_counts else None
    assert raw(r, sc, t, off, prims, capacity, counts, n, mode) == drt.OK
    torch.cuda.synchronize()
    host = lambda x: None if x is None else x.cpu().numpy()
    return host(prims), host(counts)


def csr(totals):
    return np.concatenate([[0], np.cumsum(totals.astype(np.int64))])


def reference(g, q):
    """(rows int32 [N, T], totals uint32 [N]) of one run of the restatement at capacity T = all triangles: row i is query i's whole
    list with -1 behind it.  The list at a smaller capacity is its prefix (tests/test_tri_overlap_ref.py asserts that of the
    restatement), so the tests below cut their expectations from these rows and leave them unchanged."""
    T = max(len(g.v0), 1)
    prims, totals = tv.overlap(g, q, T)
    return prims.reshape(len(q), T), totals


def cut(rows, caps):
    """The flat records of segments of `caps` slots (a scalar or [N]) from reference()'s rows."""
    n, T = rows.shape
    caps = np.broadcast_to(np.asarray(caps, np.int64), n)
    wide = np.full((n, max(T, int(caps.max()) if n else 0)), -1, np.int32)
    wide[:, :T] = rows
    return wide[np.arange(wide.shape[1])[None, :] < caps[:, None]]


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_both_modes_are_bit_equal_to_the_restatement(renderer, name):
    sc, g = scene_pair(name)
    q = sweep_queries(g, 150, 11, whole=1) if name == "soup" else sweep_queries(g, 240, 11)
    if name == "chain":
        q = np.concatenate([SPEARS, q])
    n = len(q)
    rows, totals = reference(g, q)
    whole = cut(rows, totals)
    assert name != "chain" or totals[:2].tolist() == [29, 25]
    assert (totals == 0).any() and (totals > 0).any() and not totals[-4:].any()                # nothing; something; NaN and inf
    # every triangle of every query: a count with capacity 0, the scan, the fill.  numpy in, numpy out.
    got = renderer.overlapTriangles(sc, q)
    assert isinstance(got, drt.TriList) and got.splits.dtype == np.int32 and got.prim.dtype == np.int32
    assert (got.splits == csr(totals)).all() and (got.prim == whole).all(), name
    # [N, 3, 3] and the packed [N, 12] are the same query; the pad words are ignored
    packed = tv.pack(q)
    packed[:, 9:] = np.nan
    again = renderer.overlapTriangles(sc, packed)
    assert (again.splits == got.splits).all() and (again.prim == got.prim).all()
    # tables of k slots: the first k of each list, -1 behind it, the count the total
    for k in (1, 4, 9):
        table = renderer.overlapTriangles(sc, q, k=k)
        assert isinstance(table, drt.TriTable) and table.prim.shape == (n, k) and table.prim.dtype == np.int32 and table.count.dtype == np.int32
        assert (table.prim.reshape(-1) == cut(rows, k)).all() and (table.count.view(np.uint32) == totals).all(), (name, k)
    # mode ANY is LIST's count > 0
    hit = renderer.intersectsAny(sc, q)
    assert hit.dtype == np.bool_ and hit.shape == (n,) and (hit == (totals > 0)).all()
    assert (tv.overlap(g, q, 0, tv.ANY)[1] == hit).all()
    assert (renderer.intersectsAny(sc, packed) == hit).all()
    # the raw entry point with ragged capacities, zeros included
    rng = np.random.default_rng(5)
    caps = rng.integers(0, 7, n)
    caps[rng.integers(0, n, n // 8)] = 0
    assert (caps == 0).sum() >= n // 16 and (caps > totals).any()
    offsets = csr(caps)
    prims, counts = run_raw(renderer, sc, q, offsets, int(caps.sum()), int(caps.sum()))
    assert (prims == cut(rows, caps)).all() and (counts.view(np.uint32) == totals).all()
    if name != "soup":                                                          # (the restatement itself at these capacities)
        ref, ref_counts = tv.overlap(g, q, caps)
        assert (prims == ref).all() and (counts.view(np.uint32) == ref_counts).all()
    # counts NULL: the same records
    prims2, _ = run_raw(renderer, sc, q, offsets, int(caps.sum()), int(caps.sum()), with_counts=False)
    assert prims2.tobytes() == prims.tobytes()
    # a pure count: capacity 0 and no prims; and mode ANY without offsets
    _, counts = run_raw(renderer, sc, q, np.zeros(n + 1), 0, 0, with_prims=False)
    assert (counts.view(np.uint32) == totals).all()
    _, counts = run_raw(renderer, sc, q, None, 0, 0, mode=tv.ANY, with_prims=False)
    assert (counts == (totals > 0)).all()


def test_hand_cases_zero_area_and_invalid_queries_on_one_triangle(renderer):
    """tests/test_tri_overlap_ref.py's cases against the triangle (0, 0, 0), (4, 0, 0), (0, 4, 0)."""
    T = np.float32([[[0, 0, 0], [4, 0, 0], [0, 4, 0]]])
    sc, _ = flat_scene(T)
    g = nr.from_product(sc)
    cases = [([(0, 0, 0), (-4, 0, 1), (0, -4, 1)], True), ([(0, 0, 0), (4, 0, 0), (0, 0, 4)], True),          # shared vertex, shared edge
             ([(1, 1, -1), (1, 1, 1), (5, 5, 0)], True), ([(1, 1, 0), (2, 1, 0), (1, 2, 0)], True),          # edge through, coplanar inside
             ([(3, 3, 0), (5, 3, 0), (3, 5, 0)], False), ([(0, 0, 1), (4, 0, 1), (0, 4, 1)], False),         # coplanar apart, parallel
             ([(0, 0, 0), (4, 0, 0), (0, 4, 0)], True),                                                      # itself
             ([(1, 1, -2), (1, 1, 2), (1, 1, 2)], True), ([(1, 1, 1), (2, 1, 1), (2, 1, 1)], False),         # segments: through, above
             ([(1, 1, 0)] * 3, True), ([(4, 0, 0)] * 3, True), ([(1, 1, 1)] * 3, False), ([(3, 3, 0)] * 3, False),   # points
             ([(1, 1, -1), (1, np.nan, 1), (5, 5, 0)], False), ([(1, 1, -1), (1, 1, 1), (np.inf, 5, 0)], False),     # invalid
             ([(1e30, 1e30, -1e30), (1e30, 1e30, 1e30), (5e30, 5e30, 0)], False)]                            # valid, and overflows
    q = np.float32([c for c, _ in cases])
    want = np.array([w for _, w in cases])
    assert (tv.overlap(g, q, 0)[1] == want).all()
    assert (renderer.intersectsAny(sc, q) == want).all()
    table = renderer.overlapTriangles(sc, q, k=2)
    assert (table.count == want).all() and (table.prim[:, 0] == np.where(want, 0, -1)).all() and (table.prim[:, 1] == -1).all()


@pytest.fixture(scope="module")
def batch():
    """257 queries on cornell_box, their whole lists and their tables at capacity 4."""
    sc, g = scene_pair("cornell_box")
    q = sweep_queries(g, 260, 21)[-257:]
    assert len(q) == 257
    _, totals = tv.overlap(g, q, 0)
    lists, _ = tv.overlap(g, q, totals)
    table, _ = tv.overlap(g, q, 4)
    assert totals.max() > 4 and (totals == 0).any() and ((totals > 0) & (totals < 4)).any()
    return sc, g, q, totals, lists, table


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(renderer, batch, n):
    sc, g, q, totals, lists, table = batch
    base = csr(totals)
    for sl in (slice(0, n), slice(257 - n, 257)):
        got = renderer.overlapTriangles(sc, q[sl], k=4)
        assert (got.prim.reshape(-1) == table[4 * sl.start:4 * sl.stop]).all() and (got.count.view(np.uint32) == totals[sl]).all()
        whole = renderer.overlapTriangles(sc, q[sl])
        assert (whole.splits == base[sl.start:sl.stop + 1] - base[sl.start]).all()
        assert (whole.prim == lists[base[sl.start]:base[sl.stop]]).all()
        assert (renderer.intersectsAny(sc, q[sl]) == (totals[sl] > 0)).all()


def test_about_5000_queries_a_permutation_and_a_second_run(renderer, batch):
    """20 x 257 = 5140 queries: the claim crosses shards, and waves refill lanes from more than one of them."""
    sc, g, q, totals, lists, table = batch
    tiles, k = 20, 4
    dev_q = torch.from_numpy(q).to(DEV).repeat(tiles, 1, 1)
    want = torch.from_numpy(table.reshape(-1, k)).to(DEV).repeat(tiles, 1)
    want_counts = torch.from_numpy(totals.view(np.int32)).to(DEV).repeat(tiles)
    res = renderer.overlapTriangles(sc, dev_q, k=k)
    assert res.prim.dtype == torch.int32 and torch.equal(res.prim, want) and torch.equal(res.count, want_counts)
    assert torch.equal(renderer.overlapTriangles(sc, dev_q, k=k).prim, res.prim)                   # two runs: identical bytes
    perm = torch.from_numpy(np.random.default_rng(2).permutation(len(dev_q))).to(DEV)
    shuffled = renderer.overlapTriangles(sc, dev_q[perm], k=k)
    assert torch.equal(shuffled.prim, want[perm]) and torch.equal(shuffled.count, want_counts[perm])
    assert torch.equal(renderer.intersectsAny(sc, dev_q[perm]), (want_counts > 0)[perm])
    whole = renderer.overlapTriangles(sc, dev_q)
    per_tile = int(totals.sum())
    assert int(whole.splits[-1]) == tiles * per_tile
    assert (whole.prim.reshape(tiles, per_tile) == torch.from_numpy(lists).to(DEV)[None]).all()


@pytest.mark.parametrize("name", ["cornell_box", "chain"])
def test_capacities_0_to_9_truncate_a_query_across_the_whole_scene(renderer, name):
    sc, g = scene_pair(name)
    q = SPEARS if name == "chain" else sweep_queries(g, 3, 3)[-6:-4]            # the two triangles across the whole scene
    rows, totals = reference(g, q)
    assert totals.max() > 9
    for cap in range(0, 10):
        lead = 3
        off = lead + csr(np.full(len(q), cap))
        size = int(off[-1]) + 5
        prims, counts = run_raw(renderer, sc, q, off, size, size, with_prims=True)
        assert (prims[:lead] == SENTINEL).all() and (prims[off[-1]:] == SENTINEL).all()
        assert (prims[lead:off[-1]] == cut(rows, cap)).all() and (counts.view(np.uint32) == totals).all(), cap


def test_nothing_outside_the_segments_is_written(renderer, batch):
    sc, g, q, totals, lists, table = batch
    n = len(q)
    rng = np.random.default_rng(9)
    caps = rng.integers(0, 7, n)
    lead, trail = 7, 9
    off = lead + csr(caps)
    # records before offsets[0] and from offsets[n] on are untouched
    size = int(off[-1]) + trail
    prims, counts = run_raw(renderer, sc, q, off, size, size)
    assert (prims[:lead] == SENTINEL).all() and (prims[off[-1]:] == SENTINEL).all()
    ref, ref_counts = tv.overlap(g, q, caps)
    assert (prims[lead:off[-1]] == ref).all() and (counts.view(np.uint32) == ref_counts).all()
    # a capacity stated smaller than the last offsets, ending inside a segment: the records at and beyond it are untouched (the
    # tensor is as large as the unclamped offsets need, so nothing can leave the allocation)
    i = int(np.nonzero((caps >= 2) & (np.arange(n) > n // 2))[0][0])
    stated = int(off[i]) + 1
    prims, counts = run_raw(renderer, sc, q, off, size, stated)
    assert (prims[stated:] == SENTINEL).all() and (prims[:lead] == SENTINEL).all()
    clamped = tv.caps_of(off, stated)
    assert clamped[i] == 1 and not clamped[i + 1:].any() and (clamped[:i] == caps[:i]).all()
    ref, ref_counts = tv.overlap(g, q, clamped)
    assert (prims[lead:stated] == ref).all() and (counts.view(np.uint32) == ref_counts).all()
    # decreasing pairs of offsets give capacity 0: even queries own four slots each in blocks that descend through the array
    m = n - 1                                   # an even number of queries
    b = 8 * (m // 2 - np.arange(m // 2 + 1))
    down = np.empty(m + 1, np.int64)
    down[0::2], down[1::2] = b, b[:-1] + 4
    assert down[-1] == 0 and (down[2::2] < down[1::2]).all()
    size = int(down.max()) + 8
    prims, counts = run_raw(renderer, sc, q[:m], down, size, size)
    even = np.where(np.arange(m) % 2 == 0, 4, 0)
    assert (tv.caps_of(down, size) == even).all()
    owned = (down[0:m:2, None] + np.arange(4)[None, :]).reshape(-1)
    assert (prims[owned] == tv.overlap(g, q[:m], even)[0]).all() and (counts.view(np.uint32) == totals[:m]).all()
    rest = np.ones(size, bool)
    rest[owned] = False
    assert (prims[rest] == SENTINEL).all()
    # mode ANY writes its counts and nothing else: offsets that would be wild are not read
    wild = np.full(n + 1, 2 ** 31 - 1)
    _, counts = run_raw(renderer, sc, q, wild, 0, 0, mode=tv.ANY, with_prims=False)
    assert (counts == (totals > 0)).all()


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
    q = np.concatenate([sweep_queries(g_old, 120, 4, whole=1), sweep_queries(g_new, 120, 5, whole=1)])
    old, old_counts = tv.overlap(g_old, q, 3)
    new, new_counts = tv.overlap(g_new, q, 3)
    assert (old != new).mean() > 0.02 and (old_counts != new_counts).any()
    r = drt.Renderer(0)
    got = r.overlapTriangles(sc, q, k=3)
    assert (got.prim.reshape(-1) == old).all() and (got.count.view(np.uint32) == old_counts).all()
    r.refit(sc, torch.from_numpy(moved).to(DEV))
    got = r.overlapTriangles(sc, q, k=3)
    assert (got.prim.reshape(-1) == new).all() and (got.count.view(np.uint32) == new_counts).all()
    assert (r.intersectsAny(sc, q) == (new_counts > 0)).all()
    whole = r.overlapTriangles(sc, q)
    assert (whole.splits == csr(new_counts)).all() and (whole.prim == tv.overlap(g_new, q, new_counts)[0]).all()
    # the moved mesh against itself: positions= in load order, as refit took them; the host scene's own are the old ones
    tree = lambda scene: np.ascontiguousarray(scene.m_PrimitivesBuffer["vertex"]["position"], np.float32).reshape(-1, 3, 3)
    assert (tree(host) == moved[sc.triangleOrder()]).all()
    moved_pairs = tv.self_pairs(g_new, tree(host))
    assert len(moved_pairs) > 5                                # (every vertex moved on its own: former neighbours now cut or miss)
    assert (r.selfIntersections(sc, positions=moved) == moved_pairs).all()
    got = renderer.overlapTriangles(sc, q, k=3)                # a renderer that was not refitted
    assert (got.prim.reshape(-1) == old).all() and (got.count.view(np.uint32) == old_counts).all()
    still = renderer.selfIntersections(sc)                     # the host scene's own positions: the box as it was loaded
    assert (still == tv.self_pairs(g_old, tree(sc))).all() and still.shape == (len(still), 2)


def test_torch_path_stays_on_the_device_and_orders_with_the_stream(renderer, batch):
    sc, g, q, totals, lists, table = batch
    dev = torch.device(DEV)
    n = len(q)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        dq = torch.from_numpy(q).to(dev)
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(2000000)                  # the inputs' producer is still busy when the queries are enqueued
        rows = renderer.overlapTriangles(sc, dq * 1.0, k=4)
        whole = renderer.overlapTriangles(sc, dq * 1.0)
        packed = renderer.overlapTriangles(sc, torch.from_numpy(tv.pack(q)).to(dev) * 1.0, k=4)
        hit = renderer.intersectsAny(sc, dq * 1.0)
        prim_copy = rows.prim.clone()
    assert all(x.device == dev for x in rows) and all(x.device == dev for x in whole) and hit.device == dev
    assert rows.prim.dtype == torch.int32 and rows.count.dtype == torch.int32 and hit.dtype == torch.bool
    assert tuple(rows.prim.shape) == (n, 4) and whole.splits.dtype == torch.int32 and tuple(whole.splits.shape) == (n + 1,)
    s.synchronize()
    assert (rows.prim.cpu().numpy().reshape(-1) == table).all() and (prim_copy.cpu().numpy().reshape(-1) == table).all()
    assert (packed.prim.cpu().numpy().reshape(-1) == table).all() and (rows.count.cpu().numpy().view(np.uint32) == totals).all()
    assert (whole.splits.cpu().numpy() == csr(totals)).all() and (whole.prim.cpu().numpy() == lists).all()
    assert (hit.cpu().numpy() == (totals > 0)).all()


def by_load_index(sc, pairs):
    """Pairs of tree-order triangle indices as sorted pairs of load indices."""
    order = sc.triangleOrder()
    return sorted(tuple(sorted((int(order[i]), int(order[j])))) for i, j in np.asarray(pairs).tolist())


def test_self_intersections_of_two_crossing_quads_and_a_closed_tetrahedron(renderer):
    """tests/tri_overlap_scenes.py derives the pairs by hand: of the two quads A (z = 0) and B (x = 1), A0-B0 and A0-B1 cut, A1-B0
    touch in the one point (1, 1, 0), A1-B1 are apart, and A0-A1 and B0-B1 share two vertices each and are dropped.  The builder is
    free to reorder the triangles, so the pairs are compared by load index."""
    sc, _ = flat_scene(CROSSING_QUADS)
    pairs = renderer.selfIntersections(sc)
    assert isinstance(pairs, np.ndarray) and pairs.dtype == np.int32 and pairs.shape == (3, 2) and (pairs[:, 0] < pairs[:, 1]).all()
    assert by_load_index(sc, pairs) == CROSSING_PAIRS
    assert by_load_index(sc, tv.self_pairs(nr.from_product(sc), CROSSING_QUADS[sc.triangleOrder()])) == CROSSING_PAIRS
    # positions= in load order, on the device: a device tensor comes back
    dev_pairs = renderer.selfIntersections(sc, positions=torch.from_numpy(CROSSING_QUADS).to(DEV))
    assert torch.is_tensor(dev_pairs) and dev_pairs.dtype == torch.int32 and (dev_pairs.cpu().numpy() == pairs).all()
    # before the drop every triangle lists itself, its neighbour and what it cuts
    order = sc.triangleOrder()
    lists = renderer.overlapTriangles(sc, CROSSING_QUADS[order])
    listed = {(int(order[i]), int(order[j])) for i in range(4) for j in lists.prim[lists.splits[i]:lists.splits[i + 1]]}
    assert listed == {(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2), (2, 3), (3, 0), (3, 2), (3, 3)}
    # a closed tetrahedron: every pair of faces touches along an edge, shares its two vertices, and none is reported
    tet, _ = flat_scene(TETRAHEDRON)
    none = renderer.selfIntersections(tet)
    assert none.shape == (0, 2) and none.dtype == np.int32
    assert (renderer.overlapTriangles(tet, TETRAHEDRON, k=4).count == 4).all()


def test_queries_leave_the_renderer_alone_and_work_on_a_sharded_one(renderer, batch):
    sc, g, q, totals, lists, table = batch
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
            assert (r.overlapTriangles(sc, q, k=4).prim.reshape(-1) == table).all()
            assert (r.overlapTriangles(sc, q).prim == lists).all() and (r.intersectsAny(sc, q) == (totals > 0)).all()
            assert r.kernelInfo() == info and r.getSampleCount() == n and r.kernelSpanMs() == span
            assert bytes(r.getCounters()) == counters
            assert r.GetRenderTargetImage().tobytes() == frame.tobytes() and r.GetAccumulationBuffer().tobytes() == accum.tobytes()
        r.Render(cam, sc)
        images.append((r.GetRenderTargetImage(), r.getSampleCount()))
    assert images[0][0].tobytes() == images[1][0].tobytes() and images[0][1] == images[1][1]
    r = drt.Renderer(0)
    r.setShard(8, 1, 2)
    r.ResizeBuffer(96, 64)
    got = r.overlapTriangles(sc, q, k=4)
    assert (got.prim.reshape(-1) == table).all() and (got.count.view(np.uint32) == totals).all()
    assert (r.intersectsAny(sc, q) == (totals > 0)).all()


def test_an_empty_scene_lists_nothing(renderer, batch):
    sc = drt.Scene()
    sc.addMaterial(*ONE_MATERIAL[0])
    sc.setGeometry(np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 2), np.float32), np.zeros(0, np.int32))
    drt.BVHBuilder().buildIterative(sc)
    q = batch[2]
    got = renderer.overlapTriangles(sc, q, k=3)
    assert (got.prim == -1).all() and not got.count.any()
    whole = renderer.overlapTriangles(sc, q)
    assert whole.splits.shape == (258,) and not whole.splits.any() and len(whole.prim) == 0 and whole.prim.dtype == np.int32
    assert not renderer.intersectsAny(sc, q).any()
    assert renderer.selfIntersections(sc).shape == (0, 2)


def test_error_paths(renderer, batch):
    sc, g, ref_q, totals, lists, table = batch
    dev = torch.device(DEV)
    n = 64
    tris = torch.zeros((n + 1, 12), dtype=torch.float32, device=dev)
    tris[:, 3], tris[:, 7] = 1, 1                                                # (0, 0, 0), (1, 0, 0), (0, 1, 0)
    offsets = (torch.arange(n + 2, dtype=torch.int32, device=dev) * 2)
    prims = torch.full((2 * n + 8,), SENTINEL, dtype=torch.int32, device=dev)
    counts = torch.full((n + 1,), -1, dtype=torch.int32, device=dev)
    host = np.zeros((2 * n + 8, 12), np.float32)
    L, h = drt._lib, renderer._h
    INV = drt.ERR_INVALID
    cap = 2 * n
    B, O, P, C, H = tris.data_ptr(), offsets.data_ptr(), prims.data_ptr(), counts.data_ptr(), host.ctypes.data
    for what, args in (("null tris", (h, sc._h, None, O, P, cap, C, n, 0)), ("null offsets", (h, sc._h, B, None, P, cap, C, n, 0)),
                       ("null renderer", (None, sc._h, B, O, P, cap, C, n, 0)), ("null scene", (h, None, B, O, P, cap, C, n, 1)),
                       ("mode 2", (h, sc._h, B, O, P, cap, C, n, 2)), ("mode -1", (h, sc._h, B, O, P, cap, C, n, -1)),
                       ("mode 2, n = 0", (h, sc._h, B, O, P, cap, C, 0, 2)), ("mode 2, null tris", (h, sc._h, None, O, P, cap, C, n, 2)),
                       ("both outputs null", (h, sc._h, B, O, None, 0, None, n, 0)), ("null prims with a capacity", (h, sc._h, B, O, None, cap, C, n, 0)),
                       ("prims without a capacity", (h, sc._h, B, O, P, 0, C, n, 0)),
                       ("any with prims", (h, sc._h, B, O, P, cap, C, n, 1)), ("any with a capacity", (h, sc._h, B, O, None, cap, C, n, 1)),
                       ("any without counts", (h, sc._h, B, O, None, 0, None, n, 1)),
                       ("misaligned tris", (h, sc._h, B + 4, O, P, cap, C, n, 0)), ("misaligned prims", (h, sc._h, B, O, P + 2, cap, C, n, 0)),
                       ("misaligned offsets", (h, sc._h, B, O + 2, P, cap, C, n, 0)), ("misaligned counts", (h, sc._h, B, O, P, cap, C + 1, n, 0)),
                       ("host tris", (h, sc._h, H, O, P, cap, C, n, 0)), ("host offsets", (h, sc._h, B, H, P, cap, C, n, 0)),
                       ("host prims", (h, sc._h, B, O, H, cap, C, n, 0)), ("host counts", (h, sc._h, B, O, P, cap, H, n, 0)),
                       ("host counts, any", (h, sc._h, B, None, None, 0, H, n, 1)), ("null handles, n = 0", (None, None, B, O, P, cap, C, 0, 0))):
        assert L.drt_renderer_overlap_triangles(*args, None) == INV, what
        if what.startswith("mode"):
            assert b"mode" in L.drt_last_error(), what                                                    # checked first after the handles
    for mode in (0, 1):
        assert L.drt_renderer_overlap_triangles(h, sc._h, None, None, None, 0, None, 0, mode, None) == drt.OK   # n == 0: nothing to do
        assert L.drt_renderer_overlap_triangles(h, sc._h, B, O, P, cap, C, 0, mode, None) == drt.OK
    torch.cuda.synchronize()
    assert (prims == SENTINEL).all() and (counts == -1).all()                                              # nothing was launched
    # tris need 16-byte alignment, the rest 4: one triangle and one word further on
    assert L.drt_renderer_overlap_triangles(h, sc._h, B + 48, O + 4, P + 4, cap + 2, C + 4, n, 0, None) == drt.OK
    torch.cuda.synchronize()
    assert prims[0] == SENTINEL and (prims[1:1 + 2] == SENTINEL).all() and (prims[1 + 2 + 2 * n:] == SENTINEL).all()
    assert not (prims[1 + 2:1 + 2 + 2 * n] == SENTINEL).any() and counts[0] == -1 and (counts[1:] >= 0).all()
    empty = renderer.overlapTriangles(sc, np.zeros((0, 3, 3), np.float32))
    assert empty.splits.tolist() == [0] and len(empty.prim) == 0
    assert renderer.overlapTriangles(sc, np.zeros((0, 12), np.float32), k=5).prim.shape == (0, 5)
    assert renderer.intersectsAny(sc, np.zeros((0, 3, 3), np.float32)).shape == (0,)
    for bad in (lambda: renderer.overlapTriangles(sc, tris, k=0),
                lambda: renderer.overlapTriangles(sc, tris.cpu()),                                       # wrong device
                lambda: renderer.overlapTriangles(sc, tris.double()),                                    # wrong dtype
                lambda: renderer.overlapTriangles(sc, tris[:, :11]),                                     # wrong shape
                lambda: renderer.overlapTriangles(sc, tris[:, :9]),                                      # [N, 9] is neither form
                lambda: renderer.overlapTriangles(sc, tris[:, :9].reshape(-1, 3, 3).tolist()),           # neither numpy nor torch
                lambda: renderer.intersectsAny(sc, tris.cpu()),
                lambda: renderer.intersectsAny(sc, host.astype(np.float64)),
                lambda: renderer.selfIntersections(sc, positions=np.zeros((5, 3, 3), np.float32)),       # not the scene's triangle count
                lambda: renderer.overlapTriangles(sc, host.astype(np.float64))):
        with pytest.raises(drt.DrtError) as e:
            bad()
        assert e.value.code == INV
    # a pending asynchronous batch
    r = drt.Renderer(0)
    r.ResizeBuffer(64, 32)
    r.RenderBatchAsync(drt.Camera(SCENES["cornell_box"][1]), sc, 1)
    for call in (lambda: r.overlapTriangles(sc, tris, k=2), lambda: r.overlapTriangles(sc, tris), lambda: r.intersectsAny(sc, tris)):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == INV
    assert raw(r, sc, tris, offsets, prims, cap, counts, n, 0) == INV
    r.Wait()
    r.overlapTriangles(sc, tris, k=2), r.intersectsAny(sc, tris)
    # a tree deeper than 64 levels: the chain's centroids double per triangle (scaled down so that no area overflows)
    chain = list(rq.degenerate_chain(110))
    chain[0] = (chain[0] * np.float32(2.0 ** -55)).astype(np.float32)
    deep, _ = rq.programmatic_scene(drt, *chain, 1, 2)
    assert deep.bvh_depth > 64
    for call in (lambda: renderer.overlapTriangles(deep, tris, k=2), lambda: renderer.intersectsAny(deep, tris)):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == drt.ERR_UNSUPPORTED
    assert (renderer.overlapTriangles(sc, ref_q, k=4).prim.reshape(-1) == table).all()                    # after the errors
