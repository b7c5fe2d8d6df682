"""Triangle intersection segments on the GPU (drt_renderer_intersect_triangles, kernel_intersect.hip; Renderer.intersectTriangles /
selfIntersectionSegments): every word of every slot of every segment and every count bit-equal to the restatement in
tests/intersect_ref.py, miss-filled slots included -- over one triangle, the quad, the two crossing quads, a soup, cornell_box and a tree
deeper than the LDS stack, queries from a point to a triangle across the whole scene, invalid and zero-area ones, capacities, batch
shapes, a refitted device copy, the torch and the numpy path -- nothing written outside the segments, the renderer's state untouched,
and the error codes of include/drt.h.  tests/test_intersect_ref.py asserts what the restatement does.

The scenes, the query sweep and the spears are tests/test_gpu_tri_overlap.py's, by import.  Records are compared as int32 words: the
miss record's prim = -1 is a NaN as a float."""
import numpy as np
import pytest

from tests import intersect_ref as ix
from tests import nearest_ref as nr
from tests import tri_overlap_ref as tv
from tests.scenes import SCENES
from tests.test_gpu_tri_overlap import SPEARS, _load, by_load_index, csr, flat_scene, scene_pair, sweep_queries
from tests.tri_overlap_scenes import CROSSING_PAIRS, CROSSING_QUADS, TETRAHEDRON

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -77
SCENE_NAMES = ["single", "quad", "crossing_quads", "soup", "chain", "cornell_box"]
_crossing = []


@pytest.fixture(scope="module")
def renderer():
    return drt.Renderer(0)


def pair_of(name):
    if name != "crossing_quads":
        return scene_pair(name)
    if not _crossing:
        sc, osc = flat_scene(CROSSING_QUADS)
        _crossing.append((sc, nr.from_oracle(osc)))
    return _crossing[0]


def words(rec):
    return np.ascontiguousarray(rec).view(np.int32).reshape(-1, 8)


def reference(g, q):
    """(every record of every query as int32 words [M, 8], totals uint32 [N]): one count and one fill of the restatement.  The list at
    a smaller capacity is its prefix with the miss record behind a shorter one (tests/test_intersect_ref.py asserts that of the
    restatement), so the tests below cut their expectations from these and leave them unchanged."""
    _, totals = ix.intersect(g, q, 0)
    rec, _ = ix.intersect(g, q, totals)
    return words(rec), totals


def cut(whole, totals, caps):
    """The flat words of segments of `caps` slots (a scalar or [N]) from reference()'s lists."""
    n = len(totals)
    caps = np.broadcast_to(np.asarray(caps, np.int64), n)
    start, base = csr(totals), csr(caps)
    out = np.tile(ix.MISS.view(np.int32), (int(base[-1]), 1))
    for i in np.nonzero((caps > 0) & (totals > 0))[0]:
        k = min(int(caps[i]), int(totals[i]))
        out[base[i]:base[i] + k] = whole[start[i]:start[i] + k]
    return out


def raw(r, sc, tris, offsets, out, capacity, counts, n, stream=None):
    """The entry point itself on device tensors (or None): the status code."""
    ptr = lambda x: None if x is None else x.data_ptr()
    return drt._lib.drt_renderer_intersect_triangles(r._h, sc._h, ptr(tris), ptr(offsets), ptr(out), capacity, ptr(counts), n, stream)


def run_raw(r, sc, q, offsets, size, capacity, with_out=True, with_counts=True):
    """One call on sentinel-filled buffers of `size` records: (out as int32 words [size, 8], counts) as host arrays (None where not
    given)."""
    n = len(q)
    t = torch.from_numpy(tv.pack(q)).to(DEV)
    off = torch.from_numpy(np.asarray(offsets).astype(np.int32)).to(DEV)
    out = torch.full((size, 8), SENTINEL, dtype=torch.int32, device=DEV) if with_out else None
    counts = torch.full((n,), -1, dtype=torch.int32, device=DEV) if with_counts else None
    assert raw(r, sc, t, off, out, capacity, counts, n) == drt.OK
    torch.cuda.synchronize()
    host = lambda x: None if x is None else x.cpu().numpy()
    return host(out), host(counts)


def as_words(res):
    """A CutList of numpy arrays as int32 words [M, 8]."""
    out = np.zeros((len(res.prim), 8), np.int32)
    out[:, 0:3], out[:, 4:7] = res.p.view(np.int32), res.q.view(np.int32)
    out[:, 3], out[:, 7] = res.prim, res.code
    return out


def queries_of(name, g):
    q = sweep_queries(g, 150, 11, whole=1) if name == "soup" else sweep_queries(g, 240, 11)
    if name == "chain":
        q = np.concatenate([SPEARS, q])
    if name == "crossing_quads":
        q = np.concatenate([CROSSING_QUADS, q])
    return q


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_every_record_is_bit_equal_to_the_restatement(renderer, name):
    sc, g = pair_of(name)
    q = queries_of(name, g)
    n = len(q)
    whole, totals = reference(g, q)
    if name == "chain":
        assert totals[:2].tolist() == [29, 25]                                   # the spears: records that were held in the HBM levels
    assert (totals == 0).any() and (totals > 0).any() and not totals[-4:].any()  # nothing; something; NaN and inf
    # every segment of every query: a count with capacity 0, the scan, the fill.  numpy in, numpy out.
    got = renderer.intersectTriangles(sc, q)
    assert isinstance(got, drt.CutList) and got.splits.dtype == np.int32 and got.prim.dtype == np.int32 and got.code.dtype == np.int32
    assert got.p.dtype == np.float32 and got.p.shape == (len(whole), 3) and got.q.shape == (len(whole), 3)
    assert (got.splits == csr(totals)).all() and (as_words(got) == whole).all(), name
    # [N, 3, 3] and the packed [N, 12] are the same query; the pad words are ignored
    packed = tv.pack(q)
    packed[:, 9:] = np.nan
    again = renderer.intersectTriangles(sc, packed)
    assert (again.splits == got.splits).all() and (as_words(again) == whole).all()
    # the raw entry point with ragged capacities, zeros included
    rng = np.random.default_rng(5)
    caps = rng.integers(0, 7, n)
    caps[rng.integers(0, n, n // 8)] = 0
    assert (caps == 0).sum() >= n // 16 and (caps > totals).any()
    offsets = csr(caps)
    out, counts = run_raw(renderer, sc, q, offsets, int(caps.sum()), int(caps.sum()))
    assert (out == cut(whole, totals, caps)).all() and (counts.view(np.uint32) == totals).all()
    if name != "soup":                                                           # (the restatement itself at these capacities)
        ref, ref_counts = ix.intersect(g, q, caps)
        assert (out == words(ref)).all() and (counts.view(np.uint32) == ref_counts).all()
    # counts NULL: the same records
    out2, _ = run_raw(renderer, sc, q, offsets, int(caps.sum()), int(caps.sum()), with_counts=False)
    assert out2.tobytes() == out.tobytes()
    # a pure count: capacity 0 and no out
    _, counts = run_raw(renderer, sc, q, np.zeros(n + 1), 0, 0, with_out=False)
    assert (counts.view(np.uint32) == totals).all()


def test_the_crossing_quads_by_hand(renderer):
    """tests/test_intersect_ref.py derives the three records of A0, A1 against a scene of B0, B1.  The builder is free to reorder the
    two triangles, so prim is compared by load index."""
    sc, _ = flat_scene(CROSSING_QUADS[2:])
    order = sc.triangleOrder()
    got = renderer.intersectTriangles(sc, CROSSING_QUADS[:2])
    assert got.splits.tolist() == [0, 2, 3]
    rows = sorted((i, int(order[got.prim[k]]), got.p[k].tolist(), got.q[k].tolist(), int(got.code[k])) for i in (0, 1)
                  for k in range(got.splits[i], got.splits[i + 1]))
    assert rows == [(0, 0, [1, 0, 0], [1, 1, 0], 2 + 16 * 1), (0, 1, [1, -1, 0], [1, 0, 0], 2 + 16 * 0), (1, 0, [1, 1, 0], [1, 1, 0], 4 + 16 * 1)]
    # coplanar, zero-area and invalid queries list nothing, on the triangle (0, 0, 0), (4, 0, 0), (0, 4, 0)
    one, _ = flat_scene(np.float32([[[0, 0, 0], [4, 0, 0], [0, 4, 0]]]))
    q = np.float32([[(1, 1, -1), (1, 1, 1), (5, 5, 0)], [(1, 1, 0), (2, 1, 0), (1, 2, 0)], [(0, 0, 0), (4, 0, 0), (0, 4, 0)],
                    [(1, 1, -2), (1, 1, 2), (1, 1, 2)], [(1, 1, 0)] * 3, [(1, 1, -1), (1, np.nan, 1), (5, 5, 0)],
                    [(1, 1, -1), (1, 1, 1), (np.inf, 5, 0)], [(1e30, 1e30, -1e30), (1e30, 1e30, 1e30), (5e30, 5e30, 0)]])
    want = [1, 0, 0, 0, 0, 0, 0, 0]
    assert ix.intersect(nr.from_product(one), q, 0)[1].tolist() == want
    assert np.diff(renderer.intersectTriangles(one, q).splits).tolist() == want


@pytest.fixture(scope="module")
def batch():
    """257 queries on cornell_box and their whole lists."""
    sc, g = scene_pair("cornell_box")
    q = sweep_queries(g, 260, 21)[-257:]
    assert len(q) == 257
    whole, totals = reference(g, q)
    assert totals.max() > 4 and (totals == 0).any() and ((totals > 0) & (totals < 4)).any()
    return sc, g, q, totals, whole


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(renderer, batch, n):
    sc, g, q, totals, whole = batch
    base = csr(totals)
    for sl in (slice(0, n), slice(257 - n, 257)):
        got = renderer.intersectTriangles(sc, q[sl])
        assert (got.splits == base[sl.start:sl.stop + 1] - base[sl.start]).all()
        assert (as_words(got) == whole[base[sl.start]:base[sl.stop]]).all()
        off = csr(np.full(n, 4))
        out, counts = run_raw(renderer, sc, q[sl], off, 4 * n, 4 * n)
        assert (out == cut(whole[base[sl.start]:base[sl.stop]], totals[sl], 4)).all() and (counts.view(np.uint32) == totals[sl]).all()


def test_about_5000_queries_a_permutation_and_a_second_run(renderer, batch):
    """20 x 257 = 5140 queries: the claim crosses shards, and waves refill lanes from more than one of them."""
    sc, g, q, totals, whole = batch
    tiles = 20
    dev_q = torch.from_numpy(q).to(DEV).repeat(tiles, 1, 1)
    res = renderer.intersectTriangles(sc, dev_q)
    per_tile = int(totals.sum())
    assert int(res.splits[-1]) == tiles * per_tile and torch.equal(res.splits[:258].cpu(), torch.from_numpy(csr(totals).astype(np.int32)))
    want = torch.from_numpy(whole).to(DEV)
    got = torch.stack([res.p.view(torch.int32), res.q.view(torch.int32)], dim=1).reshape(tiles, per_tile, 6)
    assert (got == torch.stack([want[:, 0:3], want[:, 4:7]], dim=1).reshape(1, per_tile, 6)).all()
    assert (res.prim.reshape(tiles, per_tile) == want[None, :, 3]).all() and (res.code.reshape(tiles, per_tile) == want[None, :, 7]).all()
    again = renderer.intersectTriangles(sc, dev_q)                                 # two runs: identical bytes
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(res, again))
    # shuffled: four slots each, compared query by query
    perm = torch.from_numpy(np.random.default_rng(2).permutation(len(dev_q))).to(DEV)
    n = len(dev_q)
    packed = torch.zeros((n, 12), dtype=torch.float32, device=DEV)
    packed[:, :9] = dev_q[perm].reshape(n, 9)
    off = torch.arange(n + 1, dtype=torch.int32, device=DEV) * 4
    out = torch.full((4 * n, 8), SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    assert raw(renderer, sc, packed, off, out, 4 * n, counts, n) == drt.OK
    table = torch.from_numpy(cut(whole, totals, 4)).to(DEV).reshape(257, 4, 8).repeat(tiles, 1, 1)
    assert torch.equal(out.reshape(n, 4, 8), table[perm])
    assert torch.equal(counts, torch.from_numpy(totals.view(np.int32)).to(DEV).repeat(tiles)[perm])


@pytest.mark.parametrize("name", ["cornell_box", "chain"])
def test_capacities_0_to_9_truncate_a_query_across_the_whole_scene(renderer, name):
    sc, g = scene_pair(name)
    q = SPEARS if name == "chain" else sweep_queries(g, 3, 3)[-6:-4]              # the two triangles across the whole scene
    whole, totals = reference(g, q)
    assert totals.max() > 9
    for cap in range(0, 10):
        lead = 3
        off = lead + csr(np.full(len(q), cap))
        size = int(off[-1]) + 5
        out, counts = run_raw(renderer, sc, q, off, size, size)
        assert (out[:lead] == SENTINEL).all() and (out[off[-1]:] == SENTINEL).all()
        assert (out[lead:off[-1]] == cut(whole, totals, cap)).all() and (counts.view(np.uint32) == totals).all(), cap


def test_nothing_outside_the_segments_is_written(renderer, batch):
    sc, g, q, totals, whole = batch
    n = len(q)
    rng = np.random.default_rng(9)
    caps = rng.integers(0, 7, n)
    lead, trail = 7, 9
    off = lead + csr(caps)
    # records before offsets[0] and from offsets[n] on are untouched
    size = int(off[-1]) + trail
    out, counts = run_raw(renderer, sc, q, off, size, size)
    assert (out[:lead] == SENTINEL).all() and (out[off[-1]:] == SENTINEL).all()
    assert (out[lead:off[-1]] == cut(whole, totals, caps)).all() and (counts.view(np.uint32) == totals).all()
    # a capacity stated smaller than the last offsets, ending inside a segment: the records at and beyond it are untouched (the
    # tensor is as large as the unclamped offsets need, so nothing can leave the allocation)
    i = int(np.nonzero((caps >= 2) & (np.arange(n) > n // 2))[0][0])
    stated = int(off[i]) + 1
    out, counts = run_raw(renderer, sc, q, off, size, stated)
    assert (out[stated:] == SENTINEL).all() and (out[:lead] == SENTINEL).all()
    clamped = ix.caps_of(off, stated)
    assert clamped[i] == 1 and not clamped[i + 1:].any() and (clamped[:i] == caps[:i]).all()
    assert (out[lead:stated] == cut(whole, totals, clamped)).all() and (counts.view(np.uint32) == totals).all()
    # decreasing pairs of offsets give capacity 0: even queries own four slots each in blocks that descend through the array
    m = n - 1                                   # an even number of queries
    b = 8 * (m // 2 - np.arange(m // 2 + 1))
    down = np.empty(m + 1, np.int64)
    down[0::2], down[1::2] = b, b[:-1] + 4
    assert down[-1] == 0 and (down[2::2] < down[1::2]).all()
    size = int(down.max()) + 8
    out, counts = run_raw(renderer, sc, q[:m], down, size, size)
    even = np.where(np.arange(m) % 2 == 0, 4, 0)
    assert (ix.caps_of(down, size) == even).all()
    owned = (down[0:m:2, None] + np.arange(4)[None, :]).reshape(-1)
    assert (out[owned] == cut(whole[:csr(totals)[m]], totals[:m], even)).all() and (counts.view(np.uint32) == totals[:m]).all()
    rest = np.ones(size, bool)
    rest[owned] = False
    assert (out[rest] == SENTINEL).all()


def test_after_a_refit_the_moved_mesh_answers(renderer):
    sc, st = _load("cornell_box")
    moved = (st[0] + np.random.default_rng(1).normal(0, 0.05, st[0].shape)).astype(np.float32)
    host, _ = _load("cornell_box")
    host.refit(moved)                                          # the host scene refitted with the same positions
    g_old, g_new = nr.from_product(sc), nr.from_product(host)
    q = np.concatenate([sweep_queries(g_old, 120, 4, whole=1), sweep_queries(g_new, 120, 5, whole=1)])
    old, old_counts = reference(g_old, q)
    new, new_counts = reference(g_new, q)
    assert (old_counts != new_counts).any() and old.tobytes() != new.tobytes()
    r = drt.Renderer(0)
    got = r.intersectTriangles(sc, q)
    assert (got.splits == csr(old_counts)).all() and (as_words(got) == old).all()
    r.refit(sc, torch.from_numpy(moved).to(DEV))
    got = r.intersectTriangles(sc, q)
    assert (got.splits == csr(new_counts)).all() and (as_words(got) == new).all()
    # the moved mesh against itself: positions= in load order, as refit took them; the host scene's own are the old ones
    tree = lambda scene: np.ascontiguousarray(scene.m_PrimitivesBuffer["vertex"]["position"], np.float32).reshape(-1, 3, 3)
    pairs, p, e, code = ix.self_cuts(g_new, tree(host))
    assert len(pairs) > 5                                      # (every vertex moved on its own: former neighbours now cut or miss)
    cuts = r.selfIntersectionSegments(sc, positions=moved)
    assert (cuts.pairs == pairs).all() and cuts.p.tobytes() == p.tobytes() and cuts.q.tobytes() == e.tobytes() and (cuts.code == code).all()
    got = renderer.intersectTriangles(sc, q)                   # a renderer that was not refitted
    assert (got.splits == csr(old_counts)).all() and (as_words(got) == old).all()


def test_torch_path_stays_on_the_device_and_orders_with_the_stream(renderer, batch):
    sc, g, q, totals, whole = batch
    dev = torch.device(DEV)
    n = len(q)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        dq = torch.from_numpy(q).to(dev)
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(2000000)                  # the inputs' producer is still busy when the queries are enqueued
        res = renderer.intersectTriangles(sc, dq * 1.0)
        packed = renderer.intersectTriangles(sc, torch.from_numpy(tv.pack(q)).to(dev) * 1.0)
        p_copy = res.p.clone()
    assert isinstance(res, drt.CutList) and all(x.device == dev for x in res) and all(x.device == dev for x in packed)
    assert res.splits.dtype == torch.int32 and tuple(res.splits.shape) == (n + 1,) and res.p.dtype == torch.float32
    assert res.prim.dtype == torch.int32 and res.code.dtype == torch.int32 and tuple(res.q.shape) == (len(whole), 3)
    s.synchronize()
    host = lambda r: drt.CutList(*(x.cpu().numpy() for x in r))
    assert (host(res).splits == csr(totals)).all() and (as_words(host(res)) == whole).all() and (as_words(host(packed)) == whole).all()
    assert p_copy.cpu().numpy().tobytes() == host(res).p.tobytes()


def test_self_intersection_segments_of_two_crossing_quads_and_a_closed_tetrahedron(renderer):
    """tests/tri_overlap_scenes.py derives the pairs by hand: (0, 2), (0, 3) cut and (1, 2) touch in the one point (1, 1, 0), in load
    order.  selfIntersections reports all three, and so does this: the touch is not in a common plane, and its segment has zero
    length.  The builder is free to reorder the triangles, so pairs are compared by load index and the records with the
    restatement."""
    sc, _ = flat_scene(CROSSING_QUADS)
    g = nr.from_product(sc)
    order = sc.triangleOrder()
    cuts = renderer.selfIntersectionSegments(sc)
    assert isinstance(cuts, drt.SelfCuts) and all(isinstance(x, np.ndarray) for x in cuts)
    assert cuts.pairs.dtype == np.int32 and cuts.pairs.shape == (3, 2) and (cuts.pairs[:, 0] < cuts.pairs[:, 1]).all()
    assert cuts.p.shape == (3, 3) and cuts.q.shape == (3, 3) and cuts.code.dtype == np.int32 and cuts.code.shape == (3,)
    assert by_load_index(sc, cuts.pairs) == CROSSING_PAIRS and (cuts.pairs == renderer.selfIntersections(sc)).all()
    pairs, p, e, code = ix.self_cuts(g, CROSSING_QUADS[order])
    assert (cuts.pairs == pairs).all() and cuts.p.tobytes() == p.tobytes() and cuts.q.tobytes() == e.tobytes() and (cuts.code == code).all()
    # the segments by hand, whichever role the builder's order gave each triangle: the two halves of x = 1, z = 0, -1 <= y <= 1, and a point
    ends = {tuple(sorted((int(order[i]), int(order[j])))): sorted([cuts.p[k].tolist(), cuts.q[k].tolist()]) for k, (i, j) in enumerate(cuts.pairs.tolist())}
    assert ends == {(0, 2): [[1, 0, 0], [1, 1, 0]], (0, 3): [[1, -1, 0], [1, 0, 0]], (1, 2): [[1, 1, 0], [1, 1, 0]]}
    # positions= in load order, on the device: device tensors come back
    dev_cuts = renderer.selfIntersectionSegments(sc, positions=torch.from_numpy(CROSSING_QUADS).to(DEV))
    assert all(torch.is_tensor(x) for x in dev_cuts) and dev_cuts.pairs.dtype == torch.int32
    assert all(a.cpu().numpy().tobytes() == b.tobytes() for a, b in zip(dev_cuts, cuts))
    # a closed tetrahedron: every pair of faces shares an edge and its two vertices, and none is reported
    tet, _ = flat_scene(TETRAHEDRON)
    none = renderer.selfIntersectionSegments(tet)
    assert none.pairs.shape == (0, 2) and none.pairs.dtype == np.int32 and none.p.shape == (0, 3) and none.code.shape == (0,)


def test_queries_leave_the_renderer_alone_and_work_on_a_sharded_one(renderer, batch):
    sc, g, q, totals, whole = batch
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
            assert (as_words(r.intersectTriangles(sc, q)) == whole).all()
            assert r.kernelInfo() == info and r.getSampleCount() == n and r.kernelSpanMs() == span
            assert bytes(r.getCounters()) == counters
            assert r.GetRenderTargetImage().tobytes() == frame.tobytes() and r.GetAccumulationBuffer().tobytes() == accum.tobytes()
        r.Render(cam, sc)
        images.append((r.GetRenderTargetImage(), r.getSampleCount()))
    assert images[0][0].tobytes() == images[1][0].tobytes() and images[0][1] == images[1][1]
    r = drt.Renderer(0)
    r.setShard(8, 1, 2)
    r.ResizeBuffer(96, 64)
    got = r.intersectTriangles(sc, q)
    assert (got.splits == csr(totals)).all() and (as_words(got) == whole).all()


def test_an_empty_scene_lists_nothing(renderer, batch):
    sc = drt.Scene()
    sc.addMaterial((0.8, 0.8, 0.8), -1)
    sc.setGeometry(np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 2), np.float32), np.zeros(0, np.int32))
    drt.BVHBuilder().buildIterative(sc)
    q = batch[2]
    got = renderer.intersectTriangles(sc, q)
    assert got.splits.shape == (258,) and not got.splits.any() and got.p.shape == (0, 3) and got.prim.dtype == np.int32
    out, counts = run_raw(renderer, sc, q, csr(np.full(len(q), 2)), 2 * len(q), 2 * len(q))
    assert (out == ix.MISS.view(np.int32)).all() and not counts.any()
    assert renderer.selfIntersectionSegments(sc).pairs.shape == (0, 2)


def test_error_paths(renderer, batch):
    sc, g, ref_q, totals, whole = batch
    dev = torch.device(DEV)
    n = 64
    tris = torch.zeros((n + 1, 12), dtype=torch.float32, device=dev)
    tris[:, 3], tris[:, 7] = 1, 1                                                # (0, 0, 0), (1, 0, 0), (0, 1, 0)
    offsets = (torch.arange(n + 2, dtype=torch.int32, device=dev) * 2)
    out = torch.full((2 * n + 8, 8), SENTINEL, dtype=torch.int32, device=dev)
    counts = torch.full((n + 1,), -1, dtype=torch.int32, device=dev)
    host = np.zeros((2 * n + 8, 12), np.float32)
    L, h = drt._lib, renderer._h
    INV = drt.ERR_INVALID
    cap = 2 * n
    B, O, P, C, H = tris.data_ptr(), offsets.data_ptr(), out.data_ptr(), counts.data_ptr(), host.ctypes.data
    for what, args in (("null tris", (h, sc._h, None, O, P, cap, C, n)), ("null offsets", (h, sc._h, B, None, P, cap, C, n)),
                       ("null renderer", (None, sc._h, B, O, P, cap, C, n)), ("null scene", (h, None, B, O, P, cap, C, n)),
                       ("both outputs null", (h, sc._h, B, O, None, 0, None, n)), ("null out with a capacity", (h, sc._h, B, O, None, cap, C, n)),
                       ("out without a capacity", (h, sc._h, B, O, P, 0, C, n)),
                       ("misaligned tris", (h, sc._h, B + 4, O, P, cap, C, n)), ("misaligned out", (h, sc._h, B, O, P + 4, cap, C, n)),
                       ("misaligned offsets", (h, sc._h, B, O + 2, P, cap, C, n)), ("misaligned counts", (h, sc._h, B, O, P, cap, C + 1, n)),
                       ("host tris", (h, sc._h, H, O, P, cap, C, n)), ("host offsets", (h, sc._h, B, H, P, cap, C, n)),
                       ("host out", (h, sc._h, B, O, H, cap, C, n)), ("host counts", (h, sc._h, B, O, P, cap, H, n)),
                       ("host counts, a pure count", (h, sc._h, B, O, None, 0, H, n)), ("null handles, n = 0", (None, None, B, O, P, cap, C, 0))):
        assert L.drt_renderer_intersect_triangles(*args, None) == INV, what
        if what.startswith("host"):
            assert b"device memory" in L.drt_last_error(), what
    assert L.drt_renderer_intersect_triangles(h, sc._h, None, None, None, 0, None, 0, None) == drt.OK       # n == 0: nothing to do
    assert L.drt_renderer_intersect_triangles(h, sc._h, B, O, P, cap, C, 0, None) == drt.OK
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (counts == -1).all()                                                  # nothing was launched
    # tris and out need 16-byte alignment, the rest 4: one triangle, one record and one word further on
    assert L.drt_renderer_intersect_triangles(h, sc._h, B + 48, O + 4, P + 32, cap + 2, C + 4, n, None) == drt.OK
    torch.cuda.synchronize()
    assert (out[0] == SENTINEL).all() and (out[1:1 + 2] == SENTINEL).all() and (out[1 + 2 + 2 * n:] == SENTINEL).all()
    assert not (out[1 + 2:1 + 2 + 2 * n] == SENTINEL).any() and counts[0] == -1 and (counts[1:] >= 0).all()
    empty = renderer.intersectTriangles(sc, np.zeros((0, 3, 3), np.float32))
    assert empty.splits.tolist() == [0] and empty.p.shape == (0, 3) and len(empty.prim) == 0
    for bad in (lambda: renderer.intersectTriangles(sc, tris.cpu()),                                        # wrong device
                lambda: renderer.intersectTriangles(sc, tris.double()),                                     # wrong dtype
                lambda: renderer.intersectTriangles(sc, tris[:, :11]),                                      # wrong shape
                lambda: renderer.intersectTriangles(sc, tris[:, :9].reshape(-1, 3, 3).tolist()),            # neither numpy nor torch
                lambda: renderer.selfIntersectionSegments(sc, positions=np.zeros((5, 3, 3), np.float32)),   # not the scene's triangle count
                lambda: renderer.intersectTriangles(sc, host.astype(np.float64))):
        with pytest.raises(drt.DrtError) as e:
            bad()
        assert e.value.code == INV
    # a pending asynchronous batch
    r = drt.Renderer(0)
    r.ResizeBuffer(64, 32)
    r.RenderBatchAsync(drt.Camera(SCENES["cornell_box"][1]), sc, 1)
    with pytest.raises(drt.DrtError) as e:
        r.intersectTriangles(sc, tris)
    assert e.value.code == INV
    assert raw(r, sc, tris, offsets, out, cap, counts, n) == INV
    r.Wait()
    r.intersectTriangles(sc, tris)
    # a tree deeper than 64 levels: the chain's centroids double per triangle (scaled down so that no area overflows)
    from tests import ray_query_ref as rq
    chain = list(rq.degenerate_chain(110))
    chain[0] = (chain[0] * np.float32(2.0 ** -55)).astype(np.float32)
    deep, _ = rq.programmatic_scene(drt, *chain, 1, 2)
    assert deep.bvh_depth > 64
    with pytest.raises(drt.DrtError) as e:
        renderer.intersectTriangles(deep, tris)
    assert e.value.code == drt.ERR_UNSUPPORTED
    assert (as_words(renderer.intersectTriangles(sc, ref_q)) == whole).all()                                 # after the errors
