"""Box overlap queries on the GPU (drt_renderer_overlap_boxes, kernel_overlap.hip; Renderer.overlapBoxes / overlapsAny / voxelize): every
slot of every segment and every count bit-equal to the restatement in tests/overlap_ref.py, -1-filled slots included -- over one
triangle, the quad, a soup, cornell_box and a tree deeper than the LDS stack, both modes, boxes from a point to the whole scene, rotated
and axis-aligned, capacities, batch shapes, a refitted device copy and the torch path -- nothing written outside the segments, the
renderer's state untouched, and the error codes of include/drt.h.  tests/test_overlap_ref.py asserts what the restatement does.

On the builder's trees a box's triangles arrive in ascending index (child 1's triangles come first and child 1 is popped first), so
here every insert is an append and a full list takes nothing more: the whole-scene boxes at capacities 1 to 9 exercise truncation and
the -1 fill, not the insert before a stored record or the eviction.  Those run in tests/test_overlap_ref.py, over a tree with
exchanged children, which the public interface cannot hand to the GPU."""
import numpy as np
import pytest

import oracle
from tests import nearest_ref as nr
from tests import overlap_ref as ov
from tests import ray_query_ref as rq
from tests import refit_ref as rf
from tests.scenes import SCENES, scene_path

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -77
ONE_MATERIAL = [((0.8, 0.8, 0.8), -1)]
SINGLE = np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
QUAD = np.float32([[[0, 0, 0], [1, 0, 0], [1, 1, 0]], [[0, 0, 0], [1, 1, 0], [0, 1, 0]]])
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
    """(product scene, Geometry of the oracle's scene) with the same tree, as tests/test_gpu_near_list.py builds them: one triangle,
    the quad, the soup of 3000 triangles with two per leaf, the chain whose 43 levels outgrow the 16 stack levels in LDS, cornell_box
    with the editor's tree."""
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


def sweep_boxes(g, n, seed, whole=2):
    """About n boxes [N, 16]: centres near surfaces, on vertices and edge midpoints and in the scene's box; halves from 0 (a point)
    over a few per cent of the extent to `whole` boxes that hold the whole scene; every other box rotated, some with axes that are
    neither unit nor orthogonal; and four with a NaN or an infinity in them."""
    rng = np.random.default_rng(seed)
    q = max(n // 3, 1)
    lo, hi = nr.bounds(g)
    extent = np.float32((hi - lo).max())
    center = np.concatenate([nr.surface_points(g, q, rng), nr.tie_points(g, q, rng), nr.box_points(g, q, rng)]).astype(np.float32)
    m = len(center)
    half = (rng.uniform(0, 1, (m, 3)) ** 3 * np.float32(0.15) * extent).astype(np.float32)
    half[::7] = 0                                                               # points
    half[3::11, 2] = 0                                                          # flat boxes
    rot, _ = np.linalg.qr(rng.normal(size=(m, 3, 3)))
    axes = rot.astype(np.float32)
    axes[::2] = np.eye(3, dtype=np.float32)
    axes[5::16] = (axes[5::16] * rng.uniform(0.5, 2, (len(axes[5::16]), 3, 1)) + 0.1).astype(np.float32)       # used as given
    boxes = ov.pack(center, half, axes)
    big = ov.pack(np.tile((lo + hi) / 2, (whole, 1)), np.tile(hi - lo, (whole, 1)))
    if whole > 1:
        big[1, 6:15] = rot[0].astype(np.float32).reshape(9)                     # the whole scene, rotated
    bad = np.repeat(boxes[:1], 4, axis=0)
    bad[0, 1], bad[1, 4], bad[2, 8], bad[3, 3] = np.nan, np.nan, np.nan, np.inf
    return np.concatenate([boxes, big, bad]).astype(np.float32)


def raw(r, sc, boxes, offsets, prims, capacity, counts, n, mode, stream=None):
    """The entry point itself on device tensors (or None): the status code."""
    ptr = lambda x: None if x is None else x.data_ptr()
    return drt._lib.drt_renderer_overlap_boxes(r._h, sc._h, ptr(boxes), ptr(offsets), ptr(prims), capacity, ptr(counts), n, mode, stream)


def run_raw(r, sc, boxes, offsets, size, capacity, mode=ov.LIST, with_prims=True, with_counts=True):
    """One call on sentinel-filled buffers of `size` records: (prims, counts) as host arrays (None where not given)."""
    n = len(boxes)
    b = torch.from_numpy(boxes).to(DEV)
    off = None if offsets is None else torch.from_numpy(np.asarray(offsets).astype(np.int32)).to(DEV)
    prims = torch.full((size,), SENTINEL, dtype=torch.int32, device=DEV) if with_prims else None
    counts = torch.full((n,), -1, dtype=torch.int32, device=DEV) if with_counts else None
    assert raw(r, sc, b, off, prims, capacity, counts, n, mode) == drt.OK
    torch.cuda.synchronize()
    host = lambda x: None if x is None else x.cpu().numpy()
    return host(prims), host(counts)


def csr(totals):
    return np.concatenate([[0], np.cumsum(totals.astype(np.int64))])


def reference(g, boxes):
    """(rows int32 [N, T], totals uint32 [N]) of one run of the restatement at capacity T = all triangles: row i is box i's whole
    list with -1 behind it.  The list at a smaller capacity is its prefix (tests/test_overlap_ref.py asserts that of the
    restatement), so the tests below cut their expectations from these rows and leave them unchanged."""
    T = max(len(g.v0), 1)
    prims, totals = ov.overlap(g, boxes, T)
    return prims.reshape(len(boxes), T), totals


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
    boxes = sweep_boxes(g, 150 if name == "soup" else 240, 11)
    n = len(boxes)
    rows, totals = reference(g, boxes)
    whole = cut(rows, totals)
    assert totals.max() == len(g.v0) and (totals == 0).any() and not totals[-4:].any()       # the whole scene; nothing; NaN and inf
    # every triangle of every box: a count with capacity 0, the scan, the fill
    got = renderer.overlapBoxes(sc, boxes)
    assert isinstance(got, drt.BoxList) and got.splits.dtype == np.int32 and got.prim.dtype == np.int32
    assert (got.splits == csr(totals)).all() and (got.prim == whole).all(), name
    # centre + half + axes and the packed form are the same query
    c, h, ax = ov.unpack(boxes)
    again = renderer.overlapBoxes(sc, c.copy(), h.copy(), ax.copy())
    assert (again.splits == got.splits).all() and (again.prim == got.prim).all()
    # tables of k slots: the first k of each list, -1 behind it, the count the total
    for k in (1, 4, 9):
        table = renderer.overlapBoxes(sc, boxes, k=k)
        assert isinstance(table, drt.BoxTable) and table.prim.shape == (n, k) and table.prim.dtype == np.int32 and table.count.dtype == np.int32
        assert (table.prim.reshape(-1) == cut(rows, k)).all() and (table.count.view(np.uint32) == totals).all(), (name, k)
    # mode ANY is LIST's count > 0
    hit = renderer.overlapsAny(sc, boxes)
    assert hit.dtype == np.bool_ and hit.shape == (n,) and (hit == (totals > 0)).all()
    assert (ov.overlap(g, boxes, 0, ov.ANY)[1] == hit).all()
    assert (renderer.overlapsAny(sc, c.copy(), h.copy(), ax.copy()) == hit).all()
    # the raw entry point with ragged capacities, zeros included
    rng = np.random.default_rng(5)
    caps = rng.integers(0, 7, n)
    caps[rng.integers(0, n, n // 8)] = 0
    assert (caps == 0).sum() >= n // 16 and (caps > totals).any() and (caps < totals).any()
    offsets = csr(caps)
    prims, counts = run_raw(renderer, sc, boxes, offsets, int(caps.sum()), int(caps.sum()))
    assert (prims == cut(rows, caps)).all() and (counts.view(np.uint32) == totals).all()
    if name != "soup":                                                          # (the restatement itself at these capacities)
        ref, ref_counts = ov.overlap(g, boxes, caps)
        assert (prims == ref).all() and (counts.view(np.uint32) == ref_counts).all()
    # counts NULL: the same records
    prims2, _ = run_raw(renderer, sc, boxes, offsets, int(caps.sum()), int(caps.sum()), with_counts=False)
    assert prims2.tobytes() == prims.tobytes()
    # a pure count: capacity 0 and no prims; and mode ANY without offsets
    _, counts = run_raw(renderer, sc, boxes, np.zeros(n + 1), 0, 0, with_prims=False)
    assert (counts.view(np.uint32) == totals).all()
    _, counts = run_raw(renderer, sc, boxes, None, 0, 0, mode=ov.ANY, with_prims=False)
    assert (counts == (totals > 0)).all()


def test_hand_derived_boxes_on_one_triangle(renderer):
    """tests/test_overlap_ref.py's cases: the hypotenuse's edge axis, touching, a point on a vertex, the rotated box."""
    sc, g = scene_pair("single")
    s = np.float32(np.sqrt(0.5))
    turned = np.float32([[s, s, 0], [-s, s, 0], [0, 0, 1]])
    raw_axes = np.float32([[1, 1, 0], [-1, 1, 0], [0, 0, 1]])
    cases = [([0.25, 0.25, 0], [0.125] * 3, None, True), ([0.75, 0.75, 0], [0.125] * 3, None, False), ([0.75, 0.75, 0], [0.25] * 3, None, True),
             ([1, 0, 0], [0] * 3, None, True), ([0.75, 0.75, 0], [0] * 3, None, False), ([0.25, 0.25, 0.125], [0.125, 0.125, 0], None, False),
             ([0.75, 0.75, 0], [0.3125, 0.0625, 0.125], turned, False), ([0.75, 0.75, 0], [0.40625, 0.0625, 0.125], turned, True),
             ([0.75, 0.75, 0], [0.40625, 0.0625, 0.125], None, False),
             ([0.75, 0.75, 0], [0.375, 0.125, 0.125], raw_axes, False), ([0.75, 0.75, 0], [0.5, 0.125, 0.125], raw_axes, True)]
    boxes = np.concatenate([ov.pack([c], [h], a) for c, h, a, _ in cases])
    want = np.array([w for *_, w in cases])
    assert (renderer.overlapsAny(sc, boxes) == want).all()
    table = renderer.overlapBoxes(sc, boxes, k=2)
    assert (table.count == want).all() and (table.prim[:, 0] == np.where(want, 0, -1)).all() and (table.prim[:, 1] == -1).all()
    # lo= / hi= corners: center = (lo + hi) / 2, half = (hi - lo) / 2
    lo, hi = np.float32([[0.625, 0.625, -0.125], [0.5, 0.5, -0.25]]), np.float32([[0.875, 0.875, 0.125], [1, 1, 0.25]])
    assert renderer.overlapsAny(sc, lo=lo, hi=hi).tolist() == [False, True]
    assert renderer.overlapBoxes(sc, lo=lo, hi=hi).splits.tolist() == [0, 0, 1]
    assert (ov.overlap(g, ov.from_corners(lo, hi), 0)[1] == [0, 1]).all()


@pytest.fixture(scope="module")
def batch():
    """257 boxes on cornell_box, their whole lists and their tables at capacity 4."""
    sc, g = scene_pair("cornell_box")
    boxes = sweep_boxes(g, 260, 21)[-257:]
    assert len(boxes) == 257
    _, totals = ov.overlap(g, boxes, 0)
    lists, _ = ov.overlap(g, boxes, totals)
    table, _ = ov.overlap(g, boxes, 4)
    assert totals.max() > 4 and (totals == 0).any() and ((totals > 0) & (totals < 4)).any()
    return sc, g, boxes, totals, lists, table


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(renderer, batch, n):
    sc, g, boxes, totals, lists, table = batch
    base = csr(totals)
    for sl in (slice(0, n), slice(257 - n, 257)):
        got = renderer.overlapBoxes(sc, boxes[sl], k=4)
        assert (got.prim.reshape(-1) == table[4 * sl.start:4 * sl.stop]).all() and (got.count.view(np.uint32) == totals[sl]).all()
        whole = renderer.overlapBoxes(sc, boxes[sl])
        assert (whole.splits == base[sl.start:sl.stop + 1] - base[sl.start]).all()
        assert (whole.prim == lists[base[sl.start]:base[sl.stop]]).all()
        assert (renderer.overlapsAny(sc, boxes[sl]) == (totals[sl] > 0)).all()


def test_about_5000_boxes_a_permutation_and_a_second_run(renderer, batch):
    """20 x 257 = 5140 boxes: the claim crosses shards, and waves refill lanes from more than one of them."""
    sc, g, boxes, totals, lists, table = batch
    tiles, k = 20, 4
    dev_boxes = torch.from_numpy(boxes).to(DEV).repeat(tiles, 1)
    want = torch.from_numpy(table.reshape(-1, k)).to(DEV).repeat(tiles, 1)
    want_counts = torch.from_numpy(totals.view(np.int32)).to(DEV).repeat(tiles)
    res = renderer.overlapBoxes(sc, dev_boxes, k=k)
    assert res.prim.dtype == torch.int32 and torch.equal(res.prim, want) and torch.equal(res.count, want_counts)
    assert torch.equal(renderer.overlapBoxes(sc, dev_boxes, k=k).prim, res.prim)                   # two runs: identical bytes
    perm = torch.from_numpy(np.random.default_rng(2).permutation(len(dev_boxes))).to(DEV)
    shuffled = renderer.overlapBoxes(sc, dev_boxes[perm], k=k)
    assert torch.equal(shuffled.prim, want[perm]) and torch.equal(shuffled.count, want_counts[perm])
    assert torch.equal(renderer.overlapsAny(sc, dev_boxes[perm]), (want_counts > 0)[perm])
    whole = renderer.overlapBoxes(sc, dev_boxes)
    per_tile = int(totals.sum())
    assert int(whole.splits[-1]) == tiles * per_tile
    assert (whole.prim.reshape(tiles, per_tile) == torch.from_numpy(lists).to(DEV)[None]).all()


def test_nothing_outside_the_segments_is_written(renderer, batch):
    sc, g, boxes, totals, lists, table = batch
    n = len(boxes)
    rng = np.random.default_rng(9)
    caps = rng.integers(0, 7, n)
    lead, trail = 7, 9
    off = lead + csr(caps)
    # records before offsets[0] and from offsets[n] on are untouched
    size = int(off[-1]) + trail
    prims, counts = run_raw(renderer, sc, boxes, off, size, size)
    assert (prims[:lead] == SENTINEL).all() and (prims[off[-1]:] == SENTINEL).all()
    ref, ref_counts = ov.overlap(g, boxes, caps)
    assert (prims[lead:off[-1]] == ref).all() and (counts.view(np.uint32) == ref_counts).all()
    # a capacity stated smaller than the last offsets, ending inside a segment: the records at and beyond it are untouched (the
    # tensor is as large as the unclamped offsets need, so nothing can leave the allocation)
    i = int(np.nonzero((caps >= 2) & (np.arange(n) > n // 2))[0][0])
    stated = int(off[i]) + 1
    prims, counts = run_raw(renderer, sc, boxes, off, size, stated)
    assert (prims[stated:] == SENTINEL).all() and (prims[:lead] == SENTINEL).all()
    clamped = ov.caps_of(off, stated)
    assert clamped[i] == 1 and not clamped[i + 1:].any() and (clamped[:i] == caps[:i]).all()
    ref, ref_counts = ov.overlap(g, boxes, clamped)
    assert (prims[lead:stated] == ref).all() and (counts.view(np.uint32) == ref_counts).all()
    # decreasing pairs of offsets give capacity 0: even boxes own four slots each in blocks that descend through the array, so
    # offsets[i + 1] < offsets[i] for every odd box, and no two segments overlap
    m = n - 1                                   # an even number of boxes
    b = 8 * (m // 2 - np.arange(m // 2 + 1))
    down = np.empty(m + 1, np.int64)
    down[0::2], down[1::2] = b, b[:-1] + 4
    assert down[-1] == 0 and (down[2::2] < down[1::2]).all()
    size = int(down.max()) + 8
    prims, counts = run_raw(renderer, sc, boxes[:m], down, size, size)
    even = np.where(np.arange(m) % 2 == 0, 4, 0)
    assert (ov.caps_of(down, size) == even).all()
    owned = (down[0:m:2, None] + np.arange(4)[None, :]).reshape(-1)
    assert (prims[owned] == ov.overlap(g, boxes[:m], even)[0]).all() and (counts.view(np.uint32) == totals[:m]).all()
    rest = np.ones(size, bool)
    rest[owned] = False
    assert (prims[rest] == SENTINEL).all()
    # mode ANY writes its counts and nothing else: offsets that would be wild are not read
    wild = np.full(n + 1, 2 ** 31 - 1)
    _, counts = run_raw(renderer, sc, boxes, wild, 0, 0, mode=ov.ANY, with_prims=False)
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
    boxes = np.concatenate([sweep_boxes(g_old, 120, 4, whole=1), sweep_boxes(g_new, 120, 5, whole=1)])
    old, old_counts = ov.overlap(g_old, boxes, 3)
    new, new_counts = ov.overlap(g_new, boxes, 3)
    assert (old != new).mean() > 0.02 and (old_counts != new_counts).any()
    r = drt.Renderer(0)
    got = r.overlapBoxes(sc, boxes, k=3)
    assert (got.prim.reshape(-1) == old).all() and (got.count.view(np.uint32) == old_counts).all()
    r.refit(sc, torch.from_numpy(moved).to(DEV))
    got = r.overlapBoxes(sc, boxes, k=3)
    assert (got.prim.reshape(-1) == new).all() and (got.count.view(np.uint32) == new_counts).all()
    assert (r.overlapsAny(sc, boxes) == (new_counts > 0)).all()
    whole = r.overlapBoxes(sc, boxes)
    assert (whole.splits == csr(new_counts)).all() and (whole.prim == ov.overlap(g_new, boxes, new_counts)[0]).all()
    got = renderer.overlapBoxes(sc, boxes, k=3)                # a renderer that was not refitted
    assert (got.prim.reshape(-1) == old).all() and (got.count.view(np.uint32) == old_counts).all()


def test_torch_path_stays_on_the_device_and_orders_with_the_stream(renderer, batch):
    sc, g, boxes, totals, lists, table = batch
    dev = torch.device(DEV)
    n = len(boxes)
    s = torch.cuda.Stream(device=dev)
    c, h, ax = ov.unpack(boxes)
    with torch.cuda.stream(s):
        dc, dh, dax = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (c, h, ax))
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(2000000)                  # the inputs' producer is still busy when the queries are enqueued
        rows = renderer.overlapBoxes(sc, dc * 1.0, dh * 1.0, dax * 1.0, k=4)
        whole = renderer.overlapBoxes(sc, dc * 1.0, dh * 1.0, dax * 1.0)
        packed = renderer.overlapBoxes(sc, torch.from_numpy(boxes).to(dev) * 1.0, k=4)
        hit = renderer.overlapsAny(sc, dc * 1.0, dh * 1.0, dax * 1.0)
        prim_copy = rows.prim.clone()
    assert all(x.device == dev for x in rows) and all(x.device == dev for x in whole) and hit.device == dev
    assert rows.prim.dtype == torch.int32 and rows.count.dtype == torch.int32 and hit.dtype == torch.bool
    assert tuple(rows.prim.shape) == (n, 4) and whole.splits.dtype == torch.int32 and tuple(whole.splits.shape) == (n + 1,)
    s.synchronize()
    assert (rows.prim.cpu().numpy().reshape(-1) == table).all() and (prim_copy.cpu().numpy().reshape(-1) == table).all()
    assert (packed.prim.cpu().numpy().reshape(-1) == table).all() and (rows.count.cpu().numpy().view(np.uint32) == totals).all()
    assert (whole.splits.cpu().numpy() == csr(totals)).all() and (whole.prim.cpu().numpy() == lists).all()
    assert (hit.cpu().numpy() == (totals > 0)).all()


def test_voxelize_a_dyadic_quad(renderer):
    """The square [0.3125, 0.6875]^2 at height z as two triangles, in the grid of 4^3 cells of side 0.25 over [0, 1]^3: every
    coordinate is dyadic, so every product and sum of the test is exact.  x and y reach into cells 1 ([0.25, 0.5]) and 2
    ([0.5, 0.75]) and stay 0.0625 away from cells 0 and 3.  At z = 0.375 the square lies inside layer 1 alone; at z = 0.5 it lies in
    the face that layers 1 and 2 share, and touching counts."""
    for z, layers in ((0.375, [1]), (0.5, [1, 2])):
        a, b = 0.3125, 0.6875
        pos = np.float32([[[a, a, z], [b, a, z], [b, b, z]], [[a, a, z], [b, b, z], [a, b, z]]])
        sc, _ = flat_scene(pos)
        vox = renderer.voxelize(sc, 4, lo=(0, 0, 0), hi=(1, 1, 1))
        assert vox.dtype == torch.bool and tuple(vox.shape) == (4, 4, 4) and vox.device == torch.device(DEV)
        want = np.zeros((4, 4, 4), bool)                                         # [Z, Y, X]
        for layer in layers:
            want[layer, 1:3, 1:3] = True
        assert (vox.cpu().numpy() == want).all(), z
        # the same boxes through overlapsAny: centres lo + (i + 0.5) * 0.25, halves 0.125, x fastest
        k = (np.arange(4, dtype=np.float32) + np.float32(0.5)) * np.float32(0.25)
        zz, yy, xx = np.meshgrid(k, k, k, indexing="ij")
        centers = np.stack([xx, yy, zz], axis=-1).reshape(-1, 3)
        hit = renderer.overlapsAny(sc, centers, np.full_like(centers, 0.125))
        assert (hit.reshape(4, 4, 4) == want).all()
        # an uneven resolution (X, Y, Z) = (2, 4, 1): cells 0.5 x 0.25 x 1
        vox = renderer.voxelize(sc, (2, 4, 1), lo=(0, 0, 0), hi=(1, 1, 1)).cpu().numpy()
        assert vox.shape == (1, 4, 2) and (vox[0] == [[False, False], [True, True], [True, True], [False, False]]).all()
    # the scene's own bounds by default: every cell of a 2 x 2 x 1 grid over the square touches it
    assert renderer.voxelize(sc, (2, 2, 1)).all()


def test_queries_leave_the_renderer_alone_and_work_on_a_sharded_one(renderer, batch):
    sc, g, boxes, totals, lists, table = batch
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
            assert (r.overlapBoxes(sc, boxes, k=4).prim.reshape(-1) == table).all()
            assert (r.overlapBoxes(sc, boxes).prim == lists).all() and (r.overlapsAny(sc, boxes) == (totals > 0)).all()
            assert r.kernelInfo() == info and r.getSampleCount() == n and r.kernelSpanMs() == span
            assert r.GetRenderTargetImage().tobytes() == frame.tobytes() and r.GetAccumulationBuffer().tobytes() == accum.tobytes()
        r.Render(cam, sc)
        images.append((r.GetRenderTargetImage(), r.getSampleCount()))
    assert images[0][0].tobytes() == images[1][0].tobytes() and images[0][1] == images[1][1]
    r = drt.Renderer(0)
    r.setShard(8, 1, 2)
    r.ResizeBuffer(96, 64)
    got = r.overlapBoxes(sc, boxes, k=4)
    assert (got.prim.reshape(-1) == table).all() and (got.count.view(np.uint32) == totals).all()
    assert (r.overlapsAny(sc, boxes) == (totals > 0)).all()


def test_an_empty_scene_lists_nothing(renderer, batch):
    sc = drt.Scene()
    sc.addMaterial(*ONE_MATERIAL[0])
    sc.setGeometry(np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 2), np.float32), np.zeros(0, np.int32))
    drt.BVHBuilder().buildIterative(sc)
    boxes = batch[2]
    got = renderer.overlapBoxes(sc, boxes, k=3)
    assert (got.prim == -1).all() and not got.count.any()
    whole = renderer.overlapBoxes(sc, boxes)
    assert whole.splits.shape == (258,) and not whole.splits.any() and len(whole.prim) == 0 and whole.prim.dtype == np.int32
    assert not renderer.overlapsAny(sc, boxes).any()


def test_error_paths(renderer, batch):
    sc, g, ref_boxes, totals, lists, table = batch
    dev = torch.device(DEV)
    n = 64
    boxes = torch.zeros((n + 1, 16), dtype=torch.float32, device=dev)
    boxes[:, 3:6], boxes[:, 6], boxes[:, 10], boxes[:, 14] = 1, 1, 1, 1
    offsets = (torch.arange(n + 2, dtype=torch.int32, device=dev) * 2)
    prims = torch.full((2 * n + 8,), SENTINEL, dtype=torch.int32, device=dev)
    counts = torch.full((n + 1,), -1, dtype=torch.int32, device=dev)
    host = np.zeros((2 * n + 8, 16), np.float32)
    L, h = drt._lib, renderer._h
    INV = drt.ERR_INVALID
    cap = 2 * n
    B, O, P, C, H = boxes.data_ptr(), offsets.data_ptr(), prims.data_ptr(), counts.data_ptr(), host.ctypes.data
    for what, args in (("null boxes", (h, sc._h, None, O, P, cap, C, n, 0)), ("null offsets", (h, sc._h, B, None, P, cap, C, n, 0)),
                       ("null renderer", (None, sc._h, B, O, P, cap, C, n, 0)), ("null scene", (h, None, B, O, P, cap, C, n, 1)),
                       ("mode 2", (h, sc._h, B, O, P, cap, C, n, 2)), ("mode -1", (h, sc._h, B, O, P, cap, C, n, -1)),
                       ("mode 2, n = 0", (h, sc._h, B, O, P, cap, C, 0, 2)), ("mode 2, null boxes", (h, sc._h, None, O, P, cap, C, n, 2)),
                       ("both outputs null", (h, sc._h, B, O, None, 0, None, n, 0)), ("null prims with a capacity", (h, sc._h, B, O, None, cap, C, n, 0)),
                       ("prims without a capacity", (h, sc._h, B, O, P, 0, C, n, 0)),
                       ("any with prims", (h, sc._h, B, O, P, cap, C, n, 1)), ("any with a capacity", (h, sc._h, B, O, None, cap, C, n, 1)),
                       ("any without counts", (h, sc._h, B, O, None, 0, None, n, 1)),
                       ("misaligned boxes", (h, sc._h, B + 4, O, P, cap, C, n, 0)), ("misaligned prims", (h, sc._h, B, O, P + 2, cap, C, n, 0)),
                       ("misaligned offsets", (h, sc._h, B, O + 2, P, cap, C, n, 0)), ("misaligned counts", (h, sc._h, B, O, P, cap, C + 1, n, 0)),
                       ("host boxes", (h, sc._h, H, O, P, cap, C, n, 0)), ("host offsets", (h, sc._h, B, H, P, cap, C, n, 0)),
                       ("host prims", (h, sc._h, B, O, H, cap, C, n, 0)), ("host counts", (h, sc._h, B, O, P, cap, H, n, 0)),
                       ("host counts, any", (h, sc._h, B, None, None, 0, H, n, 1)), ("null handles, n = 0", (None, None, B, O, P, cap, C, 0, 0))):
        assert L.drt_renderer_overlap_boxes(*args, None) == INV, what
        if what.startswith("mode"):
            assert b"mode" in L.drt_last_error(), what                                                    # checked first after the handles
    for mode in (0, 1):
        assert L.drt_renderer_overlap_boxes(h, sc._h, None, None, None, 0, None, 0, mode, None) == drt.OK   # n == 0: nothing to do
        assert L.drt_renderer_overlap_boxes(h, sc._h, B, O, P, cap, C, 0, mode, None) == drt.OK
    torch.cuda.synchronize()
    assert (prims == SENTINEL).all() and (counts == -1).all()                                              # nothing was launched
    # boxes need 16-byte alignment, the rest 4: one box and one word further on.  Every box is the unit cube about the origin.
    assert L.drt_renderer_overlap_boxes(h, sc._h, B + 64, O + 4, P + 4, cap + 2, C + 4, n, 0, None) == drt.OK
    torch.cuda.synchronize()
    assert prims[0] == SENTINEL and (prims[1:1 + 2] == SENTINEL).all() and (prims[1 + 2 + 2 * n:] == SENTINEL).all()
    assert not (prims[1 + 2:1 + 2 + 2 * n] == SENTINEL).any() and counts[0] == -1 and (counts[1:] >= 0).all()
    empty = renderer.overlapBoxes(sc, np.zeros((0, 16), np.float32))
    assert empty.splits.tolist() == [0] and len(empty.prim) == 0
    assert renderer.overlapBoxes(sc, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), k=5).prim.shape == (0, 5)
    assert renderer.overlapsAny(sc, np.zeros((0, 16), np.float32)).shape == (0,)
    c, hh = boxes[:, 0:3].contiguous(), boxes[:, 3:6].contiguous()
    for bad in (lambda: renderer.overlapBoxes(sc, boxes, k=0),
                lambda: renderer.overlapBoxes(sc, boxes.cpu()),                                          # wrong device
                lambda: renderer.overlapBoxes(sc, boxes.double()),                                       # wrong dtype
                lambda: renderer.overlapBoxes(sc, boxes[:, :15]),                                        # wrong shape
                lambda: renderer.overlapBoxes(sc, c),                                                    # a centre without a half
                lambda: renderer.overlapBoxes(sc, c, hh[:10]),                                           # mismatched counts
                lambda: renderer.overlapBoxes(sc, c, hh, boxes[:, 6:14]),                                # axes of the wrong shape
                lambda: renderer.overlapBoxes(sc, c.cpu().numpy(), hh),                                  # numpy mixed with device tensors
                lambda: renderer.overlapBoxes(sc, boxes, axes=boxes[:, 6:15].reshape(-1, 3, 3)),         # packed boxes carry their axes
                lambda: renderer.overlapBoxes(sc, c, hh, lo=c, hi=c),                                    # both forms
                lambda: renderer.overlapBoxes(sc, lo=c),                                                 # lo without hi
                lambda: renderer.overlapBoxes(sc),
                lambda: renderer.overlapsAny(sc, boxes.cpu()),
                lambda: renderer.overlapsAny(sc, c, hh[:10]),
                lambda: renderer.voxelize(sc, 0),
                lambda: renderer.overlapBoxes(sc, host.astype(np.float64))):
        with pytest.raises(drt.DrtError) as e:
            bad()
        assert e.value.code == INV
    # a pending asynchronous batch
    r = drt.Renderer(0)
    r.ResizeBuffer(64, 32)
    r.RenderBatchAsync(drt.Camera(SCENES["cornell_box"][1]), sc, 1)
    for call in (lambda: r.overlapBoxes(sc, boxes, k=2), lambda: r.overlapBoxes(sc, boxes), lambda: r.overlapsAny(sc, boxes)):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == INV
    assert raw(r, sc, boxes, offsets, prims, cap, counts, n, 0) == INV
    r.Wait()
    r.overlapBoxes(sc, boxes, k=2), r.overlapsAny(sc, boxes)
    # a tree deeper than 64 levels: the chain's centroids double per triangle (scaled down so that no area overflows)
    chain = list(rq.degenerate_chain(110))
    chain[0] = (chain[0] * np.float32(2.0 ** -55)).astype(np.float32)
    deep, _ = rq.programmatic_scene(drt, *chain, 1, 2)
    assert deep.bvh_depth > 64
    for call in (lambda: renderer.overlapBoxes(deep, boxes, k=2), lambda: renderer.overlapsAny(deep, boxes)):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == drt.ERR_UNSUPPORTED
    assert (renderer.overlapBoxes(sc, ref_boxes, k=4).prim.reshape(-1) == table).all()                    # after the errors
