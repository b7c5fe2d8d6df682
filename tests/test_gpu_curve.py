"""Intersection curves on the GPU (drt_renderer_chain_intersections, kernel_curve.hip and the phases it shares with kernel_contour.hip;
Renderer.chainIntersections / intersectionCurves, CurveList.lengths): every word of every slot and of counts bit-equal to the sequential
walk of tests/curve_ref.py, on the device's own drt_renderer_intersect_triangles output for the meshes of tests/curve_scenes.py -- spheres
in general position (one closed loop across hundreds of queries), aligned copies (open chains, statuses 3 and 4), open, non-manifold and
flipped meshes, and the band cut by one triangle at the totals round a lane, a workgroup, a scan block and three scan blocks; records
that are not live in the middle of the order, decreasing and overlapping splits, a clamped total, broken tables; two runs; a refitted
device copy; the section contours unchanged beside it; the Python lists.  tests/test_curve_ref.py asserts what the restatement does."""
import numpy as np
import pytest

from tests import contour_ref as cr
from tests import contour_scenes as cs
from tests import curve_ref as cu
from tests import curve_scenes as cv
from tests import intersect_ref as ir
from tests import nearest_ref as nr
from tests import section_ref as sr

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -77                                                                 # contour_ref.UNTOUCHED as an int32
_ref = {}


@pytest.fixture(scope="module")
def renderer():
    return drt.Renderer(0)


def records_of(cuts):
    """float32 [M, 8]: a numpy CutList packed as drt_isect."""
    rec = np.zeros((len(cuts.prim), 8), np.float32)
    rec[:, 0:3], rec[:, 4:7] = cuts.p, cuts.q
    rec.view(np.int32)[:, 3], rec.view(np.int32)[:, 7] = cuts.prim, cuts.code
    return rec


def reference(renderer, name):
    """(scene, query triangles, adjacency, query table, the device's records [M, 8], splits, slots, counts) of a case, made once: the
    records are the device's own, the two tables are dictionaries, the chains are the sequential walk."""
    if name not in _ref:
        pos, tris = cv.case(name)
        sc, _ = cs.flat_scene(drt, pos)
        cuts = renderer.intersectTriangles(sc, tris)
        rec, splits = records_of(cuts), cuts.splits.astype(np.int64)
        adj, query_adj = cr.adjacency(cs.tree_positions(sc)), cu.tri_adjacency(tris)
        words = rec.view(np.int32)
        _ref[name] = (sc, tris, adj, query_adj, rec, splits) + cu.chain(adj, query_adj, words[:, 3], words[:, 7], splits, len(pos))
    return _ref[name]


def run_raw(r, sc, rec, splits, query_adj, total=None, with_counts=True, room=8):
    """One call on sentinel-filled buffers: (slots as SLOT over the record buffer and `room` slots behind it, counts [3] or None)."""
    n = len(splits) - 1
    total = len(rec) if total is None else total
    segs = torch.from_numpy(np.ascontiguousarray(rec).view(np.int32).reshape(-1, 8)).to(DEV)
    spl = torch.from_numpy(np.asarray(splits).astype(np.int32)).to(DEV)
    table = torch.from_numpy(np.ascontiguousarray(query_adj, np.int32).reshape(-1)).to(DEV)
    slots = torch.full((len(rec) + room, 4), SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.full((3,), -1, dtype=torch.int32, device=DEV) if with_counts else None
    rc = drt._lib.drt_renderer_chain_intersections(r._h, sc._h, segs.data_ptr(), spl.data_ptr(), table.data_ptr(), slots.data_ptr(),
                                                   None if counts is None else counts.data_ptr(), n, total, None)
    assert rc == drt.OK, drt._lib.drt_last_error()
    torch.cuda.synchronize()
    return slots.cpu().numpy().view(cr.SLOT).reshape(-1), (None if counts is None else counts.cpu().numpy().view(np.uint32))


def padded(want, length):
    """The restatement's slots followed by untouched ones, `length` in all."""
    out = np.zeros(length, cr.SLOT)
    for f in cr.SLOT.names:
        out[f] = cr.UNTOUCHED
    out[:len(want)] = want
    return out


def restated(ref, rec, splits, query_adj=None, total=None):
    sc, tris, adj, own_table = ref[:4]
    words = np.ascontiguousarray(rec).view(np.int32).reshape(-1, 8)
    return cu.chain(adj, own_table if query_adj is None else query_adj, words[:, 3], words[:, 7], np.asarray(splits), len(adj) // 3, total)


def expected_lists(rec, splits, slots):
    """What Renderer.chainIntersections returns, from the restatement's slots: the CurveList fields as host arrays."""
    status = (slots["flags"] >> 1).astype(np.int32)
    kept = status != cu.NOT_LIVE
    starts = (slots["first"] == np.arange(len(slots))) & kept
    seg = slots["seg"][kept].astype(np.int64)
    before = np.cumsum(kept) - kept
    words = rec.view(np.int32)
    query = np.searchsorted(np.asarray(splits)[1:], seg, side="right").astype(np.int32)
    return (np.concatenate([before[starts], [kept.sum()]]).astype(np.int32), (slots["flags"][starts] & 1).astype(bool), rec[seg, 0:3], rec[seg, 4:7],
            query, words[seg, 3], words[seg, 7], status[kept])


def same_lists(got, want):
    got = [x.cpu().numpy() if torch.is_tensor(x) else x for x in got]
    return all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(got, want))


@pytest.mark.parametrize("name", cv.NAMES)
def test_every_slot_and_count_is_bit_equal_to_the_restatement(renderer, name):
    ref = reference(renderer, name)
    sc, tris, adj, query_adj, rec, splits, want, want_counts = ref
    total = len(rec)
    chains = cu.chain_lists(want)
    print("%s: %d queries, %d records, counts %s, the longest chain %d; statuses %s"
          % (name, len(tris), total, want_counts.tolist(), max(len(c[0]) for c in chains), np.bincount(want["flags"] >> 1, minlength=6).tolist()))
    assert total > 0 and (sc.edgeAdjacency().reshape(-1) == adj).all()
    slots, counts = run_raw(renderer, sc, rec, splits, query_adj)
    assert slots.tobytes() == padded(want, total + 8).tobytes() and counts.tobytes() == want_counts.tobytes(), name
    # counts NULL: the same slots
    again, none = run_raw(renderer, sc, rec, splits, query_adj, with_counts=False)
    assert none is None and again.tobytes() == slots.tobytes()
    # what the case is about
    if name.startswith("spheres"):
        assert want_counts.tolist() == [1, 1, 0] and (want["flags"] == 1).all() and len(chains[0][0]) == total >= 90
    if name.startswith("aligned"):
        status = set((want["flags"] >> 1).tolist())
        assert cu.NOT_LISTED in status and cu.OTHER_EDGES in status and want_counts[0] > want_counts[1]
    if name.startswith("tube") and name[4:].isdigit():
        assert total == 2 * int(name[4:]) and want_counts.tolist() == [1, 1, 0]          # a single loop of 2 m records
    if name == "tube_quad":                                                    # the loop changes query twice
        query = np.searchsorted(splits[1:], chains[0][0], side="right")
        assert want_counts.tolist() == [1, 1, 0] and (query != np.roll(query, -1)).sum() == 2
    if name in ("book", "tube_flipped"):
        assert ((want["flags"] >> 1) == cu.NON_MANIFOLD).any()
    if name in ("strip", "poke", "single", "quad"):
        assert want_counts.tolist() == [1, 0, 0] and want[-1]["flags"] >> 1 == cu.BOUNDARY
        assert total == {"single": 1, "quad": 2}.get(name, total)


@pytest.mark.parametrize("name", ["spheres1", "tube_quad", "aligned_x", "tube1537"])
def test_the_python_lists_and_their_lengths(renderer, name):
    sc, tris, adj, query_adj, rec, splits, want, _ = reference(renderer, name)
    lists = expected_lists(rec, splits, want)
    got = renderer.intersectionCurves(sc, tris)                                 # numpy in, numpy out
    assert isinstance(got, drt.CurveList) and isinstance(got.p, np.ndarray) and same_lists(got, lists), name
    dev_tris = torch.from_numpy(tris).to(DEV)
    dev = renderer.intersectionCurves(sc, dev_tris, query_adj=torch.from_numpy(query_adj.reshape(-1, 3)).to(DEV))
    assert all(x.device == torch.device(DEV) for x in dev) and same_lists(dev, lists), name
    cuts = renderer.intersectTriangles(sc, dev_tris)
    assert same_lists(renderer.chainIntersections(sc, cuts, tris=dev_tris), lists)
    assert same_lists(renderer.chainIntersections(sc, renderer.intersectTriangles(sc, tris), query_adj=query_adj.reshape(-1, 3)), lists)
    with pytest.raises(drt.DrtError) as e:
        renderer.chainIntersections(sc, cuts)                                   # neither the mesh nor its table
    assert e.value.code == drt.ERR_INVALID
    with pytest.raises(drt.DrtError):
        renderer.chainIntersections(sc, cuts, query_adj=query_adj[:-3])         # a table of another mesh
    assert drt.triEdgeAdjacency(dev_tris).device == torch.device(DEV) and drt.triEdgeAdjacency(dev_tris).cpu().numpy().tobytes() == query_adj.tobytes()
    # lengths: the sum of |q - p| per chain in float64.  Each term is a float64 square root of exact sums of squares of float32
    # differences; only the order of at most 3074 additions differs, which is worth 3074 * 2^-53 of the sum: 1e-12 is owed
    p, q = lists[2].astype(np.float64), lists[3].astype(np.float64)
    each = np.sqrt(((q - p) ** 2).sum(axis=1))
    at = lists[0]
    want_lengths = np.asarray([each[at[c]:at[c + 1]].sum() for c in range(len(at) - 1)], np.float64)
    got_lengths = got.lengths()
    assert got_lengths.dtype == np.float64 and got_lengths.shape == want_lengths.shape
    assert (np.abs(got_lengths - want_lengths) <= 1e-12 * want_lengths).all()
    on_device = dev.lengths()
    assert on_device.device == torch.device(DEV) and on_device.dtype == torch.float64
    assert (np.abs(on_device.cpu().numpy() - want_lengths) <= 1e-12 * np.maximum(want_lengths, want_lengths.sum())).all()
    if name == "tube1537":                                                      # the band's section: a 1537-gon of radius 16
        assert len(got_lengths) == 1 and abs(got_lengths[0] - 2 * np.pi * 16) < 0.05


def oversized_fill(renderer, sc, tris, splits, extra):
    """The device's fill of the same queries into ranges `extra[i]` records longer than their lists: (records, splits), with miss
    records behind every list."""
    n = len(tris)
    caps = np.diff(splits) + extra
    wide = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    packed = torch.zeros((n, 12), dtype=torch.float32, device=DEV)
    packed[:, 0:9] = torch.from_numpy(tris.reshape(n, 9)).to(DEV)
    offsets = torch.from_numpy(wide.astype(np.int32)).to(DEV)
    out = torch.full((int(wide[-1]), 8), 7.0, dtype=torch.float32, device=DEV)
    rc = drt._lib.drt_renderer_intersect_triangles(renderer._h, sc._h, packed.data_ptr(), offsets.data_ptr(), out.data_ptr(), int(wide[-1]), None, n, None)
    assert rc == drt.OK, drt._lib.drt_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy(), wide


@pytest.mark.parametrize("name", ["spheres2", "aligned_x", "tube_quad"])
def test_records_that_are_not_live(renderer, name):
    ref = reference(renderer, name)
    sc, tris, adj, query_adj, rec, splits, tight, tight_counts = ref
    n, total = len(tris), len(rec)
    # miss records in the middle of the order: every third range two records too long
    extra = np.where(np.arange(n) % 3 == 0, 2, 0)
    wide_rec, wide = oversized_fill(renderer, sc, tris, splits, extra)
    want, want_counts = restated(ref, wide_rec, wide)
    assert want_counts[2] == extra.sum() and want_counts[:2].tolist() == tight_counts[:2].tolist()
    dead, live = np.nonzero((want["flags"] >> 1) == cu.NOT_LIVE)[0], np.nonzero((want["flags"] >> 1) != cu.NOT_LIVE)[0]
    assert want["seg"][live].min() < want["seg"][dead].max() and want["seg"][dead].min() < want["seg"][live].max()      # dead records between live ones
    if name == "aligned_x":                                                    # many chains: some stand behind dead records in the order, too
        assert live.min() < dead.max() and dead.min() < live.max()
    slots, counts = run_raw(renderer, sc, wide_rec, wide, query_adj)
    assert slots.tobytes() == padded(want, len(wide_rec) + 8).tobytes() and counts.tobytes() == want_counts.tobytes()
    # the lists drop them: the tight fill's curves
    cuts = drt.CutList(wide.astype(np.int32), wide_rec[:, 0:3].copy(), wide_rec[:, 4:7].copy(), wide_rec.view(np.int32)[:, 3].copy(),
                       wide_rec.view(np.int32)[:, 7].copy())
    got = renderer.chainIntersections(sc, cuts, tris=tris)
    assert same_lists(got, expected_lists(wide_rec, wide, want)) and len(got.prim) == total
    assert same_lists(got[:4] + got[5:], expected_lists(rec, splits, tight)[:4] + expected_lists(rec, splits, tight)[5:])
    # decreasing and overlapping splits over the tight fill
    if n > 2:
        for broken in (splits[::-1].copy(), np.concatenate([splits[:n // 2], splits[n // 2:] - min(5, total // 4)]).clip(0),
                       np.concatenate([[3], splits[1:n // 3], [splits[n // 3 - 1]], splits[n // 3 + 1:]])):
            want, want_counts = restated(ref, rec, broken)
            slots, counts = run_raw(renderer, sc, rec, broken, query_adj)
            assert slots.tobytes() == padded(want, total + 8).tobytes() and counts.tobytes() == want_counts.tobytes()
    for broken in ([splits[-1], 0] + [0] * (n - 1), [0] + [2 * total] * n, [1] + list(splits[1:])):
        want, want_counts = restated(ref, rec, broken)
        slots, counts = run_raw(renderer, sc, rec, broken, query_adj)
        assert slots.tobytes() == padded(want, total + 8).tobytes() and counts.tobytes() == want_counts.tobytes()
    # a total stated smaller than the last splits: nothing at or beyond it is read or written
    for stated in (1, total // 2, total - 1):
        want, want_counts = restated(ref, rec, splits, total=stated)
        slots, counts = run_raw(renderer, sc, rec, splits, query_adj, total=stated)
        assert len(want) == stated and slots.tobytes() == padded(want, total + 8).tobytes() and counts.tobytes() == want_counts.tobytes()
        assert (slots[stated:].view(np.int32) == SENTINEL).all()
    # code digits and prims that name nothing
    bent = rec.copy()
    w = bent.view(np.int32)
    w[1, 7], w[total // 2, 7], w[total - 2, 3], w[total // 3, 7] = 3, 7 << 4, len(adj) // 3, -1
    want, want_counts = restated(ref, bent, splits)
    slots, counts = run_raw(renderer, sc, bent, splits, query_adj)
    assert want_counts[2] == 4 and slots.tobytes() == padded(want, total + 8).tobytes() and counts.tobytes() == want_counts.tobytes()


def test_broken_tables_and_repeated_prims_give_simple_paths(renderer):
    ref = reference(renderer, "tube_quad")
    sc, tris, adj, query_adj, rec, splits, tight, _ = ref
    total = len(rec)
    twice = rec.copy()
    twice.view(np.int32)[5, 3] = twice.view(np.int32)[4, 3]
    for table, records in ((np.full_like(query_adj, 3), rec), (np.full_like(query_adj, 6), rec), (np.full_like(query_adj, -7), rec),
                           (np.int32([1, 1, 1, 1, 1, 1]), rec), (query_adj, twice)):
        want, want_counts = restated(ref, records, splits, query_adj=table)
        slots, counts = run_raw(renderer, sc, records, splits, table)
        assert sorted(slots["seg"][:total].tolist()) == list(range(total)) and (slots["first"][:total] < total).all()
        assert slots.tobytes() == padded(want, total + 8).tobytes() and counts.tobytes() == want_counts.tobytes()
    # the same prim in every record of a range: every record of the other query that leaves through the diagonal claims the first
    same = rec.copy()
    same.view(np.int32)[:splits[1], 3] = same.view(np.int32)[0, 3]
    want, want_counts = restated(ref, same, splits)
    slots, counts = run_raw(renderer, sc, same, splits, query_adj)
    assert slots.tobytes() == padded(want, total + 8).tobytes() and counts.tobytes() == want_counts.tobytes()


def test_two_runs_give_the_same_bytes(renderer):
    for name in ("spheres3", "aligned_z", "tube1537"):
        sc, tris, adj, query_adj, rec, splits, want, want_counts = reference(renderer, name)
        runs = [run_raw(renderer, sc, rec, splits, query_adj) for _ in range(2)]
        assert runs[0][0].tobytes() == runs[1][0].tobytes() == padded(want, len(rec) + 8).tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
        a, b = renderer.intersectionCurves(sc, tris), renderer.intersectionCurves(sc, tris)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_after_a_refit_the_chains_follow_the_moved_geometry():
    pos, tris = cv.case("spheres1")
    sc, _ = cs.flat_scene(drt, pos)
    moved = (pos + np.float32(0.05) * np.sin(pos[..., [1, 2, 0]] * np.float32(7))).astype(np.float32)     # a function of the position: shared stays shared
    host, _ = cs.flat_scene(drt, pos)
    host.refit(moved)
    adj = cr.adjacency(cs.tree_positions(sc))
    assert (cr.adjacency(cs.tree_positions(host)) == adj).all()                # the deformation keeps the table
    query_adj = cu.tri_adjacency(tris)
    r = drt.Renderer(0)
    before = r.intersectionCurves(sc, tris)
    r.refit(sc, torch.from_numpy(moved).to(DEV))
    cuts = r.intersectTriangles(sc, tris)                                       # the refitted copy's segments
    moved_splits, moved_rec = ir.whole(nr.from_product(host), tris)             # the restatement on the refitted positions
    assert (cuts.splits == moved_splits).all() and records_of(cuts).tobytes() == moved_rec.tobytes()
    rec, splits = records_of(cuts), cuts.splits.astype(np.int64)
    want, want_counts = cu.chain(adj, query_adj, cuts.prim, cuts.code, splits, len(pos))      # ... chained by the host scene's table
    slots, counts = run_raw(r, sc, rec, splits, query_adj)
    assert slots.tobytes() == padded(want, len(rec) + 8).tobytes() and counts.tobytes() == want_counts.tobytes()
    after = r.intersectionCurves(sc, tris)
    assert same_lists(after, expected_lists(rec, splits, want)) and not same_lists(after, before)
    assert want_counts[0] >= 1 and len(rec) > 50


def test_the_section_contours_are_unchanged_beside_a_curve_call(renderer):
    """The two calls share their scratch and every phase behind the link: a plane's contours before and after curve calls of other
    sizes, against the contours' own restatement."""
    for name, planes in (("ring", sr.pack([(0, 0, 1), (0, 0, -1), (0, 0, 2)], [0, 0, 1])), ("hollow_box", sr.pack([(0, 0, 1), (1, 0, 0), (0, 0, 1)], [0, 0.5, 1.5]))):
        sc, g = cs.scene(drt, name)
        before = renderer.contours(sc, planes)
        rec, totals = sr.whole(g, planes)
        splits = np.concatenate([[0], np.cumsum(totals.astype(np.int64))])
        want, want_chains = cr.chain(cr.adjacency(cs.tree_positions(sc)), rec, splits)
        for other in ("tube1537", "single", "spheres1"):
            o = reference(renderer, other)
            slots, _ = run_raw(renderer, o[0], o[4], o[5], o[3])
            assert slots[:len(o[4])].tobytes() == o[6].tobytes()
            after = renderer.contours(sc, planes)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after)), (name, other)
        # the slots themselves, through the entry point
        segs = torch.from_numpy(np.ascontiguousarray(rec).view(np.int32).reshape(-1, 8)).to(DEV)
        spl = torch.from_numpy(splits.astype(np.int32)).to(DEV)
        out = torch.full((len(rec), 4), SENTINEL, dtype=torch.int32, device=DEV)
        chains = torch.full((len(planes), 2), -1, dtype=torch.int32, device=DEV)
        assert drt._lib.drt_renderer_chain_sections(renderer._h, sc._h, segs.data_ptr(), spl.data_ptr(), out.data_ptr(), chains.data_ptr(), len(planes), len(rec),
                                                    None) == drt.OK
        torch.cuda.synchronize()
        assert out.cpu().numpy().view(cr.SLOT).reshape(-1).tobytes() == want.tobytes() and (chains.cpu().numpy().view(np.uint32) == want_chains).all()


def test_nothing_to_do_and_the_error_codes(renderer):
    sc, tris, adj, query_adj, rec, splits, _, _ = reference(renderer, "quad")
    far = (tris + np.float32(50)).astype(np.float32)
    got = renderer.intersectionCurves(sc, far)                                  # no record at all
    assert got.chain_splits.tolist() == [0] and got.p.shape == (0, 3) and got.lengths().shape == (0,)
    none = renderer.intersectionCurves(sc, np.zeros((0, 3, 3), np.float32))
    assert none.chain_splits.tolist() == [0] and none.closed.shape == (0,)
    host = torch.zeros(64, dtype=torch.int32)                                   # host memory where device memory belongs
    segs = torch.zeros((2, 8), dtype=torch.float32, device=DEV)
    spl = torch.tensor([0, 2], dtype=torch.int32, device=DEV)
    table = torch.full((3,), -1, dtype=torch.int32, device=DEV)
    slots = torch.zeros((2, 4), dtype=torch.int32, device=DEV)
    L = drt._lib
    fn = lambda s, p, t, o, c: L.drt_renderer_chain_intersections(renderer._h, sc._h, s.data_ptr(), p.data_ptr(), t.data_ptr(), o.data_ptr(), c, 1, 2, None)
    assert fn(segs, spl, table, slots, None) == drt.OK
    for args in ((host, spl, table, slots, None), (segs, host, table, slots, None), (segs, spl, host, slots, None), (segs, spl, table, host, None),
                 (segs, spl, table, slots, host.data_ptr())):
        assert fn(*args) == drt.ERR_INVALID and b"device memory" in L.drt_last_error()
