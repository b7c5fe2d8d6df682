"""Section contours on the GPU (drt_renderer_chain_sections, kernel_contour.hip; Renderer.chainSections / contours, ContourList.areas):
every slot and every count bit-equal to the sequential walk of tests/contour_ref.py -- over the small meshes of tests/contour_scenes.py
(the 5 000-record ring takes all 13 jumping rounds), cornell_box, the soup, the fan and the degenerate mesh; ranges with trailing miss
records, truncated and empty ranges, a clamped total; one plane, and 500 planes permuted and run twice; chains NULL; a refitted device
copy; the Python lists; the areas of the chains; unsorted input; the renderer's state untouched; an empty scene; the error codes.
tests/test_contour_ref.py asserts what the restatement does."""
import numpy as np
import pytest

from tests import contour_ref as cr
from tests import contour_scenes as cs
from tests import nearest_ref as nr
from tests import ray_query_ref as rq
from tests import refit_ref as rf
from tests import section_ref as sr
from tests.scenes import SCENES, scene_path

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -77
_ref = {}


@pytest.fixture(scope="module")
def renderer():
    return drt.Renderer(0)


def csr(totals):
    return np.concatenate([[0], np.cumsum(np.asarray(totals).astype(np.int64))])


def reference(name):
    """(scene, Geometry, planes, records, totals, adjacency, slots, chains) of a scene and its planes, computed once."""
    if name not in _ref:
        sc, g = cs.scene(drt, name)
        planes = cs.planes(name, g)
        if name == "degenerate":
            planes = np.concatenate([planes, cs.degenerate_planes()])
        rec, totals = sr.whole(g, planes)
        adj = cr.adjacency(cs.tree_positions(sc))
        slots, chains = cr.chain(adj, rec, csr(totals))
        _ref[name] = (sc, g, planes, rec, totals, adj, slots, chains)
    return _ref[name]


def raw(r, sc, segs, splits, slots, chains, n, total, stream=None):
    """The entry point itself on device tensors (or None): the status code."""
    ptr = lambda x: None if x is None else x.data_ptr()
    return drt._lib.drt_renderer_chain_sections(r._h, sc._h, ptr(segs), ptr(splits), ptr(slots), ptr(chains), n, total, stream)


def run_raw(r, sc, rec, splits, total=None, with_chains=True):
    """One call on sentinel-filled buffers: (slots as SLOT over the whole record buffer, chains [n, 2] or None) as host arrays."""
    n = len(splits) - 1
    total = len(rec) if total is None else total
    segs = torch.from_numpy(np.ascontiguousarray(rec).view(np.int32).reshape(-1, 8)).to(DEV)
    spl = torch.from_numpy(np.asarray(splits).astype(np.int32)).to(DEV)
    slots = torch.full((max(len(rec), 1), 4), SENTINEL, dtype=torch.int32, device=DEV)
    chains = torch.full((n, 2), -1, dtype=torch.int32, device=DEV) if with_chains else None
    assert raw(r, sc, segs, spl, slots, chains, n, total) == drt.OK
    torch.cuda.synchronize()
    return slots.cpu().numpy().view(cr.SLOT).reshape(-1)[:len(rec)], (None if chains is None else chains.cpu().numpy().view(np.uint32))


def expected_lists(rec, slots, chains):
    """What Renderer.chainSections returns, from the restatement's slots: the ContourList fields as host arrays."""
    status = (slots["flags"] >> 1).astype(np.int32)
    kept = status != cr.MISS
    starts = (slots["first"] == np.arange(len(slots))) & kept
    seg = slots["seg"][kept].astype(np.int64)
    before = np.cumsum(kept) - kept
    return (csr(chains[:, 0]).astype(np.int32), np.concatenate([before[starts], [kept.sum()]]).astype(np.int32), (slots["flags"][starts] & 1).astype(bool),
            rec["p"][seg], rec["q"][seg], rec["prim"][seg], rec["code"][seg], status[kept])


def same_lists(got, want):
    got = [x.cpu().numpy() if torch.is_tensor(x) else x for x in got]
    return all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(got, want))


@pytest.mark.parametrize("name", cs.ALL_NAMES)
def test_every_slot_and_count_is_bit_equal_to_the_restatement(renderer, name):
    sc, g, planes, rec, totals, adj, want, want_chains = reference(name)
    splits = csr(totals)
    lengths = want["length"][want["first"] == np.arange(len(want))]
    print("%s: %d planes, %d records, %d chains (%d closed), the longest %d; statuses %s"
          % (name, len(planes), len(rec), want_chains[:, 0].sum(), want_chains[:, 1].sum(), lengths.max(initial=0),
             np.bincount(want["flags"] >> 1, minlength=6).tolist()))
    assert len(rec) > 0 and ((totals == 0).any() or name == "ring")
    assert (sc.edgeAdjacency().reshape(-1) == adj).all()
    slots, chains = run_raw(renderer, sc, rec, splits)
    assert slots.tobytes() == want.tobytes() and (chains == want_chains).all(), name
    if name == "ring":
        assert lengths.max() == 5000 and want_chains[0].tolist() == [1, 1]        # one closed chain: all 13 rounds
    if name in cs.EXACT_CLOSED:
        assert (slots["flags"] == 1).all() and (chains[:, 0] == chains[:, 1]).all()
    if name in ("book", "flipped_quad"):
        assert ((slots["flags"] >> 1) == cr.NON_MANIFOLD).any()
    if name in ("soup", "fan"):
        assert (lengths == 1).mean() > 0.5                                        # mostly chains of one
    if name in ("cornell_box", "degenerate"):
        assert len(set((slots["flags"] >> 1).tolist())) >= (3 if name == "degenerate" else 2) and lengths.max() > 2
    # chains NULL: the same slots
    again, none = run_raw(renderer, sc, rec, splits, with_chains=False)
    assert none is None and again.tobytes() == want.tobytes()
    # the Python lists: contours = planeSections followed by chainSections; numpy in, numpy out
    lists = expected_lists(rec, want, want_chains)
    got = renderer.contours(sc, planes)
    assert isinstance(got, drt.ContourList) and isinstance(got.p, np.ndarray) and same_lists(got, lists), name
    assert got.normals.tobytes() == planes[:, 0:3].tobytes()
    sec = renderer.planeSections(sc, torch.from_numpy(planes).to(DEV))
    dev = renderer.chainSections(sc, sec)
    assert all(x.device == torch.device(DEV) for x in dev) and dev.normals is None and same_lists(dev, lists), name
    assert same_lists(renderer.chainSections(sc, renderer.planeSections(sc, planes)), lists)
    assert same_lists(renderer.contours(sc, torch.from_numpy(planes[:, 0:3].copy()).to(DEV), torch.from_numpy(planes[:, 3].copy()).to(DEV)), lists)


@pytest.mark.parametrize("name", ["tetrahedron", "two_cubes", "cornell_box", "soup"])
def test_trailing_misses_truncated_and_empty_ranges(renderer, name):
    sc, g, planes, full, totals, adj, _, _ = reference(name)
    n = len(planes)
    rng = np.random.default_rng(5)
    caps = (totals.astype(np.int64) + rng.integers(-3, 4, n)).clip(0)
    caps[rng.integers(0, n, n // 6)] = 0                                       # empty ranges between full ones
    assert (caps > totals).any() and ((caps < totals) & (caps > 0)).any() and ((caps == 0) & (totals > 0)).any()
    lead, trail = 3, 5
    rec, _ = sr.sections(g, planes, caps)                                      # the restatement's fill at these capacities: prefixes, then misses
    buf = np.concatenate([np.repeat(sr.MISS, lead), rec, np.repeat(sr.MISS, trail)])
    buf[:lead]["prim"], buf[len(buf) - trail:]["prim"] = 0, 0                  # (records outside every range: never read)
    splits = lead + csr(caps)
    want, want_chains = cr.chain(adj, buf, splits)
    assert ((want["flags"] >> 1) == cr.MISS).any() and (((want["flags"] >> 1) == cr.NOT_LISTED).any() or name == "soup")   # (a soup shares no edge)
    slots, chains = run_raw(renderer, sc, buf, splits)
    assert (slots[:lead].view(np.int32) == SENTINEL).all() and (slots[len(buf) - trail:].view(np.int32) == SENTINEL).all()
    assert slots.tobytes() == want.tobytes() and (chains == want_chains).all()
    # a total stated smaller than the last splits, ending inside a range: nothing at or beyond it is read or written
    i = int(np.nonzero((caps >= 2) & (totals >= 1) & (np.arange(n) > n // 2))[0][0])
    stated = int(splits[i]) + 1
    want, want_chains = cr.chain(adj, buf, splits, total=stated)
    slots, chains = run_raw(renderer, sc, buf, splits, total=stated)
    assert (slots[stated:].view(np.int32) == SENTINEL).all() and not want_chains[i + 1:].any() and want_chains[i].tolist() == [1, 0]
    assert slots[:stated].tobytes() == want.tobytes() and (chains == want_chains).all()
    # a decreasing pair is an empty range: the first plane's and the last one's (their records then lie outside every range)
    broken = splits.copy()
    broken[0], broken[n] = broken[1] + 2, broken[n - 1] - 1
    want, want_chains = cr.chain(adj, buf, broken)
    slots, chains = run_raw(renderer, sc, buf, broken)
    assert not want_chains[0].any() and not want_chains[n - 1].any() and (want[:splits[1]].view(np.uint32) == cr.UNTOUCHED).all()
    assert slots.tobytes() == want.tobytes() and (chains == want_chains).all()


def test_one_plane_and_500_planes_permuted_twice(renderer):
    sc, g = cs.scene(drt, "cornell_box")
    rng = np.random.default_rng(31)
    nn = rng.normal(size=(500, 3)).astype(np.float32)
    planes = sr.pack(nn, nr.dot(nn, nr.box_points(g, 500, rng)))
    full, totals = sr.whole(g, planes)
    adj = cr.adjacency(cs.tree_positions(sc))
    start = csr(totals)
    want, want_chains = cr.chain(adj, full, start)
    slots, chains = run_raw(renderer, sc, full, start)
    assert slots.tobytes() == want.tobytes() and (chains == want_chains).all()
    perm = np.random.default_rng(2).permutation(len(planes))
    shuffled = np.concatenate([full[start[i]:start[i + 1]] for i in perm])
    want, want_chains = cr.chain(adj, shuffled, csr(totals[perm]))
    runs = [run_raw(renderer, sc, shuffled, csr(totals[perm])) for _ in range(2)]
    assert runs[0][0].tobytes() == runs[1][0].tobytes() == want.tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    assert (runs[0][1] == want_chains).all()
    a, b = renderer.contours(sc, planes[perm]), renderer.contours(sc, planes[perm])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and same_lists(a, expected_lists(shuffled, want, want_chains))
    # n = 1: the longest list alone
    i = int(totals.argmax())
    one = full[start[i]:start[i + 1]]
    want, want_chains = cr.chain(adj, one, [0, len(one)])
    slots, chains = run_raw(renderer, sc, one, [0, len(one)])
    assert len(one) > 20 and slots.tobytes() == want.tobytes() and (chains == want_chains).all()


def test_a_neighbour_cut_through_other_edges_ends_the_chain(renderer):
    """Status 4 needs neighbours that disagree on a shared vertex, which exact coordinates never do: the tetrahedron's cycle at z = 2
    with one record's code rewritten, so that it is entered through another edge than its neighbour leaves through."""
    sc, g = cs.scene(drt, "tetrahedron")
    rec, totals = sr.whole(g, sr.pack([(0, 0, 1)], [2]))
    adj = cr.adjacency(cs.tree_positions(sc))
    assert len(rec) == 3
    for j in range(3):
        for code in range(8):
            bent = rec.copy()
            bent["code"][j] = code
            want, want_chains = cr.chain(adj, bent, [0, 3]) if code & 3 != 3 else (None, None)
            slots, chains = run_raw(renderer, sc, bent, [0, 3])
            if want is None:                                                   # no apex 3: the record is read as a miss record
                assert (slots["flags"][slots["seg"] == j] >> 1 == cr.MISS).all()
            else:
                assert slots.tobytes() == want.tobytes() and (chains == want_chains).all(), (j, code)
    bent = rec.copy()
    bent["code"][0] ^= 3
    assert ((cr.chain(adj, bent, [0, 3])[0]["flags"] >> 1) == cr.OTHER_EDGES).any()


def test_unsorted_input_completes_inside_its_ranges(renderer):
    sc, g, planes, rec, totals, adj, _, _ = reference("cornell_box")
    splits = csr(totals)
    rng = np.random.default_rng(9)
    mixed = rec.copy()
    for i in range(0, len(totals), 2):                                         # every other range shuffled, and a record in it repeated
        lo, hi = splits[i], splits[i + 1]
        mixed[lo:hi] = mixed[lo:hi][rng.permutation(hi - lo)]
        if hi - lo > 2:
            mixed[lo + 1] = mixed[lo]
    slots, chains = run_raw(renderer, sc, mixed, splits)
    want, want_chains = cr.chain(adj, rec, splits)
    for i in range(len(totals)):
        lo, hi = splits[i], splits[i + 1]
        mine = slots[lo:hi]
        assert ((mine["seg"] >= lo) & (mine["seg"] < hi) & (mine["first"] >= lo) & (mine["first"] < hi) & (mine["length"] <= hi - lo)).all(), i
        if i % 2:                                                              # the ranges left alone are chained as ever
            assert mine.tobytes() == want[lo:hi].tobytes() and (chains[i] == want_chains[i]).all(), i


def _load(name):
    sc = drt.Scene()
    sc.loadGLTFmodel(scene_path(name))
    st = rf.streams(sc.m_PrimitivesBuffer)
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
    b.buildIterative(sc)
    return sc, st


def test_after_a_refit_that_keeps_shared_positions_shared(renderer):
    sc, st = _load("cornell_box")
    moved = (st[0] + np.float32(0.05) * np.sin(st[0][..., [1, 2, 0]] * np.float32(7))).astype(np.float32)     # a function of the position: shared stays shared
    host, _ = _load("cornell_box")
    host.refit(moved)
    adj = cr.adjacency(cs.tree_positions(sc))
    assert (cr.adjacency(cs.tree_positions(host)) == adj).all()                # the deformation keeps the table
    g_new = nr.from_product(host)
    planes = cs.planes("cornell_box", g_new)
    rec, totals = sr.whole(g_new, planes)
    want, want_chains = cr.chain(adj, rec, csr(totals))
    r = drt.Renderer(0)
    before = r.contours(sc, planes)
    r.refit(sc, torch.from_numpy(moved).to(DEV))
    after = r.contours(sc, planes)                                              # the refitted copy's segments, the host scene's table
    assert same_lists(after, expected_lists(rec, want, want_chains)) and not same_lists(before, expected_lists(rec, want, want_chains))
    assert same_lists(renderer.contours(sc, planes), before)                    # a renderer that was not refitted


def check_areas(renderer, name):
    """ContourList.areas against the same formula on the restatement's chains (contour_ref.areas, float64, chain by chain), asserted on
    EVERY chain, by the criterion of tests/test_gpu_section.py's check_areas.  Only the order of the float64 sum differs: the terms'
    products of fp32 values are exact in float64, and two sums of the same m products in different orders differ by at most about
    m * 2^-53 * sum |products|.  With mass = 0.5 * sum |products| of the chain:
      every closed chain       |got - want| <= 1e-12 * mass: each of the two sums is within 3 m * 2^-53 of the mass, m <= 64 records
                               here, so 2 * 192 * 1.1e-16 = 4.3e-14 of the mass is owed
      where mass <= 20 |area|  |got - want| <= 1e-12 * |area|: 4.3e-14 * 20 = 8.5e-13 is owed
      mass == 0                got == 0 exactly
      an open chain            NaN
    Returns (got, want, mass, the ContourList)."""
    sc, g, planes, rec, totals, adj, slots, chains = reference(name)
    want, mass = cr.areas(planes, rec, slots, chains, csr(totals))
    lst = renderer.contours(sc, planes)
    got = lst.areas()
    assert got.dtype == np.float64 and got.shape == want.shape == (len(lst.closed),)
    lengths = np.diff(lst.chain_splits)
    assert lengths.max() <= 64
    closed = lst.closed
    assert np.isnan(got[~closed]).all() and np.isnan(want[~closed]).all() and np.isfinite(got[closed]).all()
    diff = np.abs(got - want)
    some, owed = closed & (mass > 0), closed & (mass > 0) & (mass <= 20 * np.abs(want))
    print("%s: %d chains, %d closed, %d well conditioned; largest |got - want| / |area| there %.3e, largest |got - want| / mass %.3e"
          % (name, len(got), closed.sum(), owed.sum(), (diff[owed] / np.abs(want)[owed]).max(initial=0), (diff[some] / mass[some]).max(initial=0)))
    assert (diff[some] <= 1e-12 * mass[some]).all(), name
    assert (diff[owed] <= 1e-12 * np.abs(want)[owed]).all(), name
    assert (got[closed & ~(mass > 0)] == 0).all(), name
    return got, want, mass, lst


def test_chain_areas_equal_the_restatement_s_and_sum_to_the_section_areas(renderer):
    for name in ("tetrahedron", "cube", "two_cubes", "hollow_box", "cornell_box"):
        got, want, mass, lst = check_areas(renderer, name)
        sc, g, planes = reference(name)[:3]
        # from device tensors, and with the normals given: the same values
        dev = renderer.contours(sc, torch.from_numpy(planes).to(DEV))
        a = dev.areas()
        assert a.device == torch.device(DEV) and a.dtype == torch.float64 and np.array_equal(a.cpu().numpy(), got, equal_nan=True)
        assert np.array_equal(renderer.chainSections(sc, renderer.planeSections(sc, planes)).areas(planes), got, equal_nan=True)
        if name in cs.EXACT_CLOSED:
            # every chain closed: the chain areas of a plane sum to its section area, each sum within 1e-12 of the plane's mass
            assert lst.closed.all()
            whole = renderer.sectionAreas(sc, planes)
            for i in range(len(planes)):
                mine = slice(lst.splits[i], lst.splits[i + 1])
                assert abs(got[mine].sum() - whole[i]) <= 1e-12 * mass[mine].sum(), (name, i)
    # the hand cases: the tetrahedron at z = 2 encloses 2; the hollow box at z = 0 an outer 16 and a hole of 4
    sc, g, planes = reference("tetrahedron")[:3]
    assert renderer.contours(sc, planes[:1]).areas().tolist() == [2.0]
    sc, g, planes = reference("hollow_box")[:3]
    lst = renderer.contours(sc, planes[:1])
    assert lst.splits.tolist() == [0, 2] and lst.closed.all() and sorted(lst.areas().tolist()) == [-4.0, 16.0]
    assert renderer.sectionAreas(sc, planes[:1]).tolist() == [12.0]
    with pytest.raises(drt.DrtError):
        renderer.chainSections(sc, renderer.planeSections(sc, planes)).areas()          # no normals to go by
    with pytest.raises(drt.DrtError):
        lst.areas(planes[:3])                                                           # three normals for one plane


def test_queries_leave_the_renderer_alone(renderer):
    sc, g, planes, rec, totals, adj, want, want_chains = reference("cornell_box")
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
            assert same_lists(r.contours(sc, planes), expected_lists(rec, want, want_chains))
            assert r.kernelInfo() == info and r.getSampleCount() == n and r.kernelSpanMs() == span
            assert bytes(r.getCounters()) == counters
            assert r.GetRenderTargetImage().tobytes() == frame.tobytes() and r.GetAccumulationBuffer().tobytes() == accum.tobytes()
        r.Render(cam, sc)
        images.append((r.GetRenderTargetImage(), r.getSampleCount()))
    assert images[0][0].tobytes() == images[1][0].tobytes() and images[0][1] == images[1][1]


def test_an_empty_scene_chains_nothing(renderer):
    sc = drt.Scene()
    sc.addMaterial(*cs.ONE_MATERIAL[0])
    sc.setGeometry(np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 2), np.float32), np.zeros(0, np.int32))
    drt.BVHBuilder().buildIterative(sc)
    planes = sr.pack(np.eye(3, dtype=np.float32), [0, 1, 2])
    got = renderer.contours(sc, planes)
    assert got.splits.tolist() == [0, 0, 0, 0] and got.chain_splits.tolist() == [0] and len(got.closed) == 0 and got.p.shape == (0, 3)
    assert got.areas().shape == (0,)
    # miss records only: each stays where it is
    slots, chains = run_raw(renderer, sc, np.repeat(sr.MISS, 6), [0, 2, 4, 6])
    assert [tuple(int(x) for x in s) for s in slots] == [(j, j, 1, cr.MISS << 1) for j in range(6)] and not chains.any()
    # records of another scene's triangles: none of them is a triangle of this one
    rec = reference("tetrahedron")[3]
    slots, chains = run_raw(renderer, sc, rec, [0, len(rec)])
    assert ((slots["flags"] >> 1) == cr.MISS).all() and not chains.any()


def test_error_paths(renderer):
    sc, g, planes, rec, totals, adj, want, want_chains = reference("cornell_box")
    dev = torch.device(DEV)
    n, total = len(totals), len(rec)
    segs = torch.from_numpy(np.concatenate([rec, rec[:4]]).view(np.int32).reshape(-1, 8)).to(dev)
    splits = torch.from_numpy(np.concatenate([csr(totals), [total]]).astype(np.int32)).to(dev)
    slots = torch.full((total + 4, 4), SENTINEL, dtype=torch.int32, device=dev)
    chains = torch.full((n + 1, 2), -1, dtype=torch.int32, device=dev)
    host = np.zeros((total + 4, 8), np.int32)
    L, h = drt._lib, renderer._h
    INV = drt.ERR_INVALID
    S, P, O, C, H = segs.data_ptr(), splits.data_ptr(), slots.data_ptr(), chains.data_ptr(), host.ctypes.data
    for what, args in (("null segs", (h, sc._h, None, P, O, C, n, total)), ("null splits", (h, sc._h, S, None, O, C, n, total)),
                       ("null slots", (h, sc._h, S, P, None, C, n, total)), ("null renderer", (None, sc._h, S, P, O, C, n, total)),
                       ("null scene", (h, None, S, P, O, C, n, total)), ("null handles, n = 0", (None, None, S, P, O, C, 0, 0)),
                       ("misaligned segs", (h, sc._h, S + 4, P, O, C, n, total)), ("misaligned slots", (h, sc._h, S, P, O + 8, C, n, total)),
                       ("misaligned splits", (h, sc._h, S, P + 2, O, C, n, total)), ("misaligned chains", (h, sc._h, S, P, O, C + 1, n, total)),
                       ("2^31 planes", (h, sc._h, S, P, O, C, 2 ** 31, total)), ("2^31 records", (h, sc._h, S, P, O, C, n, 2 ** 31)),
                       ("host segs", (h, sc._h, H, P, O, C, n, total)), ("host splits", (h, sc._h, S, H, O, C, n, total)),
                       ("host slots", (h, sc._h, S, P, H, C, n, total)), ("host chains", (h, sc._h, S, P, O, H, n, total))):
        assert L.drt_renderer_chain_sections(*args, None) == INV, what
    for args in ((h, sc._h, None, None, None, None, 0, 0), (h, sc._h, S, P, O, C, 0, total), (h, sc._h, S, P, O, C, n, 0)):
        assert L.drt_renderer_chain_sections(*args, None) == drt.OK                # n == 0 or total == 0: nothing to do
    torch.cuda.synchronize()
    assert (slots == SENTINEL).all() and (chains == -1).all()                      # nothing was launched
    # segs and slots need 16-byte alignment, the rest 4: half a record, one slot and one word further on
    assert L.drt_renderer_chain_sections(h, sc._h, S, P + 4, O + 16, C + 4, n, total, None) == drt.OK
    torch.cuda.synchronize()
    assert (slots[0] == SENTINEL).all() and (chains.reshape(-1)[0] == -1).all()
    shifted = np.concatenate([csr(totals)[1:], [total]])
    want2, want2_chains = cr.chain(adj, rec, shifted)
    got = slots[1:1 + total].cpu().numpy().view(cr.SLOT).reshape(-1)
    inside = slice(int(shifted[0]), total)
    assert got[inside].tobytes() == want2[inside].tobytes() and (got[:inside.start].view(np.int32) == SENTINEL).all()
    assert (chains.reshape(-1)[1:1 + 2 * n].cpu().numpy().view(np.uint32) == want2_chains.reshape(-1)).all()
    for bad in (lambda: renderer.chainSections(sc, None), lambda: renderer.chainSections(sc, (1, 2, 3, 4, 5)),
                lambda: renderer.chainSections(sc, drt.SectionList(*[torch.zeros(1)] * 5)),                         # wrong device and dtype
                lambda: renderer.chainSections(sc, renderer.planeSections(sc, planes)._replace(prim=np.zeros(total, np.int64))),
                lambda: renderer.chainSections(sc, renderer.planeSections(sc, planes)._replace(code=np.zeros(3, np.int32))),
                lambda: renderer.contours(sc, planes.astype(np.float64)), lambda: renderer.contours(sc, planes[:, :3])):
        with pytest.raises(drt.DrtError) as e:
            bad()
        assert e.value.code == INV
    empty = renderer.contours(sc, np.zeros((0, 4), np.float32))
    assert empty.splits.tolist() == [0] and empty.chain_splits.tolist() == [0] and len(empty.prim) == 0 and empty.areas().shape == (0,)
    # a pending asynchronous batch
    r = drt.Renderer(0)
    r.ResizeBuffer(64, 32)
    r.RenderBatchAsync(drt.Camera(SCENES["cornell_box"][1]), sc, 1)
    with pytest.raises(drt.DrtError) as e:
        r.chainSections(sc, drt.SectionList(*(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (csr(totals).astype(np.int32), rec["p"], rec["q"], rec["prim"], rec["code"]))))
    assert e.value.code == INV
    assert raw(r, sc, segs, splits, slots, chains, n, total) == INV
    r.Wait()
    assert same_lists(r.contours(sc, planes), expected_lists(rec, want, want_chains))
    # a tree deeper than 64 levels: the scene's upload refuses it
    chain = list(rq.degenerate_chain(110))
    chain[0] = (chain[0] * np.float32(2.0 ** -55)).astype(np.float32)
    deep, _ = rq.programmatic_scene(drt, *chain, 1, 2)
    assert deep.bvh_depth > 64
    assert raw(renderer, deep, segs, splits, slots, chains, n, total) == drt.ERR_UNSUPPORTED
    assert same_lists(renderer.contours(sc, planes), expected_lists(rec, want, want_chains))               # after the errors
