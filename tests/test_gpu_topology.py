"""Mesh topology on the GPU (drt_renderer_shell_labels, drt_renderer_boundary_loops, drt_renderer_shell_terms, kernel_topology.hip;
Renderer.shells / boundaryLoops / shellTerms / shellMeasures): every label, count, slot and loop count bit-equal to the union-find and
the sequential walk of tests/topology_ref.py, and every term record bit-equal to the numpy expression on the device's own records --
over the meshes of tests/topology_scenes.py (the strip and the band need several labelling rounds and 13 jumping rounds), cornell_box,
the soup and the degenerate mesh; counting with NULL slots; a truncating capacity; the second call, served from the cache; a device
refit; a new upload; an empty scene; the error codes; the Python lists in numpy and torch; area, volume and area vector.
tests/test_topology_ref.py asserts what the restatement does."""
import numpy as np
import pytest

from tests import contour_ref as cr
from tests import contour_scenes as cs
from tests import ray_query_ref as rq
from tests import refit_ref as rf
from tests import topology_ref as tr
from tests import topology_scenes as ts
from tests.scenes import SCENES, scene_path

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -77
PAD = 4
_ref = {}


@pytest.fixture(scope="module")
def renderer():
    return drt.Renderer(0)


def restate(sc):
    """(adjacency, labels, counts, slots, loop counts) of a scene, by the restatements."""
    adj = cr.adjacency(ts.tree_positions(sc))
    label = tr.labels(adj)
    slots, loop_counts = tr.loops(adj)
    return adj, label, tr.counts(adj, label), slots, loop_counts


def reference(name):
    """(scene, adjacency, labels, counts, slots, loop counts) of a named scene, computed once."""
    if name not in _ref:
        sc = ts.scene(drt, name)
        _ref[name] = (sc,) + restate(sc)
    return _ref[name]


def run_labels(r, sc, n, with_counts=True):
    """drt_renderer_shell_labels on sentinel-filled buffers: (labels [n], counts [3] or None) as host arrays; the padding stays."""
    labels = torch.full((n + PAD,), SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.full((3 + PAD,), SENTINEL, dtype=torch.int32, device=DEV) if with_counts else None
    assert drt._lib.drt_renderer_shell_labels(r._h, sc._h, labels.data_ptr(), counts.data_ptr() if with_counts else None, None) == drt.OK
    torch.cuda.synchronize()
    assert (labels[n:] == SENTINEL).all() and (counts is None or (counts[3:] == SENTINEL).all())
    return labels[:n].cpu().numpy(), (None if counts is None else counts[:3].cpu().numpy().view(np.uint32))


def run_loops(r, sc, capacity):
    """drt_renderer_boundary_loops with `capacity` slots (None: slots NULL, a pure count) in front of sentinels: (slots as SLOT over
    the capacity, counts [3])."""
    counts = torch.full((3 + PAD,), SENTINEL, dtype=torch.int32, device=DEV)
    slots = None if capacity is None else torch.full((capacity + PAD, 4), SENTINEL, dtype=torch.int32, device=DEV)
    rc = drt._lib.drt_renderer_boundary_loops(r._h, sc._h, None if slots is None else slots.data_ptr(), capacity or 0, counts.data_ptr(), None)
    assert rc == drt.OK
    torch.cuda.synchronize()
    assert (counts[3:] == SENTINEL).all() and (slots is None or (slots[capacity:] == SENTINEL).all())
    got = np.zeros(0, tr.SLOT) if slots is None else slots[:capacity].cpu().numpy().view(tr.SLOT).reshape(-1)
    return got, counts[:3].cpu().numpy().view(np.uint32)


def device_terms(r, sc):
    """(the term records the product wrote, the numpy expression on the records the device holds) as TERM arrays."""
    got = r.shellTerms(sc)
    assert got.dtype == torch.float64 and got.device == torch.device(DEV)
    hot = r.debugReadDeviceScene(sc)[1]
    return got.cpu().numpy().view(tr.TERM).reshape(-1), tr.terms(*tr.hot_words(hot))


def expected_shells(adj, label):
    index, tri, open_edges, bad_edges, watertight = tr.per_shell(adj, label)
    return (label, index, len(tri), tri, open_edges, bad_edges, watertight)


def expected_loops(slots, index):
    first = np.nonzero(slots["first"] == np.arange(len(slots)))[0]
    h = slots["half_edge"].astype(np.int32)
    return (np.concatenate([first, [len(slots)]]).astype(np.int32), (slots["flags"][first] & 1).astype(bool), h, h // 3, h % 3,
            index[h[first] // 3].astype(np.int32), (slots["flags"] >> 1).astype(np.int32))


def same(got, want):
    for a, b in zip(got, want):
        if isinstance(b, int):
            if a != b:
                return False
            continue
        a = a.cpu().numpy() if torch.is_tensor(a) else a
        if a.dtype != b.dtype or a.shape != b.shape or a.tobytes() != b.tobytes():
            return False
    return True


def check_measures(name, got, term, index, n_shells):
    """Renderer.shellMeasures against the same sums of the same term records by math.fsum (tests/topology_ref.py: exact, rounded once),
    by the criterion of tests/test_gpu_section.py's check_areas, per shell and per component, with mass = the sum of the absolute terms:
      everywhere               |got - want| <= 1e-12 * mass
      where mass <= 20 |want|  |got - want| <= 1e-12 * |want|
      mass == 0                got == 0 exactly
    What is owed: the terms are the same bits (the square root of the areas is the correctly rounded one on both sides, or one ulp
    apart: 2.2e-16 of the mass), the reference is exact, and the product's running sum carries its rounding errors along, so a shell's
    sum is a few roundings of its own size off, 1e-15 of the mass, plus second-order terms of the sums in front of it."""
    area, volume, vector, m_area, m_volume, m_vector = tr.measures(term, index, n_shells)
    assert all(x.dtype == np.float64 for x in got) and got.area.shape == (n_shells,) and got.volume.shape == (n_shells,) and got.area_vector.shape == (n_shells, 3)
    for what, g, w, m in (("area", got.area, area, m_area), ("volume", got.volume, volume, m_volume), ("area_vector", got.area_vector, vector, m_vector)):
        diff = np.abs(g - w)
        some, owed = m > 0, (m > 0) & (m <= 20 * np.abs(w))
        print("%s %s: largest |got - want| / mass %.3e, / |want| where well conditioned %.3e (%d of %d)"
              % (name, what, (diff[some] / m[some]).max(initial=0), (diff[owed] / np.abs(w)[owed]).max(initial=0), owed.sum(), owed.size))
        assert (diff[some] <= 1e-12 * m[some]).all(), (name, what)
        assert (diff[owed] <= 1e-12 * np.abs(w)[owed]).all(), (name, what)
        assert (g[~some] == 0).all(), (name, what)
    return area, volume, vector


@pytest.mark.parametrize("name", ts.ALL_NAMES)
def test_every_label_count_slot_and_term_is_bit_equal_to_the_restatement(renderer, name):
    sc, adj, label, counts, want, want_counts = reference(name)
    n, m = len(label), len(want)
    print("%s: %d triangles, %s shells / open / bad, %s records / loops / closed" % (name, n, counts.tolist(), want_counts.tolist()))
    assert (sc.edgeAdjacency().reshape(-1) == adj).all()
    got, got_counts = run_labels(renderer, sc, n)
    assert got.tobytes() == label.tobytes() and (got_counts == counts).all(), name
    steps = renderer.topologySteps()
    print("%s: labelling steps enqueued, busy, hooks: %s" % (name, steps))
    assert steps[0] >= steps[1] >= steps[2] >= 1 and steps[0] > steps[1]
    # the second call is served from the cache; counts NULL
    again, none = run_labels(renderer, sc, n, with_counts=False)
    assert none is None and again.tobytes() == label.tobytes() and renderer.topologySteps() == steps
    # the loops: a pure count, then the slots, twice
    nothing, only_counts = run_loops(renderer, sc, None)
    assert len(nothing) == 0 and (only_counts == want_counts).all(), name
    if m:
        for _ in range(2):
            slots, loop_counts = run_loops(renderer, sc, m)
            assert slots.tobytes() == want.tobytes() and (loop_counts == want_counts).all(), name
    # the terms: the expression on the records the device holds
    term, want_term = device_terms(renderer, sc)
    assert term.tobytes() == want_term.tobytes(), name
    # the Python lists, numpy and torch
    shells = expected_shells(adj, label)
    for as_torch in (False, True):
        sh = renderer.shells(sc, as_torch=as_torch)
        assert isinstance(sh, drt.Shells) and isinstance(sh.count, int) and same(sh, shells), name
        assert all((torch.is_tensor(x) and x.device == torch.device(DEV)) if as_torch else isinstance(x, np.ndarray) for x in sh if not isinstance(x, int))
        loops = renderer.boundaryLoops(sc, as_torch=as_torch)
        assert isinstance(loops, drt.LoopList) and same(loops, expected_loops(want, shells[1])), name
        ms = renderer.shellMeasures(sc, as_torch=as_torch)
        assert isinstance(ms, drt.ShellMeasures) and all(torch.is_tensor(x) == as_torch for x in ms)
        if as_torch:
            assert all(x.dtype == torch.float64 and x.device == torch.device(DEV) for x in ms)
            ms = drt.ShellMeasures(*(x.cpu().numpy() for x in ms))
        check_measures(name, ms, want_term, shells[1], shells[2])
    if name in ("ring", "strip"):
        assert shells[2] == 1 and steps[2] >= 2                                   # one shell, and more than one round of hooks
    if name == "ring":
        assert want_counts.tolist() == [2 * cs.RING_QUADS, 2, 2]
    if name == "strip":
        assert want_counts.tolist() == [2 * ts.STRIP_QUADS + 2, 1, 1]
    if name in ("book", "flipped_quad", "degenerate"):
        assert ((want["flags"] >> 1) == cr.NON_MANIFOLD).any() and want_counts[2] < want_counts[1]
    if name in ("soup", "degenerate", "cornell_box"):
        assert counts[0] > 1 and m > 0


def test_the_hand_values_are_exact(renderer):
    ms = renderer.shellMeasures(ts.scene(drt, "tetrahedron"))
    assert ms.volume.tolist() == [64.0 / 6.0] and ms.area_vector.tolist() == [[0.0, 0.0, 0.0]]
    assert abs(ms.area[0] - 0.5 * (48.0 + np.sqrt(768.0))) <= 1e-12 * ms.area[0]
    sc = ts.scene(drt, "two_cubes")                                              # boxes of 1 x 1 x 1 and 1 x 1 x 1.5; tree order may swap them
    sh, ms = renderer.shells(sc), renderer.shellMeasures(sc)
    assert sh.count == 2 and sh.triangles.tolist() == [12, 12] and sh.watertight.all()
    assert sorted(ms.volume.tolist()) == [1.0, 1.5] and sorted(ms.area.tolist()) == [6.0, 8.0] and not ms.area_vector.any()
    sc = ts.scene(drt, "hollow_box")                                             # sides 4 and 2, the inner one inward
    pos = ts.tree_positions(sc)
    sides = sorted({float(np.ptp(pos[sh_tris].reshape(-1, 3)[:, 0])) for sh_tris in (renderer.shells(sc).index == 0, renderer.shells(sc).index == 1)})
    ms = renderer.shellMeasures(sc)
    assert sides == [2.0, 4.0] and sorted(ms.volume.tolist()) == [-sides[0] ** 3, sides[1] ** 3] == [-8.0, 64.0]
    assert sorted(ms.area.tolist()) == [24.0, 96.0] and not ms.area_vector.any() and renderer.shells(sc).watertight.all()
    loops = renderer.boundaryLoops(sc)
    assert loops.splits.tolist() == [0] and len(loops.half_edge) == 0 and len(loops.closed) == 0


@pytest.mark.parametrize("name", ["quad", "two_fans", "ring", "cornell_box"])
def test_a_small_capacity_truncates_between_sentinels(renderer, name):
    sc, adj, label, counts, want, want_counts = reference(name)
    m = len(want)
    for capacity in sorted({1, m // 2, m - 1, m + 3}):
        slots, loop_counts = run_loops(renderer, sc, capacity)                    # (run_loops checks the sentinels behind the capacity)
        kept = min(capacity, m)
        assert slots[:kept].tobytes() == want[:kept].tobytes() and (loop_counts == want_counts).all(), (name, capacity)
        assert (slots[kept:].view(np.int32) == SENTINEL).all(), (name, capacity)


def _load(name):
    sc = drt.Scene()
    sc.loadGLTFmodel(scene_path(name))
    st = rf.streams(sc.m_PrimitivesBuffer)
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
    b.buildIterative(sc)
    return sc, st


def test_a_device_refit_keeps_labels_and_loops_and_moves_the_terms():
    sc, st = _load("cornell_box")
    moved = (st[0] + np.float32(0.05) * np.sin(st[0][..., [1, 2, 0]] * np.float32(7))).astype(np.float32)     # a function of the position: shared stays shared
    host, _ = _load("cornell_box")
    host.refit(moved)
    adj, label, counts, want, want_counts = restate(sc)
    assert (cr.adjacency(ts.tree_positions(host)) == adj).all()                # the deformation keeps the table
    r = drt.Renderer(0)
    n, m = len(label), len(want)
    before, want_before = device_terms(r, sc)
    assert before.tobytes() == want_before.tobytes()
    assert run_labels(r, sc, n)[0].tobytes() == label.tobytes()
    steps = r.topologySteps()
    measures_before = r.shellMeasures(sc)
    r.refit(sc, torch.from_numpy(moved).to(DEV))
    got, got_counts = run_labels(r, sc, n)
    slots, loop_counts = run_loops(r, sc, m)
    assert got.tobytes() == label.tobytes() and (got_counts == counts).all() and slots.tobytes() == want.tobytes() and (loop_counts == want_counts).all()
    assert r.topologySteps() == steps                                            # nothing was labelled again
    after, want_after = device_terms(r, sc)                                      # the refitted records, read back from the device
    assert after.tobytes() == want_after.tobytes() and after.tobytes() != before.tobytes()
    host_terms = tr.terms(*tr.hot_words(host.debugPack()[1]))
    assert after.tobytes() == host_terms.tobytes()                               # ... which are the host refit's
    index, tri = tr.per_shell(adj, label)[:2]
    area, volume, vector = check_measures("refitted cornell_box", r.shellMeasures(sc), want_after, index, len(tri))
    assert not np.array_equal(r.shellMeasures(sc).area, measures_before.area)


def test_a_new_upload_drops_the_cache(renderer):
    a, b = reference("two_cubes"), reference("book")
    for sc, adj, label, counts, want, want_counts in (a, b, a):
        got, got_counts = run_labels(renderer, sc, len(label))
        assert got.tobytes() == label.tobytes() and (got_counts == counts).all()
        assert (run_loops(renderer, sc, None)[1] == want_counts).all()
    # the same scene, changed on the host: its two triangles pulled apart
    sc = cs.flat_scene(drt, cs.QUAD, leaf=4)[0]
    assert renderer.shells(sc).count == 1 and renderer.boundaryLoops(sc).splits.tolist() == [0, 4]
    apart = cs.QUAD.copy()
    apart[1] += np.float32([0, 0, 1])
    sc.refit(apart)
    adj, label, counts, want, want_counts = restate(sc)
    assert counts.tolist() == [2, 6, 0]
    sh = renderer.shells(sc)
    assert sh.count == 2 and sh.label.tobytes() == label.tobytes() and sh.open_edges.tolist() == [3, 3]
    assert same(renderer.boundaryLoops(sc), expected_loops(want, sh.index))
    term, want_term = device_terms(renderer, sc)
    assert term.tobytes() == want_term.tobytes()


def test_an_empty_scene_has_no_shells(renderer):
    sc = ts.empty_scene(drt)
    labels, counts = run_labels(renderer, sc, 0)
    assert len(labels) == 0 and counts.tolist() == [0, 0, 0]
    assert run_loops(renderer, sc, None)[1].tolist() == [0, 0, 0]
    slots, loop_counts = run_loops(renderer, sc, 5)
    assert (slots.view(np.int32) == SENTINEL).all() and loop_counts.tolist() == [0, 0, 0]
    sh = renderer.shells(sc)
    assert sh.count == 0 and sh.label.shape == (0,) and sh.index.shape == (0,) and sh.triangles.shape == (0,) and sh.watertight.shape == (0,)
    loops = renderer.boundaryLoops(sc)
    assert loops.splits.tolist() == [0] and all(len(x) == 0 for x in loops[1:])
    ms = renderer.shellMeasures(sc)
    assert ms.area.shape == (0,) and ms.volume.shape == (0,) and ms.area_vector.shape == (0, 3)
    assert renderer.shellTerms(sc).shape == (0, 4)


def test_queries_leave_the_renderer_alone():
    sc, adj, label, counts, want, want_counts = reference("cornell_box")
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
            assert r.shells(sc).label.tobytes() == label.tobytes() and len(r.boundaryLoops(sc).half_edge) == len(want)
            assert r.shellMeasures(sc).area.shape == (int(counts[0]),)
            assert r.kernelInfo() == info and r.getSampleCount() == n and r.kernelSpanMs() == span
            assert bytes(r.getCounters()) == counters
            assert r.GetRenderTargetImage().tobytes() == frame.tobytes() and r.GetAccumulationBuffer().tobytes() == accum.tobytes()
        r.Render(cam, sc)
        images.append((r.GetRenderTargetImage(), r.getSampleCount()))
    assert images[0][0].tobytes() == images[1][0].tobytes() and images[0][1] == images[1][1]


def test_error_paths(renderer):
    sc, adj, label, counts, want, want_counts = reference("cornell_box")
    n, m = len(label), len(want)
    L, h, INV = drt._lib, renderer._h, drt.ERR_INVALID
    labels = torch.full((n + PAD,), SENTINEL, dtype=torch.int32, device=DEV)
    cnt = torch.full((8,), SENTINEL, dtype=torch.int32, device=DEV)
    slots = torch.full((m + PAD, 4), SENTINEL, dtype=torch.int32, device=DEV)
    terms = torch.full((n + 1, 4), -1.0, dtype=torch.float64, device=DEV)
    host = np.zeros((4 * n + 64,), np.float64)
    A, C, S, T, H = labels.data_ptr(), cnt.data_ptr(), slots.data_ptr(), terms.data_ptr(), (host.ctypes.data + 15) & ~15
    for what, call in (("null renderer", lambda: L.drt_renderer_shell_labels(None, sc._h, A, C, None)),
                       ("null scene", lambda: L.drt_renderer_shell_labels(h, None, A, C, None)),
                       ("null labels", lambda: L.drt_renderer_shell_labels(h, sc._h, None, C, None)),
                       ("misaligned labels", lambda: L.drt_renderer_shell_labels(h, sc._h, A + 2, C, None)),
                       ("misaligned counts", lambda: L.drt_renderer_shell_labels(h, sc._h, A, C + 1, None)),
                       ("host labels", lambda: L.drt_renderer_shell_labels(h, sc._h, H, C, None)),
                       ("host counts", lambda: L.drt_renderer_shell_labels(h, sc._h, A, H, None)),
                       ("null loop counts", lambda: L.drt_renderer_boundary_loops(h, sc._h, S, m, None, None)),
                       ("slots without a capacity", lambda: L.drt_renderer_boundary_loops(h, sc._h, S, 0, C, None)),
                       ("a capacity without slots", lambda: L.drt_renderer_boundary_loops(h, sc._h, None, m, C, None)),
                       ("misaligned slots", lambda: L.drt_renderer_boundary_loops(h, sc._h, S + 8, m, C, None)),
                       ("2^31 slots", lambda: L.drt_renderer_boundary_loops(h, sc._h, S, 2 ** 31, C, None)),
                       ("host slots", lambda: L.drt_renderer_boundary_loops(h, sc._h, H, m, C, None)),
                       ("host loop counts", lambda: L.drt_renderer_boundary_loops(h, sc._h, S, m, H, None)),
                       ("null terms", lambda: L.drt_renderer_shell_terms(h, sc._h, None, None)),
                       ("misaligned terms", lambda: L.drt_renderer_shell_terms(h, sc._h, T + 8, None)),
                       ("host terms", lambda: L.drt_renderer_shell_terms(h, sc._h, H, None)),
                       ("host table", lambda: L.drt_renderer_edge_adjacency(h, sc._h, H, None))):
        assert call() == INV, what
    torch.cuda.synchronize()
    assert (labels == SENTINEL).all() and (cnt == SENTINEL).all() and (slots == SENTINEL).all() and (terms == -1.0).all()       # nothing was launched
    # slots and terms need 16-byte alignment, the rest 4: one slot, one word and half a record further on
    assert L.drt_renderer_shell_labels(h, sc._h, A + 4, C + 4, None) == drt.OK
    assert L.drt_renderer_boundary_loops(h, sc._h, S + 16, m, C + 16, None) == drt.OK
    assert L.drt_renderer_shell_terms(h, sc._h, T + 16, None) == drt.OK
    torch.cuda.synchronize()
    assert labels[1:1 + n].cpu().numpy().tobytes() == label.tobytes() and labels[0] == SENTINEL and (labels[1 + n:] == SENTINEL).all()
    assert (cnt[1:4].cpu().numpy().view(np.uint32) == counts).all() and (cnt[4:7].cpu().numpy().view(np.uint32) == want_counts).all() and cnt[7] == SENTINEL
    assert slots[1:1 + m].cpu().numpy().view(tr.SLOT).reshape(-1).tobytes() == want.tobytes() and (slots[0] == SENTINEL).all() and (slots[1 + m:] == SENTINEL).all()
    got_terms = terms.reshape(-1)[2:2 + 4 * n].cpu().numpy()
    assert got_terms.tobytes() == device_terms(renderer, sc)[1].tobytes() and (terms.reshape(-1)[:2] == -1.0).all() and (terms.reshape(-1)[2 + 4 * n:] == -1.0).all()
    # a scene without a BVH: the table is in tree order
    flat = drt.Scene()
    flat.addMaterial(*cs.ONE_MATERIAL[0])
    k = len(cs.QUAD)
    flat.setGeometry(cs.QUAD, np.zeros((k, 3, 3), np.float32), np.zeros((k, 3, 2), np.float32), np.zeros(k, np.int32))
    assert L.drt_renderer_shell_labels(h, flat._h, A, C, None) == INV and b"BVH" in L.drt_last_error()
    assert L.drt_renderer_boundary_loops(h, flat._h, S, m, C, None) == INV and L.drt_renderer_shell_terms(h, flat._h, T, None) == INV
    with pytest.raises(drt.DrtError) as e:
        renderer.shells(flat)
    assert e.value.code == INV
    # a pending asynchronous batch
    r = drt.Renderer(0)
    r.ResizeBuffer(64, 32)
    r.RenderBatchAsync(drt.Camera(SCENES["cornell_box"][1]), sc, 1)
    for bad in (lambda: r.shells(sc), lambda: r.boundaryLoops(sc), lambda: r.shellMeasures(sc), lambda: r.shellTerms(sc)):
        with pytest.raises(drt.DrtError) as e:
            bad()
        assert e.value.code == INV and "pending" in str(e.value)
    r.Wait()
    assert r.shells(sc).label.tobytes() == label.tobytes()
    # a tree deeper than 64 levels: the scene's upload refuses it
    chain = list(rq.degenerate_chain(110))
    chain[0] = (chain[0] * np.float32(2.0 ** -55)).astype(np.float32)
    deep, _ = rq.programmatic_scene(drt, *chain, 1, 2)
    assert deep.bvh_depth > 64
    assert L.drt_renderer_shell_labels(h, deep._h, A, C, None) == drt.ERR_UNSUPPORTED
    assert L.drt_renderer_boundary_loops(h, deep._h, S, m, C, None) == drt.ERR_UNSUPPORTED
    assert L.drt_renderer_shell_terms(h, deep._h, T, None) == drt.ERR_UNSUPPORTED
    assert renderer.shells(sc).label.tobytes() == label.tobytes()                # after the errors
