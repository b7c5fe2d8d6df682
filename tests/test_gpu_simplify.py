"""Mesh simplification on the device (drt_renderer_simplify, kernel_simplify.hip) against tests/simplify_ref.py, bit for bit, cluster
and counts included: vertex and triangle counts around a wave, a workgroup and the scans' trips; every vertex in one cell and every
vertex in its own; a lattice soup; grids of one cell and of nearly 2^31; vertices outside the grid and not finite, indices out of range;
meshes of every size; both placements; every capacity with sentinels behind it; numpy, tensors, a side stream and two runs; and a
damaged torus remeshed, welded, simplified and rendered with its vertex normals."""
import numpy as np
import pytest

from tests import inside_ref as ir
from tests import ray_query_ref as rq
from tests import simplify_ref as sr
from tests import weld_ref as wd

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

F = np.float32
DEV = "cuda:0"
PLACEMENTS = ["mean", "quadric"]
SEAMS = [1, 63, 64, 65, 255, 256, 257, 65535, 65536, 65537]      # a wave, a workgroup of the scan, one trip of the offsets launch


@pytest.fixture(scope="module")
def renderer():
    return drt.Renderer(0)


def box(lo, hi, res):
    """(lo, cell, dims) as the wrapper makes them from an explicit box: cell = (hi - lo) / res in float32"""
    lo, hi = np.asarray(lo, F).reshape(3), np.asarray(hi, F).reshape(3)
    dims = np.asarray(res, np.int64) * np.ones(3, np.int64)
    return lo, ((hi - lo) / dims.astype(F)).astype(F), dims


def same(got, want, what):
    g = [x.cpu().numpy() if torch.is_tensor(x) else x for x in got]
    assert [x.dtype for x in g] == [np.float32, np.int32, np.int32, np.int32, np.int32], what
    assert (len(g[0]), len(g[1])) == want.counts and g[0].shape[1:] == (3,) and g[1].shape[1:] == (3,), (what, len(g[0]), len(g[1]), want.counts)
    assert g[3].tolist() == want.cluster.tolist(), what
    assert g[2].tolist() == want.first.tolist(), what
    assert g[1].tolist() == want.faces.tolist(), what
    assert g[4].tolist() == want.source.tolist(), what
    if g[0].tobytes() != want.vertices.tobytes():
        bad = np.nonzero((g[0].view(np.uint32) != want.vertices.view(np.uint32)).any(axis=1))[0]
        raise AssertionError("%s: %d of %d positions differ, first at cluster %d: %r against %r" %
                             (what, len(bad), len(g[0]), bad[0], g[0][bad[0]].tolist(), want.vertices[bad[0]].tolist()))


def against_the_restatement(renderer, v, f, lo, hi, res, placement, what):
    got = renderer.simplify((v, f), resolution=res, lo=lo, hi=hi, placement=placement)
    want = sr.simplify(v, f, *box(lo, hi, res), drt.SIMPLIFY_PLACEMENTS[placement])
    same(got, want, what)
    return got, want


def cloud(nv, nt, seed):
    """nv random vertices of the unit cube and nt random triangles of them"""
    rng = np.random.default_rng(seed)
    return rng.random((nv, 3)).astype(F), rng.integers(0, nv, (nt, 3)).astype(np.int32)


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("n", SEAMS)
def test_vertex_counts_around_every_seam(renderer, n, placement):
    v, f = cloud(n, 2 * n + 1, n)
    res = max(1, int(round((n / 4) ** (1 / 3))))                                # about four vertices per cell
    got, want = against_the_restatement(renderer, v, f, (0, 0, 0), (1, 1, 1), res, placement, n)
    assert n == 1 or want.counts[0] < n


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("n", SEAMS)
def test_triangle_counts_around_every_seam(renderer, n, placement):
    v, f = cloud(500, n, n + 7)
    got, want = against_the_restatement(renderer, v, f, (0, 0, 0), (1, 1, 1), (5, 4, 3), placement, n)
    assert n < 63 or 0 < want.counts[1] < n


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("n", [64, 4096])
def test_every_vertex_in_one_cell(renderer, n, placement):
    v, f = cloud(n, 3 * n, n)                                                   # every atomic of the call lands on one cluster
    got, want = against_the_restatement(renderer, v, f, (-1, -1, -1), (2, 2, 2), 1, placement, n)
    assert want.counts == (1, 0) and got.first.tolist() == [0] and not got.cluster.any() and want.sums[0, 0] == n
    assert placement == "mean" or want.sums[0, 4:].all()


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_every_vertex_in_a_cell_of_its_own(renderer, placement):
    idx = np.random.default_rng(2).permutation(16 ** 3)[:3000]
    v = (np.stack([idx % 16, idx // 16 % 16, idx // 256], axis=1) + np.random.default_rng(3).random((3000, 3)) * 0.9).astype(F)
    f = np.random.default_rng(4).integers(0, 3000, (7000, 3)).astype(np.int32)
    got, want = against_the_restatement(renderer, v, f, (0, 0, 0), (16, 16, 16), 16, placement, "singletons")
    keep = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])
    assert got.vertices.tobytes() == v.tobytes() and got.faces.tobytes() == f[keep].tobytes()      # the input, byte for byte
    assert got.cluster.tolist() == list(range(3000)) and got.source.tolist() == np.nonzero(keep)[0].tolist()


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_a_lattice_soup(renderer, placement):
    soup = np.random.default_rng(3).integers(0, 12, (50_000, 3, 3)).astype(F)
    v, f, _, _ = wd.weld(soup)
    assert len(v) == 12 ** 3
    got, want = against_the_restatement(renderer, v, f, (-0.5, -0.5, -0.5), (11.5, 11.5, 11.5), 4, placement, "lattice")
    assert want.counts[0] == 64 and (want.sums[:, 0] == 27).all() and 30_000 < want.counts[1] < 50_000


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_a_grid_of_one_cell_and_a_grid_of_nearly_two_to_the_31_cells(renderer, placement):
    v, f = cloud(700, 1500, 12)
    v = v * F(1.5) - F(0.25)                                                    # a part of them outside
    got, want = against_the_restatement(renderer, v, f, (0, 0, 0), (1, 1, 1), (1, 1, 1), placement, "1x1x1")
    assert 1 < want.counts[0] < 700 and want.sums[:, 0].max() > 100
    dims = np.array([2048, 1024, 1023])
    rng = np.random.default_rng(13)
    base = (rng.random((150, 3)) * dims).astype(F)
    base[:8] = dims - rng.random((8, 3)) * 2                                    # the last cells: keys just below 2^31
    v = np.concatenate([base, base + rng.random((150, 3)).astype(F) * F(0.25), base[:50]]).astype(F)
    f = rng.integers(0, len(v), (900, 3)).astype(np.int32)
    got, want = against_the_restatement(renderer, v, f, (0, 0, 0), tuple(float(d) for d in dims), tuple(int(d) for d in dims), placement, "2^31")
    key, _ = sr.keys_of(v, *box((0, 0, 0), dims, dims))
    assert key.max() > 2 ** 31 - 2 ** 23 and 150 <= want.counts[0] < 300 and (want.sums[:, 0] > 1).sum() > 60


def hostile(seed=21):
    """vertices outside the grid on every side, NaNs and infinities, indices out of range on both sides, triangles that name a vertex
    twice and three times, triangles without area"""
    v, f = cloud(900, 2500, seed)
    v = v * F(1.4) - F(0.2)
    for row, col, value in ((5, 0, np.nan), (17, 1, np.inf), (40, 2, -np.inf), (41, 0, np.nan), (300, 1, np.nan)):
        v[row, col] = value
    v[41, 1], v[41, 2] = np.inf, -np.inf
    v[600:620] = v[100:120]                                                     # coincident vertices: triangles of no area among them
    f[3], f[50], f[51], f[700] = (900, 1, 2), (-1, 5, 6), (2 ** 31 - 1, 7, 8), (-2 ** 31, 9, 10)
    f[10, 1], f[11, 2], f[12] = f[10, 0], f[11, 1], (44, 44, 44)
    f[13], f[14] = (100, 600, 101), (5, 17, 40)
    return v, f


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_a_hostile_mesh(renderer, placement):
    v, f = hostile()
    got, want = against_the_restatement(renderer, v, f, (0, 0, 0), (1, 1, 1), 5, placement, "hostile")
    key, _ = sr.keys_of(v, *box((0, 0, 0), (1, 1, 1), 5))
    outside = np.nonzero(key == sr.OUTSIDE)[0]
    assert len(outside) > 200 and got.vertices[want.cluster[outside]].tobytes() == v[outside].tobytes()      # what is outside stays, bit for bit
    assert (got.source < 2500).all() and not np.isin([3, 50, 51, 700, 10, 11, 12], got.source).any()


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("exponent", [-100, -20, 20, 100])
def test_meshes_scaled_by_powers_of_two(renderer, exponent, placement):
    v, f = sr.sphere(13, 20)
    s = F(2.0 ** exponent)
    got, want = against_the_restatement(renderer, v * s, f, tuple(F(-0.9) * s for _ in range(3)), tuple(F(0.9) * s for _ in range(3)), 5, placement, exponent)
    # a power of two changes nothing -- until the cross products leave float32 (edges beyond about 2^-37 .. 2^31): then no triangle
    # contributes and quadric placement is the mean
    like = sr.MEAN if abs(exponent) == 100 else drt.SIMPLIFY_PLACEMENTS[placement]
    unit = sr.simplify(v, f, *box((-0.9,) * 3, (0.9,) * 3, 5), like)
    assert want.counts == unit.counts and (want.vertices / s).tobytes() == unit.vertices.tobytes()
    assert abs(exponent) != 100 or not want.sums[:, 4:].any()


def small_mesh():
    v, f = cloud(40, 60, 31)
    v[7, 0] = np.nan
    return v, f


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_every_capacity_with_sentinels_behind_it(renderer, placement):
    v, f = small_mesh()
    lo, cell, dims = box((0, 0, 0), (1, 1, 1), 2)
    want = sr.simplify(v, f, lo, cell, dims, drt.SIMPLIFY_PLACEMENTS[placement])
    C, M = want.counts
    assert 4 < C < 12 and 10 < M < 60
    grid = drt._Grid()
    grid.lo[:], grid.cell[:], grid.dims[:] = [float(x) for x in lo], [float(x) for x in cell], [int(x) for x in dims]
    dv, df = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    import ctypes
    for vc, tc in [(vc, M) for vc in range(C + 6)] + [(C, tc) for tc in range(M + 6)] + [(0, 0), (C + 5, M + 5)]:
        cluster = torch.full((40,), -7, dtype=torch.int32, device=DEV)
        ov = torch.full((vc + 3, 3), -7.0, dtype=torch.float32, device=DEV)
        fi = torch.full((vc + 3,), -7, dtype=torch.int32, device=DEV)
        of = torch.full((tc + 3, 3), -7, dtype=torch.int32, device=DEV)
        so = torch.full((tc + 3,), -7, dtype=torch.int32, device=DEV)
        counts = torch.full((3,), -7, dtype=torch.int32, device=DEV)
        rc = drt._lib.drt_renderer_simplify(renderer._h, dv.data_ptr(), 40, df.data_ptr(), 60, ctypes.byref(grid), drt.SIMPLIFY_PLACEMENTS[placement],
                                            cluster.data_ptr(), ov.data_ptr() if vc else None, fi.data_ptr() if vc else None, vc,
                                            of.data_ptr() if tc else None, so.data_ptr() if tc else None, tc, counts.data_ptr(), stream)
        assert rc == 0, drt._lib.drt_last_error()
        assert counts.tolist() == [C, M, -7] and cluster.tolist() == want.cluster.tolist(), (vc, tc)
        kv, kt = min(vc, C), min(tc, M)
        assert fi[:kv].tolist() == want.first[:kv].tolist() and (fi[kv:] == -7).all(), (vc, tc)
        assert ov[:kv].cpu().numpy().tobytes() == want.vertices[:kv].tobytes() and (ov[kv:] == -7).all(), (vc, tc)
        assert of[:kt].tolist() == want.faces[:kt].tolist() and (of[kt:] == -7).all(), (vc, tc)
        assert so[:kt].tolist() == want.source[:kt].tolist() and (so[kt:] == -7).all(), (vc, tc)
    # no vertices: C = M = 0 and nothing else is looked at
    counts = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    rc = drt._lib.drt_renderer_simplify(renderer._h, None, 0, df.data_ptr(), 60, ctypes.byref(grid), 1, None, None, None, 0, None, None, 0, counts.data_ptr(), stream)
    assert rc == 0 and counts.tolist() == [0, 0, -7]


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_numpy_tensors_a_side_stream_two_runs_and_the_default_box(renderer, placement):
    v, f = sr.sphere(17, 30)
    v[3, 1] = np.nan
    host = renderer.simplify(drt.IndexedMesh(v, f, None), resolution=(5, 6, 4), placement=placement)
    assert isinstance(host, drt.SimplifiedMesh) and all(isinstance(x, np.ndarray) for x in host)
    want = sr.simplify(v, f, *sr.default_grid(v, (5, 6, 4)), drt.SIMPLIFY_PLACEMENTS[placement])
    same(host, want, "numpy, the default box")
    assert (want.sums[:, 0] >= 1).sum() == want.counts[0] - 1                  # every finite vertex is in the default box
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        dv, df = torch.from_numpy(v).to(DEV, non_blocking=True), torch.from_numpy(f).to(DEV, non_blocking=True)
        dev = renderer.simplify((dv, df), resolution=(5, 6, 4), placement=placement)
        again = renderer.simplify(drt.IndexedMesh(dv, df, None), resolution=(5, 6, 4), placement=placement)
        by_cell = renderer.simplify((dv, df), cell=0.31, placement=placement)
    side.synchronize()
    assert all(torch.is_tensor(x) and x.is_cuda for x in dev)
    same(dev, want, "tensors on a side stream")
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(dev, again))      # two runs, the same bytes (a NaN among them)
    same(by_cell, sr.simplify(v, f, *sr.default_grid(v, None, 0.31), drt.SIMPLIFY_PLACEMENTS[placement]), "cell=")
    assert torch.equal(dev.triangles().view(torch.int32), dev.vertices[dev.faces.long()].view(torch.int32))
    empty = renderer.simplify((np.zeros((0, 3), F), np.zeros((0, 3), np.int32)), resolution=3, placement=placement)
    assert [x.shape for x in empty] == [(0, 3), (0, 3), (0,), (0,), (0,)]
    # what takes an IndexedMesh takes the result
    normals = renderer.vertexNormals(host)
    assert normals.tobytes() == wd.vertex_normals(want.vertices, want.faces).tobytes()
    assert renderer.smooth(host, iterations=1).vertices.tobytes() == wd.smooth(want.vertices, want.faces, [0.5, -0.53]).tobytes()


def test_both_forms_of_the_sums_give_the_same_bytes(renderer, monkeypatch):
    """the library combines runs of lanes that name one cluster before its atomics; DRT_SIMPLIFY_SUMS=plain adds term by term"""
    soup = np.random.default_rng(8).integers(0, 10, (20_000, 3, 3)).astype(F)
    v, f, _, _ = wd.weld(soup)
    order = np.lexsort((v[:, 0], v[:, 1], v[:, 2]))                             # neighbours in memory are neighbours in space: long runs
    rank = np.empty(len(v), np.int64)
    rank[order] = np.arange(len(v))
    v, f = v[order], rank[f].astype(np.int32)
    f = f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))]
    results = {}
    for form in ("plain", "runs", None):
        if form is None:
            monkeypatch.delenv("DRT_SIMPLIFY_SUMS", raising=False)
        else:
            monkeypatch.setenv("DRT_SIMPLIFY_SUMS", form)
        results[form] = against_the_restatement(renderer, v, f, (-0.5, -0.5, -0.5), (9.5, 9.5, 9.5), 2, "quadric", form)[0]
    assert results["plain"].vertices.tobytes() == results["runs"].vertices.tobytes() == results[None].vertices.tobytes()


def open_torus(seed=17):
    pos = ir.torus()
    keep = np.ones(len(pos), bool)
    keep[np.random.default_rng(seed).choice(len(pos), len(pos) // 10, replace=False)] = False
    return pos[keep]


def shells_of(faces):
    """(triangles per shell sorted, open half-edges, bad half-edges) of an index buffer by integers: drt.h "mesh topology" on twins_of"""
    adj = wd.twins_of(faces).reshape(-1)
    label = np.arange(len(faces))

    def find(t):
        while label[t] != t:
            label[t] = label[label[t]]
            t = label[t]
        return t

    for h in np.nonzero(adj >= 0)[0]:
        a, b = find(h // 3), find(adj[h] // 3)
        label[max(a, b)] = min(a, b)
    roots = np.array([find(t) for t in range(len(faces))])
    return sorted(np.unique(roots, return_counts=True)[1].tolist()), int((adj == -1).sum()), int((adj == -2).sum())


def test_end_to_end_a_damaged_torus_remeshed_welded_simplified_and_shaded(renderer):
    damaged, _ = rq.programmatic_scene(drt, *ir.streams(open_torus()), 4, 8)
    mesh = renderer.weld(renderer.remesh(damaged, 32))
    small = renderer.simplify(mesh, resolution=12)
    v, f = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
    want = sr.simplify(v, f, *sr.default_grid(v, 12))
    same(small, want, "remesh")
    n_tris = small.faces.shape[0]
    assert 0 < n_tris < len(f) // 4 and sr.directed_edge_balance(small.faces.cpu().numpy())      # closed in, closed out, by integers
    normals = renderer.vertexNormals(small)
    assert normals.cpu().numpy().tobytes() == wd.vertex_normals(want.vertices, want.faces).tobytes()
    sc = small.toScene(normals=normals)
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = 4, 8
    b.buildIterative(sc)
    sh = renderer.shells(sc)
    sizes, open_edges, bad_edges = shells_of(want.faces)
    assert sh.count == len(sizes) and sorted(sh.triangles.tolist()) == sizes
    assert int(np.sum(sh.open_edges)) == open_edges == 0 and int(np.sum(sh.bad_edges)) == bad_edges
    # the renderer's shading normal at the three corners of every triangle is the vertex normal, bit for bit
    order = np.asarray(sc.triangleOrder(), np.int64)                          # tree index -> load index
    prim = np.arange(n_tris, dtype=np.int32)
    faces, nrm = small.faces.cpu().numpy(), normals.cpu().numpy()
    for k, (u, w) in enumerate(((0.0, 0.0), (1.0, 0.0), (0.0, 1.0))):
        s = renderer.surface(sc, prim, np.full(n_tris, u, np.float32), np.full(n_tris, w, np.float32))
        assert s.load_index.tolist() == order.tolist()
        assert s.shading.tobytes() == nrm[faces[order, k]].tobytes(), k
