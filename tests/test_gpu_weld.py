"""Vertex welding, vertex normals and smoothing on the device (drt_renderer_weld / _vertex_normals / _smooth_vertices,
kernel_weld.hip) against tests/weld_ref.py, bit for bit: corner counts around a wave, a workgroup and the scan's trips, soups with no
and with nothing but duplicates, every special bit pattern, both strides, numpy, tensors and a side stream, a truncated capacity; both
normal weights and one and ten smoothing steps on a mesh with an index out of range, a lone vertex and a vertex that is not finite;
and a damaged torus remeshed, welded, smoothed and rendered with its vertex normals."""
import ctypes

import numpy as np
import pytest

from tests import inside_ref as ir
from tests import isosurface_ref as iso
from tests import ray_query_ref as rq
from tests import weld_ref as wd

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_cache = {}


@pytest.fixture(scope="module")
def renderer():
    return drt.Renderer(0)


def same_mesh(got, tris, what):
    vertices, faces, first, v = wd.weld(tris)
    g = [x.cpu().numpy() if torch.is_tensor(x) else x for x in got]
    assert g[0].shape == (v, 3) and g[0].dtype == np.float32 and g[1].dtype == np.int32 and g[2].dtype == np.int32, what
    assert g[1].tolist() == faces.tolist(), what
    assert g[2].tolist() == first.tolist(), what
    assert g[0].tobytes() == vertices.tobytes(), what


def distinct_soup(n, seed):
    """n triangles whose 3 n positions all differ"""
    t = np.random.default_rng(seed).standard_normal((n, 3, 3)).astype(np.float32)
    t[:, :, 0] += np.arange(3 * n, dtype=np.float32).reshape(n, 3)        # (x differs by at least ... the index: no two alike)
    assert len(np.unique(wd.corners(t), axis=0)) == 3 * n
    return t


def lattice_soup(n, side, seed):
    return np.random.default_rng(seed).integers(0, side, (n, 3, 3)).astype(np.float32)


# 63 | 66 corners straddle a wave, 255 | 258 a workgroup of the scan, 4 098 sixteen workgroups, 65 535 | 65 538 one trip of the offsets
@pytest.mark.parametrize("n", [1, 2, 21, 22, 85, 86, 1366, 21845, 21846])
def test_corner_counts_around_every_seam(renderer, n):
    for t in (distinct_soup(n, n), lattice_soup(n, 5, n + 1)):
        same_mesh(renderer.weld(t), t, n)


@pytest.mark.parametrize("n", [64, 4096])
def test_every_corner_at_one_position(renderer, n):
    t = np.full((n, 3, 3), 0.25, np.float32)
    t[:, :, 1], t[:, :, 2] = -3.5, 1e-40
    mesh = renderer.weld(t)
    same_mesh(mesh, t, n)
    assert mesh.vertices.shape == (1, 3) and mesh.first.tolist() == [0] and not mesh.faces.any()


def test_many_duplicates_on_a_small_lattice(renderer):
    t = lattice_soup(50_000, 12, 3)
    mesh = renderer.weld(t)
    same_mesh(mesh, t, "lattice")
    assert len(mesh.vertices) == 12 ** 3
    assert mesh.triangles().tobytes() == t.tobytes()                      # the gather gives the soup back


def special_soup(n=700, seed=9):
    pool = np.array([0x00000000, 0x80000000, 0x7FC00000, 0x7FC00001, 0xFFC00000, 0x7F800001, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001,
                     0x007FFFFF, 0x3F800000, 0x7F7FFFFF], np.uint32)
    return pool[np.random.default_rng(seed).integers(0, len(pool), (n, 3, 3))].view(np.float32)


def test_zeros_of_both_signs_nans_infinities_and_denormals(renderer):
    t = special_soup()
    mesh = renderer.weld(t)
    same_mesh(mesh, t, "special")
    words = mesh.vertices.view(np.uint32)
    assert len(np.unique(words, axis=0)) == len(words) > 1000              # 13^3 = 2197 possible positions, compared by their bits
    hand = np.zeros((2, 3, 3), np.float32)
    hand.view(np.uint32)[0, 1, 0], hand.view(np.uint32)[1, 0, 0], hand.view(np.uint32)[1, 1, 0] = 0x80000000, 0x7FC00000, 0x7FC00001
    mesh = renderer.weld(hand)
    same_mesh(mesh, hand, "hand")
    assert mesh.faces.tolist() == [[0, 1, 0], [2, 3, 0]]                  # +0 | -0 | +0, then two NaNs of different bits


def test_both_strides_numpy_tensors_and_a_side_stream(renderer):
    t = lattice_soup(3000, 7, 21)
    packed = np.zeros((3000, 12), np.float32)
    packed[:, 0:9] = t.reshape(-1, 9)
    packed[:, 9:12] = np.random.default_rng(1).standard_normal((3000, 3))  # (the pad words are not read)
    host = renderer.weld(t)
    assert all(isinstance(x, np.ndarray) for x in host)
    same_mesh(host, t, "36")
    same_mesh(renderer.weld(packed), t, "48")
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        rec = torch.from_numpy(packed).to(DEV, non_blocking=True)
        view = rec[:, 0:9].unflatten(1, (3, 3))                           # what Isosurface.tris is: read in place
        dev = renderer.weld(view)
        dev36 = renderer.weld(torch.from_numpy(t).to(DEV, non_blocking=True))
        again = renderer.weld(view)
    side.synchronize()
    assert view.stride() == (12, 3, 1) and all(torch.is_tensor(x) and x.is_cuda for x in dev)
    same_mesh(dev, t, "view")
    same_mesh(dev36, t, "tensor 36")
    assert all(torch.equal(a, b) for a, b in zip(dev, again))             # two runs, the same bytes
    assert torch.equal(dev.triangles(), view)


def test_a_truncated_capacity_keeps_faces_and_the_count(renderer):
    t = lattice_soup(2000, 9, 4)
    vertices, faces, first, v = wd.weld(t)
    d = torch.from_numpy(t).to(DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    for cap, with_vertices in ((0, False), (1, True), (v // 2, True), (v // 2, False), (v, True), (v + 5, True)):
        f = torch.full((2000, 3), -7, dtype=torch.int32, device=DEV)
        fi = torch.full((max(cap, 1) + 3,), -7, dtype=torch.int32, device=DEV)
        ve = torch.full((max(cap, 1) + 3, 3), -7.0, dtype=torch.float32, device=DEV)
        count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
        rc = drt._lib.drt_renderer_weld(renderer._h, d.data_ptr(), 2000, 36, f.data_ptr(), fi.data_ptr() if cap else None,
                                        ve.data_ptr() if with_vertices else None, cap, count.data_ptr(), stream)
        assert rc == 0, drt._lib.drt_last_error()
        assert int(count.item()) == v and f.cpu().numpy().tolist() == faces.tolist(), cap
        k = min(cap, v)
        assert fi.cpu().numpy()[:k].tolist() == first[:k].tolist() and (fi[k:] == -7).all(), cap
        if with_vertices:
            assert ve.cpu().numpy()[:k].tobytes() == vertices[:k].tobytes() and (ve[k:] == -7).all(), cap
        else:
            assert (ve == -7).all()


def sphere_mesh(res=14):
    """the restatement's isosurface of a sphere, welded by the restatement, with a lone vertex appended"""
    if ("sphere", res) not in _cache:
        lo, hi = np.float32([-1.03, -1.01, -1.02]), np.float32([1.01, 1.04, 1.02])
        f, cell = iso.sphere_sdf(res, lo, hi, 0.8)
        t = iso.triangles(iso.isosurface(f, 0.0, lo, cell)[1])
        vertices, faces, _, _ = wd.weld(t)
        _cache[("sphere", res)] = (np.concatenate([vertices, np.float32([[0.1, 0.2, 0.3]])]), faces)
    v, f = _cache[("sphere", res)]
    return v.copy(), f.copy()


def hostile_mesh():
    """... with indices out of range on both sides, a NaN vertex, an infinite one and a triangle that names a vertex twice"""
    v, f = sphere_mesh()
    f[5, 1], f[17, 0], f[40, 2] = len(v), -1, f[40, 0]
    v[f[100, 0], 1], v[f[300, 2], 0] = np.nan, np.inf
    return v, f


@pytest.mark.parametrize("weight", ["angle", "area"])
@pytest.mark.parametrize("mesh", [sphere_mesh, hostile_mesh])
def test_vertex_normals_are_the_restatements(renderer, mesh, weight):
    v, f = mesh()
    want = wd.vertex_normals(v, f, drt.NORMAL_WEIGHTS[weight])
    got = renderer.vertexNormals(drt.IndexedMesh(v, f, None), weight=weight)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32
    assert got.tobytes() == want.tobytes(), np.abs(got - want).max()
    dev = renderer.vertexNormals((torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)), weight=weight)
    assert dev.is_cuda and dev.cpu().numpy().tobytes() == want.tobytes()
    assert not got[-1].any() and np.abs(np.linalg.norm(got[:-1][np.isfinite(v[:-1]).all(axis=1)], axis=1) - 1).max() < 1e-6    # the lone vertex
    # scale does not change the result's nature: tiny and huge triangles go through the same fixed point
    for s in (np.float32(2.0 ** -60), np.float32(2.0 ** 40)):
        assert renderer.vertexNormals((v * s, f), weight=weight).tobytes() == wd.vertex_normals(v * s, f, drt.NORMAL_WEIGHTS[weight]).tobytes()


@pytest.mark.parametrize("factors", [[0.5], [0.5, -0.53] * 5, [], [0.0], [1.0, -1.0, 0.25]])
@pytest.mark.parametrize("mesh", [sphere_mesh, hostile_mesh])
def test_smoothing_is_the_restatements(renderer, mesh, factors):
    v, f = mesh()
    fixed = np.zeros(len(v), bool)
    fixed[::7] = True
    for fx in (None, fixed):
        want = wd.smooth(v, f, factors, fx)
        got = renderer.smooth(drt.IndexedMesh(v, f, None), factors=factors, fixed=fx)
        assert got.faces is f and got.vertices.tobytes() == want.tobytes(), (factors, np.nanmax(np.abs(got.vertices - want)))
        if fx is not None:
            assert got.vertices[fixed].tobytes() == v[fixed].tobytes()
    if not factors or factors == [0.0]:
        assert want.tobytes() == v.tobytes()
    dev = renderer.smooth(drt.IndexedMesh(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), None), factors=factors, fixed=torch.from_numpy(fixed).to(DEV))
    assert dev.vertices.is_cuda and dev.vertices.cpu().numpy().tobytes() == want.tobytes()


def test_the_keywords_of_smooth_and_coordinates_of_every_size(renderer):
    v, f = sphere_mesh()
    mesh = drt.IndexedMesh(v, f, None)
    assert renderer.smooth(mesh, iterations=3).vertices.tobytes() == wd.smooth(v, f, [0.5, -0.53] * 3).tobytes()
    assert renderer.smooth(mesh, iterations=4, lam=0.4, mu=None).vertices.tobytes() == wd.smooth(v, f, [0.4] * 4).tobytes()
    for s in (np.float32(2.0 ** -140), np.float32(2.0 ** 100), np.float32(0.0)):     # denormal coordinates, huge ones, all zeros
        assert renderer.smooth((v * s, f), factors=[0.5, -0.53]).vertices.tobytes() == wd.smooth(v * s, f, [0.5, -0.53]).tobytes()


def open_torus(seed=17):
    pos = ir.torus()
    keep = np.ones(len(pos), bool)
    keep[np.random.default_rng(seed).choice(len(pos), len(pos) // 10, replace=False)] = False
    return pos[keep]


def test_end_to_end_a_damaged_torus_welded_smoothed_and_shaded(renderer):
    damaged, _ = rq.programmatic_scene(drt, *ir.streams(open_torus()), 4, 8)
    surf = renderer.remesh(damaged, 24)
    mesh = renderer.weld(surf)
    same_mesh(mesh, surf.tris.cpu().numpy(), "remesh")
    n_tris, n_vertices = mesh.faces.shape[0], mesh.vertices.shape[0]
    edges, uses = wd.edges_of(mesh.faces.cpu().numpy())
    assert (uses == 2).all() and n_vertices - len(edges) + n_tris == 0     # a closed torus, by integers
    sm = renderer.smooth(mesh)                                            # Taubin, ten pairs
    assert sm.faces is mesh.faces and not torch.equal(sm.vertices, mesh.vertices)
    assert sm.vertices.cpu().numpy().tobytes() == wd.smooth(mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy(), [0.5, -0.53] * 10).tobytes()
    normals = renderer.vertexNormals(sm)
    assert normals.cpu().numpy().tobytes() == wd.vertex_normals(sm.vertices.cpu().numpy(), sm.faces.cpu().numpy()).tobytes()
    tris = sm.triangles()
    assert tris.shape == (n_tris, 3, 3) and (drt.triEdgeAdjacency(tris.cpu().numpy()) >= 0).all()
    sc = sm.toScene(normals=normals)
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = 4, 8
    b.buildIterative(sc)
    sh = renderer.shells(sc)
    assert sh.count == 1 and sh.watertight.tolist() == [True] and sh.triangles.tolist() == [n_tris]
    # the renderer's shading normal at the three corners of every triangle is the welded vertex normal, bit for bit
    order = np.asarray(sc.triangleOrder(), np.int64)                      # tree index -> load index
    prim = np.arange(n_tris, dtype=np.int32)
    faces, nrm = sm.faces.cpu().numpy(), normals.cpu().numpy()
    for k, (u, v) in enumerate(((0.0, 0.0), (1.0, 0.0), (0.0, 1.0))):
        s = renderer.surface(sc, prim, np.full(n_tris, u, np.float32), np.full(n_tris, v, np.float32))
        assert s.load_index.tolist() == order.tolist()
        want = nrm[faces[order, k]]
        assert s.shading.tobytes() == want.tobytes(), k
