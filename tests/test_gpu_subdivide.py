"""Subdivision on the device (drt_renderer_subdivide, kernel_subdivide.hip) against tests/subdivide_ref.py, byte for byte and for both
schemes: welded soups with half-edge counts around a wave, a workgroup and the scan's trips, without and with crowds; one edge with
thousands of members, fans, a vertex with 4 096 neighbours, twins and same-way pairs; faces that repeat a vertex, indices out of range,
every special bit pattern, M = 0, M near FLT_MAX and near the smallest denormal, unused vertices; a sphere's isosurface whole, holed
and simplified into a non-manifold mesh, two levels deep; numpy, tensors, a side stream, every capacity, no parents, no levels, and a
SubdividedMesh handed on to the other mesh calls and to a scene."""
import numpy as np
import pytest

from tests import adjacency_inputs as ai
from tests import adjacency_ref as ar
from tests import subdivide_ref as sr
from tests import weld_ref as wd

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FAMILIES = dict(ai.families())
SCHEMES = (("midpoint", sr.MIDPOINT), ("loop", sr.LOOP))
_welded = {}


@pytest.fixture(scope="module")
def renderer():
    return drt.Renderer(0)


def host(x):
    return x.cpu().numpy() if torch.is_tensor(x) else x


def welded(name):
    """(vertices, faces) of a family of tests/adjacency_inputs.py, welded by the restatement, made once"""
    if name not in _welded:
        v, f = wd.weld(FAMILIES[name])[:2]
        _welded[name] = (np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32))
    return _welded[name]


def same_bytes(got, want, what):
    for g, w, field in zip(got, want, ("vertices", "faces", "parents")):
        g = host(g)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, field, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, field, int((g.view(np.uint32) != w.view(np.uint32)).sum()))


def same_mesh(renderer, v, f, what):
    """both schemes: the restatement's bytes; returns the restatement's detail of the Loop level"""
    detail = {}
    for name, code in SCHEMES:
        want = sr.subdivide(v, f, code, detail)
        got = renderer.subdivide((v, f), scheme=name)
        assert isinstance(got, drt.SubdividedMesh) and isinstance(got.vertices, np.ndarray), what
        same_bytes(got, want, (what, name))
    return detail


@pytest.mark.parametrize("n", ai.COUNTS)
def test_half_edge_counts_around_every_seam(renderer, n):
    d = same_mesh(renderer, *welded("distinct(%d)" % n), ("distinct", n))
    assert (d["n_cr"] == 2).all() and not d["interior"].any()                   # every triangle on its own
    d = same_mesh(renderer, *welded("lattice(%d)" % n), ("lattice", n))
    assert n < 20000 or (d["n_cr"] > 2).mean() > 0.9                            # 125 vertices, every one of them crowded


@pytest.mark.parametrize("n", [64, 4096])
def test_one_triangle_many_times_is_three_edges(renderer, n):
    v, f = welded("copies(%d)" % n)
    d = same_mesh(renderer, v, f, ("copies", n))
    assert len(d["half_edge"]) == 3 and d["n_cr"].tolist() == [2, 2, 2]         # an edge counts once however many triangles share it
    got = renderer.subdivide((v, f))
    assert len(got.vertices) == 6 and (got.vertices[:3] != v).any()


def test_fans_pairs_and_a_vertex_with_4096_neighbours(renderer):
    for n in (3, 4, 65):
        d = same_mesh(renderer, *welded("fan(%d)" % n), ("fan", n))
        assert d["n_cr"][:2].tolist() == [n + 1, n + 1] and (d["n_cr"][2:] == 2).all()
    d = same_mesh(renderer, *welded("reversed pair"), "reversed pair")
    assert d["interior"].all() and d["n_int"].tolist() == [2, 2, 2]
    d = same_mesh(renderer, *welded("same-way pair"), "same-way pair")
    assert not d["interior"].any() and d["n_cr"].tolist() == [2, 2, 2]
    n = 4096                                                                   # a closed fan round vertex 0: 4 096 atomics on one sum
    a = 2 * np.pi * np.arange(n) / n
    v = np.concatenate([np.float32([[0.1, -0.2, 0.7]]), np.stack([np.cos(a), np.sin(a), 0.05 * np.cos(7 * a)], axis=1).astype(np.float32)])
    ring = np.arange(n, dtype=np.int32)
    f = np.stack([np.zeros(n, np.int32), 1 + ring, 1 + (ring + 1) % n], axis=1)
    d = same_mesh(renderer, v, f, "closed fan")
    assert d["n_int"][0] == n and d["n_cr"][0] == 0 and (d["n_cr"][1:] == 2).all() and (d["n_int"][1:] == 1).all()


def test_faces_that_repeat_a_vertex_and_indices_out_of_range(renderer):
    same_mesh(renderer, *welded("zero length"), "zero length")
    rng = np.random.default_rng(11)
    v = rng.standard_normal((9, 3)).astype(np.float32)
    big = 2 ** 31 - 1
    f = np.int32([[0, 1, 2], [2, 1, 3], [3, 3, 4], [5, 5, 5], [4, 3, 4], [0, -1, 1], [1, 9, 2], [big, 2, 3], [big, big, 0], [-1, 9, big],
                  [6, 7, -1], [7, 6, 9], [-2 ** 31, 0, 5]])
    d = same_mesh(renderer, v, f, "hostile indices")                           # (vertex 8 is used by no face)
    got = renderer.subdivide((v, f))
    assert (~d["usable"]).sum() >= 10 and (got.vertices[9:].view(np.uint32)[~d["usable"]] == sr.NAN_WORD).all()
    assert got.faces[4 * 2].tolist()[0] == 3 and got.faces[4 * 3].tolist() == [5, 5, 5] and got.faces[4 * 3 + 3].tolist() == [5, 5, 5]      # m(h) = faces[h]
    assert (got.faces == big).sum() >= 4 and (got.faces == -1).sum() >= 3 and (got.faces == 9).sum() >= 3      # the children copy the index
    assert got.vertices[8].tobytes() == v[8].tobytes() and got.parents[8].tolist() == [8, 8]
    # no vertices at all: every index is out of range, every odd vertex is the NaN words
    none = np.zeros((0, 3), np.float32)
    d = same_mesh(renderer, none, f[:4], "no vertices")
    assert not d["usable"].any()


def test_special_values_zero_and_the_ends_of_the_range(renderer):
    d = same_mesh(renderer, *welded("special"), "special")
    assert 0 < d["usable"].sum() < len(d["usable"])
    same_mesh(renderer, *welded("special line"), "special line")
    same_mesh(renderer, *welded("special edges"), "special edges")
    v, f = welded("sphere")
    assert same_mesh(renderer, np.zeros_like(v), f, "M = 0")["k"] == 0
    assert same_mesh(renderer, (v * np.float32(-0.0)).astype(np.float32), f, "M = 0, signed")["k"] == 0
    huge = (v.astype(np.float64) * (3.2e38 / float(np.abs(v).max()))).astype(np.float32)      # M = 3.2e38, above 2^127
    assert np.isfinite(huge).all() and same_mesh(renderer, huge, f, "M near FLT_MAX")["k"] == 27 - 127
    tiny = (np.round(v * 7) * np.float32(1e-45)).astype(np.float32)            # whole multiples of the smallest denormal, up to 6
    assert 0 < np.abs(tiny).max() < 1e-44 and same_mesh(renderer, tiny, f, "M near the smallest denormal")["k"] == 27 + 147
    mixed = v.copy()
    mixed[::7] *= np.float32(1e-42)                                            # denormals beside ordinary values
    mixed[5, 1], mixed[11, 0] = np.inf, -np.inf
    mixed.view(np.uint32)[17, 2] = 0xFFC00123
    same_mesh(renderer, mixed, f, "mixed")
    extra = np.concatenate([v, np.float32([[5, 5, 5], [np.nan, 0, 0]])])       # vertices no face uses; the first one sets M
    d = same_mesh(renderer, extra, f, "unused")
    assert d["k"] == 27 - 2 and d["n_int"][-2:].tolist() == [0, 0]


def test_a_sphere_stays_closed_two_levels_deep(renderer):
    v, f = welded("sphere")
    d = same_mesh(renderer, v, f, "sphere")
    assert d["interior"].all() and (d["n_cr"] == 0).all() and (d["n_int"] >= 3).all()
    for name, code in SCHEMES:
        want = sr.levels(v, f, 2, code)
        mesh = drt.IndexedMesh(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), None)
        got = renderer.subdivide(mesh, levels=2, scheme=name)
        assert all(torch.is_tensor(x) and x.is_cuda for x in got)
        same_bytes(got, want, ("two levels", name))
        edges = renderer.edgeAdjacency(got, edges=True)
        adj = edges.adj.reshape(-1).to(torch.int64)
        assert (adj >= 0).all() and torch.equal(adj[adj], torch.arange(len(adj), device=DEV))     # closed in, closed out
        assert len(got.faces) == 16 * len(f) and edges.euler(len(got.vertices)) == 2 == ar.euler(len(v), len(d["half_edge"]), len(f))
    r2 = np.linalg.norm(host(got.vertices).astype(np.float64), axis=1)
    assert r2.std() < np.linalg.norm(v.astype(np.float64), axis=1).std()       # Loop made it rounder


def test_a_holed_sphere_has_every_kind_of_vertex(renderer):
    v, f = welded("holed sphere")
    d = same_mesh(renderer, v, f, "holed sphere")
    kinds = set(d["n_cr"].tolist())
    assert 0 in kinds and 2 in kinds and len(kinds - {0, 2}) > 0, kinds         # smooth, crease, and vertices that stay
    want = sr.levels(v, f, 2, sr.LOOP)
    same_bytes(renderer.subdivide((v, f), levels=2), want, "holed sphere, two levels")
    adj2 = ar.by_index(want[1])[0]
    assert (adj2 == -1).sum() == 4 * (d["adj"] == -1).sum() and (adj2 == -2).sum() == 0      # a boundary stays one


def test_a_simplified_non_manifold_mesh(renderer):
    t = ai.sphere()
    t = np.concatenate([t, (t * np.float32(0.9)).astype(np.float32)])          # two concentric sheets in one cell: tests/test_gpu_adjacency.py
    small = renderer.simplify(renderer.weld(t), resolution=4)
    d = same_mesh(renderer, small.vertices, small.faces, "simplified")
    assert (d["adj"] == -2).sum() > 0 and (d["n_cr"] > 2).any()
    got = renderer.subdivide(small, levels=2)                                  # a SimplifiedMesh goes in unchanged
    same_bytes(got, sr.levels(small.vertices, small.faces, 2, sr.LOOP), "simplified, two levels")
    # a fan stays one: each of its half-edges becomes two per level (and triangles that clustering made equal share their inner edges too)
    assert (ar.by_index(got.faces)[0] == -2).sum() >= 4 * (d["adj"] == -2).sum()


def test_numpy_tensors_a_side_stream_and_two_runs(renderer):
    v, f = welded("lattice(1366)")
    want = {name: sr.subdivide(v, f, code) for name, code in SCHEMES}
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        dv, df = torch.from_numpy(v).to(DEV, non_blocking=True), torch.from_numpy(f).to(DEV, non_blocking=True)
        runs = [(name, renderer.subdivide((dv, df), scheme=name)) for name in ("loop", "midpoint", "loop", "midpoint")]
    side.synchronize()
    for name, got in runs:
        assert all(torch.is_tensor(x) and x.is_cuda for x in got)
        same_bytes(got, want[name], ("side stream", name))
    for name, _ in SCHEMES:
        same_bytes(renderer.subdivide(drt.IndexedMesh(v, f, None), scheme=name), want[name], ("numpy", name))
    # levels=0 returns the input's arrays
    none = renderer.subdivide((v, f), levels=0)
    assert none.vertices is v and none.faces is f and none.parents is None
    none = renderer.subdivide((dv, df), levels=0, scheme="midpoint")
    assert none.vertices is dv and none.faces is df
    empty = renderer.subdivide((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)))
    assert empty.vertices.shape == (0, 3) and empty.faces.shape == (0, 3) and empty.parents.shape == (0, 2)
    loose = renderer.subdivide((v, np.zeros((0, 3), np.int32)))                 # no triangles: the vertices are copied
    assert loose.vertices.tobytes() == v.tobytes() and loose.parents.tolist() == [[i, i] for i in range(len(v))] and len(loose.faces) == 0


def test_every_capacity_and_no_parents(renderer):
    v, f = welded("lattice(86)")
    nv, nt = len(v), len(f)
    dv, df = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    for name, code in SCHEMES:
        want_v, want_f, want_p = sr.subdivide(v, f, code)
        total = len(want_v)
        assert total > nv + 3
        for cap in (0, 1, nv - 1, nv, nv + 1, total - 1, total, total + 5):
            for with_parents in (True, False):
                out_v = torch.full((cap + 3, 3), -7.0, dtype=torch.float32, device=DEV)
                out_p = torch.full((cap + 3, 2), -7, dtype=torch.int32, device=DEV)
                out_f = torch.full((4 * nt + 1, 3), -7, dtype=torch.int32, device=DEV)
                count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
                rc = drt._lib.drt_renderer_subdivide(renderer._h, dv.data_ptr(), nv, df.data_ptr(), nt, code, out_v.data_ptr() if cap else None,
                                                     out_p.data_ptr() if cap and with_parents else None, cap, out_f.data_ptr(),
                                                     count.data_ptr(), stream)
                assert rc == 0, drt._lib.drt_last_error()
                k = min(cap, total)
                what = (name, cap, with_parents)
                assert int(count.item()) == total, what                        # always the total
                assert host(out_f)[:4 * nt].tobytes() == want_f.tobytes() and (out_f[4 * nt:] == -7).all(), what
                assert host(out_v)[:k].tobytes() == want_v[:k].tobytes() and (out_v[k:] == -7).all(), what      # sentinels behind the stored part
                if with_parents:
                    assert host(out_p)[:k].tobytes() == want_p[:k].tobytes() and (out_p[k:] == -7).all(), what
                else:
                    assert (out_p == -7).all(), what


def test_a_subdivided_mesh_goes_on_to_the_other_calls(renderer):
    v, f = welded("holed sphere")
    mesh = renderer.subdivide((v, f))
    normals = renderer.vertexNormals(mesh)
    assert normals.shape == mesh.vertices.shape and np.isfinite(normals).all()
    edges = renderer.edgeAdjacency(mesh, edges=True)
    assert edges.adj.tobytes() == ar.by_index(mesh.faces)[0].tobytes()
    border = renderer.boundaryVertices(mesh)
    smooth = renderer.smooth(mesh, iterations=2, fixed="boundary")
    assert isinstance(smooth, drt.IndexedMesh) and smooth.first is None and smooth.faces is mesh.faces
    assert smooth.vertices[border].tobytes() == mesh.vertices[border].tobytes() and (smooth.vertices[~border] != mesh.vertices[~border]).any()
    again = renderer.subdivide(mesh, scheme="midpoint")
    same_bytes(again, sr.subdivide(mesh.vertices, mesh.faces, sr.MIDPOINT), "a SubdividedMesh in")
    small = renderer.simplify(mesh, resolution=6)
    assert 0 < len(small.faces) < len(mesh.faces)
    sc = mesh.toScene(normals=normals)
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
    b.buildIterative(sc)
    centres = mesh.triangles().mean(axis=1).astype(np.float32)[::37]
    origins = (centres * np.float32(3)).astype(np.float32)                      # outside the sphere, looking at a triangle's centre
    hits = renderer.traceRays(sc, origins, (centres - origins).astype(np.float32))
    assert (host(hits.prim) >= 0).all() and len(centres) > 10
