"""Edge adjacency on the device (drt_renderer_tri_adjacency / _face_adjacency / _boundary_vertices, kernel_adjacency.hip, and the
uploaded scene's table) against tests/adjacency_ref.py, byte for byte: half-edge counts around a wave, a workgroup and the scan's
trips on soups without and with crowds, copies of one triangle, twins, fans, zero-length edges, every special bit pattern, both
strides, numpy, tensors and a side stream, a truncated capacity; a sphere's isosurface by position and by index, its Euler
characteristic, its boundary after holes are cut, smoothing with fixed="boundary", a simplified mesh; the scene's table on both routes
and after a device refit; and intersection curves through the device table."""
import os

import numpy as np
import pytest

from tests import adjacency_inputs as ai
from tests import adjacency_ref as ar
from tests import contour_scenes as cs
from tests import hostile_surfaces as hs
from tests import topology_scenes as ts
from tests import weld_ref as wd

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FAMILIES = dict(ai.families())


@pytest.fixture(scope="module")
def renderer():
    return drt.Renderer(0)


def host(x):
    return x.cpu().numpy() if torch.is_tensor(x) else x


def same_tables(renderer, tris, what):
    """by position and, on the restated weld's faces, by index; with and without the edges: the restatement's bytes"""
    adj, edge, half_edge = ar.by_position(tris)
    faces = wd.weld(tris)[1]
    vertices = np.zeros((int(faces.max(initial=-1)) + 1, 3), np.float32)      # (never read: the index route reads no vertex)
    for mesh in (tris, (vertices, faces)):
        got = renderer.edgeAdjacency(mesh)
        assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got.shape == adj.shape, what
        assert got.tobytes() == adj.tobytes(), what
        me = renderer.edgeAdjacency(mesh, edges=True)
        assert me.count == len(half_edge), what
        for g, w in zip(me[:3], (adj, edge, half_edge)):
            assert g.dtype == np.int32 and g.shape == w.shape and g.tobytes() == w.tobytes(), what
    return adj


@pytest.mark.parametrize("n", ai.COUNTS)
def test_half_edge_counts_around_every_seam(renderer, n):
    assert (same_tables(renderer, FAMILIES["distinct(%d)" % n], n) == -1).all()
    crowded = same_tables(renderer, FAMILIES["lattice(%d)" % n], n)
    assert n < 20000 or (crowded == -2).mean() > 0.9                           # 65 535 half-edges on the 7 750 pairs of 125 positions


@pytest.mark.parametrize("n", [64, 4096])
def test_one_triangle_many_times(renderer, n):
    assert (same_tables(renderer, FAMILIES["copies(%d)" % n], n) == -2).all()     # three slots take every half-edge


def test_twins_same_way_pairs_fans_and_zero_length_edges(renderer):
    assert same_tables(renderer, FAMILIES["reversed pair"], "reversed").tolist() == [[4, 3, 5], [1, 0, 2]]
    assert (same_tables(renderer, FAMILIES["same-way pair"], "same way") == -2).all()
    for n in (3, 4, 65):
        adj = same_tables(renderer, FAMILIES["fan(%d)" % n], "fan")
        assert (adj[:, 0] == -2).all() and (adj[:, 1:] == -1).all()
    assert same_tables(renderer, FAMILIES["zero length"], "zero length").tolist() == [[7, 6, -2], [-2, -2, -2], [1, 0, -2], [-2, -2, -2]]
    me = renderer.edgeAdjacency(FAMILIES["zero length"], edges=True)
    assert me.edge.tolist() == [[0, 1, 2], [-1, 2, 2], [1, 0, 2], [-1, -1, -1]] and me.half_edge.tolist() == [0, 1, 2]


def test_zeros_of_both_signs_nans_infinities_and_denormals(renderer):
    same_tables(renderer, FAMILIES["special"], "special")
    line = same_tables(renderer, FAMILIES["special line"], "special line")
    assert (line >= 0).any() and (line == -1).any() and (line == -2).any()
    assert same_tables(renderer, FAMILIES["special edges"], "special edges").tolist() == [[3, -1, -1], [0, -1, -1], [-2, 8, 7]]


def test_both_strides_numpy_tensors_and_a_side_stream(renderer):
    t = ai.lattice_soup(3000, 7, 21)
    want = ar.by_position(t)
    packed = np.zeros((3000, 12), np.float32)
    packed[:, 0:9] = t.reshape(-1, 9)
    packed[:, 9:12] = np.random.default_rng(1).standard_normal((3000, 3))    # (the pad words are not read)
    assert renderer.edgeAdjacency(t).tobytes() == want[0].tobytes()
    assert renderer.edgeAdjacency(packed).tobytes() == want[0].tobytes()
    faces = wd.weld(t)[1]
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        rec = torch.from_numpy(packed).to(DEV, non_blocking=True)
        view = rec[:, 0:9].unflatten(1, (3, 3))                               # what Isosurface.tris is: read in place, 48 bytes apart
        dev = renderer.edgeAdjacency(view, edges=True)
        dev36 = renderer.edgeAdjacency(torch.from_numpy(t).to(DEV, non_blocking=True))
        f = torch.from_numpy(faces).to(DEV, non_blocking=True)
        by_index = renderer.edgeAdjacency((torch.zeros((int(faces.max()) + 1, 3), device=DEV), f), edges=True)
        again = renderer.edgeAdjacency(view, edges=True)
    side.synchronize()
    assert view.stride() == (12, 3, 1) and all(torch.is_tensor(x) and x.is_cuda for x in dev[:3]) and torch.is_tensor(dev36)
    for got in (dev, by_index, again):
        assert got.count == len(want[2])
        for g, w in zip(got[:3], want):
            assert host(g).tobytes() == w.tobytes()
    assert host(dev36).tobytes() == want[0].tobytes()


def test_a_truncated_capacity_keeps_the_count_and_the_first_edges(renderer):
    t = ai.lattice_soup(2000, 9, 4)
    adj, edge, half_edge = ar.by_position(t)
    faces = torch.from_numpy(wd.weld(t)[1]).to(DEV)
    e = len(half_edge)
    d = torch.from_numpy(t).to(DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    for cap in (0, 1, e // 2, e, e + 5):
        for by_position in (True, False):
            a = torch.full((2000, 3), -7, dtype=torch.int32, device=DEV)
            ed = torch.full((2000, 3), -7, dtype=torch.int32, device=DEV)
            he = torch.full((max(cap, 1) + 3,), -7, dtype=torch.int32, device=DEV)
            count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
            tail = (a.data_ptr(), ed.data_ptr(), he.data_ptr() if cap else None, cap, count.data_ptr(), stream)
            if by_position:
                rc = drt._lib.drt_renderer_tri_adjacency(renderer._h, d.data_ptr(), 2000, 36, *tail)
            else:
                rc = drt._lib.drt_renderer_face_adjacency(renderer._h, faces.data_ptr(), 2000, *tail)
            assert rc == 0, drt._lib.drt_last_error()
            assert int(count.item()) == e and host(a).tobytes() == adj.tobytes() and host(ed).tobytes() == edge.tobytes(), cap
            k = min(cap, e)
            assert host(he)[:k].tolist() == half_edge[:k].tolist() and (he[k:] == -7).all(), cap
    # no edges asked for: nothing but adj is written; no triangles: nothing at all
    a = torch.full((2000, 3), -7, dtype=torch.int32, device=DEV)
    assert drt._lib.drt_renderer_tri_adjacency(renderer._h, d.data_ptr(), 2000, 36, a.data_ptr(), None, None, 0, None, stream) == 0
    assert host(a).tobytes() == adj.tobytes()
    count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    assert drt._lib.drt_renderer_face_adjacency(renderer._h, None, 0, None, None, None, 0, count.data_ptr(), stream) == 0
    assert int(count.item()) == -7
    assert renderer.edgeAdjacency(np.zeros((0, 3, 3), np.float32)).shape == (0, 3)
    assert renderer.edgeAdjacency(np.zeros((0, 3, 3), np.float32), edges=True).count == 0


def test_a_sphere_by_position_and_by_index_and_its_euler_characteristic(renderer):
    t = torch.from_numpy(ai.sphere()).to(DEV)
    mesh = renderer.weld(t)
    by_position, by_index = renderer.edgeAdjacency(t, edges=True), renderer.edgeAdjacency(mesh, edges=True)
    want = ar.by_position(ai.sphere())
    for got in (by_position, by_index):
        for g, w in zip(got[:3], want):
            assert host(g).tobytes() == w.tobytes()
    adj = by_index.adj.reshape(-1).to(torch.int64)
    assert (adj >= 0).all() and torch.equal(adj[adj], torch.arange(len(adj), device=DEV))
    assert 2 * by_index.count == 3 * len(t) and by_index.euler(len(mesh.vertices)) == 2
    assert not renderer.boundaryVertices(mesh).any()


def scene_of(mesh):
    sc = drt.IndexedMesh(*(host(x) for x in mesh[:3])).toScene()
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8                        # the editor's tree
    b.buildIterative(sc)
    return sc


def test_boundary_vertices_of_a_holed_sphere_and_smoothing_that_keeps_them(renderer):
    t = ai.holed_sphere()
    mesh = renderer.weld(t)
    v = len(mesh.vertices)
    adj = ar.by_index(mesh.faces)[0]
    want = ar.boundary_vertices(mesh.faces, adj, v)
    got = renderer.boundaryVertices(mesh)
    assert got.dtype == bool and got.tolist() == want.tolist() and 0 < got.sum() < v
    assert renderer.boundaryVertices(mesh, adj=adj).tolist() == want.tolist()
    assert renderer.boundaryVertices(mesh, bad=True).tolist() == want.tolist()          # no bad edge here
    dev = drt.IndexedMesh(*(torch.from_numpy(x).to(DEV) for x in mesh))
    on_device = renderer.boundaryVertices(dev, adj=renderer.edgeAdjacency(dev))
    assert torch.is_tensor(on_device) and on_device.dtype == torch.bool and host(on_device).tolist() == want.tolist()
    # ... and they are the vertices of the boundary loops of the mesh as a scene (tree order, by position)
    sc = scene_of(mesh)
    loops = renderer.boundaryLoops(sc)
    tree = ts.tree_positions(sc)
    ends = np.concatenate([tree[loops.prim, loops.edge], tree[loops.prim, (loops.edge + 1) % 3]])
    assert {p.tobytes() for p in ends} == {p.tobytes() for p in mesh.vertices[want]}
    # smoothing that keeps the boundary
    fixed = renderer.smooth(mesh, iterations=3, fixed="boundary")
    assert fixed.vertices.tobytes() == renderer.smooth(mesh, iterations=3, fixed=want).vertices.tobytes()
    assert fixed.vertices[want].tobytes() == mesh.vertices[want].tobytes()
    assert fixed.vertices.tobytes() != renderer.smooth(mesh, iterations=3).vertices.tobytes()
    with pytest.raises(drt.DrtError):
        renderer.smooth(mesh, fixed="edges")
    # the flag and the bounds check, against the restatement: three triangles on one edge, indices out of range on both sides
    f = np.int32([[0, 1, 2], [0, 1, 3], [0, 1, 4], [5, 6, 9], [7, -1, 8]])
    small = (np.zeros((9, 3), np.float32), f)
    a = renderer.edgeAdjacency(small)
    assert a.tobytes() == ar.by_index(f)[0].tobytes()
    for table in (a, np.where(a == -1, 0, a).astype(np.int32)):
        for bad in (False, True):
            assert renderer.boundaryVertices(small, adj=table, bad=bad).tolist() == ar.boundary_vertices(f, table, 9, bad).tolist()


@pytest.mark.parametrize("sheets", [1, 2])
def test_a_simplified_mesh_has_the_restatements_bad_edges(renderer, sheets):
    """resolution=4 on one sphere, and on two concentric ones (radii 0.8 and 0.72): there a cell holds two sheets of the surface, and
    clustering makes non-manifold edges -- 572 of 636 half-edges in the restatements"""
    t = ai.sphere()
    if sheets == 2:
        t = np.concatenate([t, (t * np.float32(0.9)).astype(np.float32)])
    small = renderer.simplify(renderer.weld(t), resolution=4)
    want = ar.by_index(small.faces)
    got = renderer.edgeAdjacency(small, edges=True)
    print("simplified: %d triangles, %d bad half-edges, %d open" % (len(small.faces), (want[0] == -2).sum(), (want[0] == -1).sum()))
    assert (got.adj == -2).sum() == (want[0] == -2).sum() and ((want[0] == -2).sum() > 0) == (sheets == 2)
    for g, w in zip(got[:3], want):
        assert g.tobytes() == w.tobytes()
    assert renderer.boundaryVertices(small, bad=True).tolist() == ar.boundary_vertices(small.faces, want[0], len(small.vertices), True).tolist()
    assert not renderer.boundaryVertices(small).any()


def device_table(r, sc):
    n = len(sc.m_PrimitivesBuffer)
    adj = torch.full((max(n, 1), 3), -7, dtype=torch.int32, device=DEV)
    assert drt._lib.drt_renderer_edge_adjacency(r._h, sc._h, adj.data_ptr(), None) == 0, drt._lib.drt_last_error()
    torch.cuda.synchronize()
    return adj[:n].cpu().numpy()


def route_scenes():
    for name in ts.ALL_NAMES:
        yield name, lambda name=name: ts.scene(drt, name)
    for name in hs.CAPPED_MESHES:                                              # (the fourth hostile mesh, the soup, is "degenerate" above)
        yield name, lambda name=name: cs.flat_scene(drt, hs.mesh(name).pos)[0]


@pytest.fixture(scope="module")
def host_route_renderer():
    before = os.environ.get("DRT_ADJACENCY")
    os.environ["DRT_ADJACENCY"] = "host"
    try:
        return drt.Renderer(0)                                                 # read when the renderer is created
    finally:
        if before is None:
            del os.environ["DRT_ADJACENCY"]
        else:
            os.environ["DRT_ADJACENCY"] = before


ROUTE_SCENES = list(route_scenes())


@pytest.mark.parametrize("name,make", ROUTE_SCENES, ids=[s[0] for s in ROUTE_SCENES])
def test_the_scenes_table_is_the_hosts_on_both_routes(renderer, host_route_renderer, name, make):
    sc = make()
    want = sc.edgeAdjacency()
    assert want.tobytes() == ar.by_position(ts.tree_positions(sc))[0].tobytes()
    for r, route in ((renderer, 2), (host_route_renderer, 1)):
        r.shells(sc)
        assert device_table(r, sc).tobytes() == want.tobytes(), (name, route)
        assert r.adjacencyRoute() == route, name


def test_a_device_refit_before_and_after_leaves_the_table_alone():
    """The table is made from the host scene's positions: a device refit that tears every triangle off its neighbours BEFORE the
    first topology call changes the device's records, not the table; one after it changes nothing either."""
    sc = ts.scene(drt, "two_cubes")
    pos = ts.positions("two_cubes")
    want = sc.edgeAdjacency()
    assert (want >= 0).all()
    torn = (pos + np.random.default_rng(3).random(pos.shape).astype(np.float32)).astype(np.float32)     # every corner moves on its own
    assert (ar.by_position(torn)[0] == -1).all()
    r = drt.Renderer(0)
    assert r.adjacencyRoute() == 0
    r.refit(sc, torch.from_numpy(torn).to(DEV))
    assert r.adjacencyRoute() == 0
    r.shells(sc)
    assert r.adjacencyRoute() == 2 and device_table(r, sc).tobytes() == want.tobytes()
    r.refit(sc, torch.from_numpy((pos + np.float32(1)).astype(np.float32)).to(DEV))
    assert device_table(r, sc).tobytes() == want.tobytes() and r.adjacencyRoute() == 2


def test_intersection_curves_through_the_device_table(renderer):
    sc = ts.scene(drt, "hollow_box")
    tool = (ai.sphere() * np.float32(1.6)).astype(np.float32)                  # radius 1.28: through the inner box's faces
    d = torch.from_numpy(tool).to(DEV)
    got = renderer.intersectionCurves(sc, d)
    want = renderer.intersectionCurves(sc, d, query_adj=drt.triEdgeAdjacency(d))
    assert len(got) == len(want) and len(host(got.chain_splits)) > 1
    for g, w in zip(got, want):
        assert host(g).tobytes() == host(w).tobytes()
    assert host(renderer.edgeAdjacency(d)).tobytes() == drt.triEdgeAdjacency(tool).tobytes()
