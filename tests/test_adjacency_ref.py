"""tests/adjacency_ref.py on its own, without a GPU: by position it is drt.triEdgeAdjacency (the host routine, which
tests/cpp/edge_adjacency_check.cpp tests on its own and under a sanitizer) on every input family of the device tests; by index on the
restated weld's faces it is the table by position; the edge numbering is by first appearance and gives V - E + F = 2 per sphere; the
boundary flags follow the table."""
import numpy as np
import pytest

from tests import adjacency_inputs as ai
from tests import adjacency_ref as ar
from tests import weld_ref as wd

drt = pytest.importorskip("dustraytracer_amd")

FAMILIES = list(ai.families())


@pytest.mark.parametrize("name,tris", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_by_position_is_the_host_routine_and_by_index_agrees(name, tris):
    adj, edge, half_edge = ar.by_position(tris)
    host = drt.triEdgeAdjacency(tris)
    assert adj.dtype == np.int32 and adj.tobytes() == host.tobytes()
    packed = np.zeros((len(tris), 12), np.float32)
    packed[:, 0:9], packed[:, 9:12] = tris.reshape(-1, 9), 7.0
    assert ar.by_position(packed)[0].tobytes() == host.tobytes()                # the pad words are not read
    faces = wd.weld(tris)[1]
    for got, want in zip(ar.by_index(faces), (adj, edge, half_edge)):
        assert got.tobytes() == want.tobytes()
    # the numbering: a representative is the smallest half-edge of its edge, representatives ascend, every live half-edge has an edge
    flat = edge.reshape(-1)
    assert (np.diff(half_edge) > 0).all() and flat[half_edge].tolist() == list(range(len(half_edge)))
    live = flat >= 0
    assert (half_edge[flat[live]] <= np.flatnonzero(live)).all()
    w = ar.position_words(tris)
    ends_equal = (w == np.roll(w, -1, axis=1)).all(axis=2).reshape(-1)
    assert (live == ~ends_equal).all() and (adj.reshape(-1)[ends_equal] == -2).all()
    twins = adj.reshape(-1)
    paired = np.flatnonzero(twins >= 0)
    assert (twins[twins[paired]] == paired).all() and (flat[twins[paired]] == flat[paired]).all()


def test_what_the_families_are_meant_to_hit():
    table = dict((name, ar.by_position(t)[0]) for name, t in FAMILIES)
    for n in ai.COUNTS:
        assert (table["distinct(%d)" % n] == -1).all()
    assert (table["lattice(21846)"] == -2).mean() > 0.9
    for name in ("copies(64)", "copies(4096)", "same-way pair", "fan(3)", "fan(4)", "fan(65)"):
        assert (table[name][:, 0] == -2).all(), name
    assert (table["copies(4096)"] == -2).all() and (table["same-way pair"] == -2).all()
    assert (table["fan(65)"][:, 1:] == -1).all()
    assert table["reversed pair"].tolist() == [[4, 3, 5], [1, 0, 2]]
    # (A, B, C), (A, A, C), (C, B, A), (A, A, A): the edge A - C is there four times, the zero-length ones are in no group
    assert table["zero length"].tolist() == [[7, 6, -2], [-2, -2, -2], [1, 0, -2], [-2, -2, -2]]
    # +0 -> -0 and -0 -> +0 are twins; (NaN, NaN, NaN'): one zero-length edge, and the other two are each other's twins
    assert table["special edges"].tolist() == [[3, -1, -1], [0, -1, -1], [-2, 8, 7]]
    line = table["special line"]
    assert (line >= 0).any() and (line == -1).any() and (line == -2).any()


def test_a_closed_isosurface_has_euler_characteristic_two_per_sphere():
    t = ai.sphere()
    adj, edge, half_edge = ar.by_position(t)
    v = wd.weld(t)[3]
    assert (adj >= 0).all() and 2 * len(half_edge) == 3 * len(t)
    assert ar.euler(v, len(half_edge), len(t)) == 2
    two = np.concatenate([t, t + np.float32([4, 0, 0])])
    assert ar.euler(wd.weld(two)[3], len(ar.by_position(two)[2]), len(two)) == 4
    assert ar.euler(8, 12 + 6, 12) == 2                                          # a cube of twelve triangles


def test_boundary_vertices_follow_the_table():
    t = ai.holed_sphere()
    vertices, faces, _, v = wd.weld(t)
    adj = ar.by_index(faces)[0]
    assert (adj == -1).any() and not (adj == -2).any()
    got = ar.boundary_vertices(faces, adj, v)
    want = np.zeros(v, bool)
    for tri in range(len(faces)):
        for e in range(3):
            if adj[tri, e] == -1:
                want[faces[tri, e]] = want[faces[tri, (e + 1) % 3]] = True
    assert got.tolist() == want.tolist() and 0 < got.sum() < v
    # -2 counts only with the flag; a triangle with an index out of range is skipped, on both sides of the range
    f = np.int32([[0, 1, 2], [0, 1, 3], [0, 1, 4], [5, 6, 9], [7, -1, 8]])
    a = ar.by_index(f)[0]
    assert a.tolist() == [[-2, -1, -1], [-2, -1, -1], [-2, -1, -1], [-1, -1, -1], [-1, -1, -1]]
    assert ar.boundary_vertices(f, a, 9).tolist() == [True, True, True, True, True, False, False, False, False]
    assert ar.boundary_vertices(f, np.where(a == -1, 0, a), 9).tolist() == [False] * 9
    assert ar.boundary_vertices(f, np.where(a == -1, 0, a), 9, bad=True).tolist() == [True, True] + [False] * 7
    assert ar.boundary_vertices(f, a, 10)[[5, 6, 9]].all()


def test_mesh_edges_counts_its_euler_characteristic():
    me = drt.MeshEdges(np.zeros((12, 3), np.int32), np.zeros((12, 3), np.int32), np.zeros(18, np.int32), 18)
    assert drt.MeshEdges._fields == ("adj", "edge", "half_edge", "count") and me.euler(8) == 2
