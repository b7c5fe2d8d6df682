"""The mesh-topology rule of include/drt.h as tests/topology_ref.py restates it (CPU only): the hand-derived shells, loops and measures
of the small meshes of tests/topology_scenes.py; the labels a fixed point and the loops a partition of the boundary on every one."""
import numpy as np
import pytest

from tests import contour_ref as cr
from tests import contour_scenes as cs
from tests import topology_ref as tr
from tests import topology_scenes as ts
from tests.tri_overlap_scenes import TETRAHEDRON

drt = pytest.importorskip("dustraytracer_amd")


def rows(slots):
    return [tuple(int(x) for x in s) for s in slots]


def topology(pos):
    """(adjacency, labels, counts, slots, loop counts) of positions as they stand, by the restatements alone."""
    adj = cr.adjacency(pos)
    label = tr.labels(adj)
    slots, loop_counts = tr.loops(adj)
    return adj, label, tr.counts(adj, label).tolist(), slots, loop_counts.tolist()


def measures(pos):
    adj = cr.adjacency(pos)
    index, tri = tr.per_shell(adj, tr.labels(adj))[:2]
    return tr.measures(tr.terms(*tr.packed(pos)), index, len(tri))[:3]


def test_the_single_triangle_is_one_shell_and_one_closed_loop_of_three():
    adj, label, counts, slots, loop_counts = topology(cs.SINGLE)
    assert label.tolist() == [0] and counts == [1, 3, 0]
    assert rows(slots) == [(0, 0, 3, 1), (1, 0, 3, 1), (2, 0, 3, 1)] and loop_counts == [3, 1, 1]
    area, volume, vector = measures(cs.SINGLE)
    assert area.tolist() == [0.5] and volume.tolist() == [0.0] and vector.tolist() == [[0.0, 0.0, 0.5]]


def test_the_quad_s_loop_runs_round_both_triangles():
    """Half-edges 2 and 3 are the diagonal.  0 ends at (1,0,0): edge 1 of the same triangle is open, succ(0) = 1.  1 ends at (1,1,0):
    edge 2 is the diagonal, its twin 3 is triangle 1's edge 0, whose next edge 4 is open: succ(1) = 4.  succ(4) = 5; 5 ends at (0,0,0):
    edge 0 of triangle 1 is 3, twin 2, triangle 0's next edge is 0: succ(5) = 0."""
    adj, label, counts, slots, loop_counts = topology(cs.QUAD)
    assert adj.tolist() == [-1, -1, 3, 2, -1, -1] and label.tolist() == [0, 0] and counts == [1, 4, 0]
    assert [tr.successor(adj, h)[0] for h in (0, 1, 4, 5)] == [1, 4, 5, 0]
    assert rows(slots) == [(0, 0, 4, 1), (1, 0, 4, 1), (4, 0, 4, 1), (5, 0, 4, 1)] and loop_counts == [4, 1, 1]
    # the other triangle first: half-edge 0 is the diagonal now, and the cycle starts at 1, its smallest member
    adj, label, counts, slots, loop_counts = topology(cs.QUAD[::-1])
    assert adj.tolist() == [5, -1, -1, -1, -1, 0] and slots["half_edge"].tolist() == [1, 2, 3, 4] and loop_counts == [4, 1, 1]


def test_the_tetrahedron_is_watertight_with_its_hand_volume_and_area():
    adj, label, counts, slots, loop_counts = topology(TETRAHEDRON)
    assert label.tolist() == [0, 0, 0, 0] and counts == [1, 0, 0] and len(slots) == 0 and loop_counts == [0, 0, 0]
    assert tr.per_shell(adj, label)[4].tolist() == [True]
    # the corner of a cube of side 4: volume 4^3 / 6; three faces of area 8 and one of |(16, 16, 16)| / 2
    term = tr.terms(*tr.packed(TETRAHEDRON))
    assert term["w"].tolist() == [0.0, 0.0, 0.0, 64.0] and term["c"].tolist() == [[0, 0, -16], [0, -16, 0], [-16, 0, 0], [16, 16, 16]]
    area, volume, vector = measures(TETRAHEDRON)
    assert volume.tolist() == [64.0 / 6.0] and vector.tolist() == [[0.0, 0.0, 0.0]] and area.tolist() == [0.5 * (48.0 + np.sqrt(768.0))]


def test_boxes_have_their_volumes_and_the_hollow_box_a_negative_one():
    pos = cs.positions("two_cubes")
    adj, label, counts, slots, loop_counts = topology(pos)
    assert label.tolist() == [0] * 12 + [12] * 12 and counts == [2, 0, 0] and loop_counts == [0, 0, 0]
    area, volume, vector = measures(pos)
    assert volume.tolist() == [1.0, 1.5] and area.tolist() == [6.0, 8.0] and not vector.any()
    pos = cs.positions("hollow_box")                                          # sides 4 and 2, the inner box's faces inward
    lo, hi = pos[:12].reshape(-1, 3).min(axis=0), pos[:12].reshape(-1, 3).max(axis=0)
    lo_in, hi_in = pos[12:].reshape(-1, 3).min(axis=0), pos[12:].reshape(-1, 3).max(axis=0)
    area, volume, vector = measures(pos)
    assert volume.tolist() == [float(np.prod(hi - lo)), -float(np.prod(hi_in - lo_in))] == [64.0, -8.0]
    assert area.tolist() == [96.0, 24.0] and not vector.any()
    assert tr.per_shell(cr.adjacency(pos), tr.labels(cr.adjacency(pos)))[4].tolist() == [True, True]


def test_the_book_is_three_shells_whose_loops_stop_at_the_spine():
    """Each leaf: edge 0 is the spine (-2), edges 1 and 2 are open.  3 t + 1 ends at the leaf's own vertex, where edge 2 follows;
    3 t + 2 ends on the spine: no successor, status 2."""
    adj, label, counts, slots, loop_counts = topology(cs.BOOK)
    assert label.tolist() == [0, 1, 2] and counts == [3, 6, 3]
    nm = cr.NON_MANIFOLD << 1
    assert rows(slots) == [(1, 0, 2, 0), (2, 0, 2, nm), (4, 2, 2, 0), (5, 2, 2, nm), (7, 4, 2, 0), (8, 4, 2, nm)] and loop_counts == [6, 3, 0]
    index, tri, open_edges, bad_edges, watertight = tr.per_shell(adj, label)
    assert tri.tolist() == [1, 1, 1] and open_edges.tolist() == [2, 2, 2] and bad_edges.tolist() == [1, 1, 1] and not watertight.any()


def test_the_flipped_quad_is_two_shells():
    adj, label, counts, slots, loop_counts = topology(cs.FLIPPED_QUAD)
    assert adj.tolist() == [-1, -1, -2, -1, -1, -2] and label.tolist() == [0, 1] and counts == [2, 4, 2]
    nm = cr.NON_MANIFOLD << 1
    assert rows(slots) == [(0, 0, 2, 0), (1, 0, 2, nm), (3, 2, 2, 0), (4, 2, 2, nm)] and loop_counts == [4, 2, 0]


def test_a_shared_vertex_joins_nothing_and_merges_no_loops():
    adj, label, counts, slots, loop_counts = topology(ts.CORNER_PAIR)
    assert (adj == -1).all() and label.tolist() == [0, 1] and counts == [2, 6, 0]
    assert rows(slots) == [(0, 0, 3, 1), (1, 0, 3, 1), (2, 0, 3, 1), (3, 3, 3, 1), (4, 3, 3, 1), (5, 3, 3, 1)] and loop_counts == [6, 2, 2]
    # two fans round one centre: each is a shell with a loop of three rim edges and two spokes, both through the centre
    pos = ts.two_fans()
    adj, label, counts, slots, loop_counts = topology(pos)
    assert label.tolist() == [0, 0, 0, 3, 3, 3] and counts == [2, 10, 0] and loop_counts == [10, 2, 2]
    lists = tr.loop_lists(slots)
    assert [len(m) for m, _ in lists] == [5, 5] and all(closed for _, closed in lists)
    assert {h // 3 for h in lists[0][0]} == {0, 1, 2} and {h // 3 for h in lists[1][0]} == {3, 4, 5}


def test_the_open_fan_rotates_through_every_spoke():
    pos = ts.open_fan()
    adj, label, counts, slots, loop_counts = topology(pos)
    n = ts.FAN_VALENCE - 1
    assert len(pos) == n and (label == 0).all() and counts == [1, n + 2, 0] and loop_counts == [n + 2, 1, 1]
    steps = [tr.successor(adj, int(h))[2] for h in slots["half_edge"]]
    assert max(steps) == n - 1 and sorted(steps)[:-1] == [0] * 2 + [1] * (n - 1)      # the rim turns through one twin, the last spoke through all


@pytest.mark.parametrize("name", ts.CPU_NAMES)
def test_the_labels_are_a_fixed_point_and_the_loops_partition_the_boundary(name):
    sc = ts.scene(drt, name)
    adj = cr.adjacency(ts.tree_positions(sc))
    label = tr.labels(adj)
    n = len(label)
    assert (label <= np.arange(n)).all() and (label[label] == label).all()
    has = np.nonzero(adj >= 0)[0]
    assert (label[has // 3] == label[adj[has] // 3]).all()                   # equal across every twin pair
    slots, loop_counts = tr.loops(adj)
    assert sorted(slots["half_edge"].tolist()) == np.nonzero(adj == -1)[0].tolist()      # every boundary half-edge in exactly one loop
    for members, closed in tr.loop_lists(slots):
        assert len({int(label[h // 3]) for h in members}) == 1              # a loop lies in one shell
        assert not closed or members[0] == min(members)
        for a, b in zip(members, members[1:] + (members[:1] if closed else [])):
            assert tr.successor(adj, a)[0] == b
    shells = int((label == np.arange(n)).sum())
    print("%s: %d triangles, %d shells, %d open and %d bad half-edges, %d loops (%d closed)"
          % (name, n, shells, (adj == -1).sum(), (adj == -2).sum(), loop_counts[1], loop_counts[2]))
    want = {"single": (1, 1, 1), "quad": (1, 1, 1), "tetrahedron": (1, 0, 0), "two_cubes": (2, 0, 0), "hollow_box": (2, 0, 0), "book": (3, 3, 0),
            "flipped_quad": (2, 2, 0), "corner_pair": (2, 2, 2), "two_fans": (2, 2, 2), "open_fan": (1, 1, 1), "ring": (1, 2, 2), "strip": (1, 1, 1)}
    if name in want:
        assert (shells, int(loop_counts[1]), int(loop_counts[2])) == want[name]
    if name == "ring":
        assert [len(m) for m, _ in tr.loop_lists(slots)] == [cs.RING_QUADS] * 2
    if name == "strip":
        assert n == 2 * ts.STRIP_QUADS and len(slots) == 2 * ts.STRIP_QUADS + 2
        assert measures(ts.tree_positions(sc))[0].tolist() == [float(ts.STRIP_QUADS)]
