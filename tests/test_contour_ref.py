"""The section-contour rule of include/drt.h as tests/contour_ref.py restates it (CPU only): the hand-derived adjacency and chains of the
tetrahedron, the quad, the book and the flipped quad; the adjacency an involution and the chains a partition on every small scene; and
the ring, whose plane z = 0 is one closed chain of 5 000 records."""
import numpy as np
import pytest

from tests import contour_ref as cr
from tests import contour_scenes as cs
from tests import nearest_ref as nr
from tests import section_ref as sr
from tests.tri_overlap_scenes import TETRAHEDRON

drt = pytest.importorskip("dustraytracer_amd")


def cut(pos, planes):
    """(records, splits, adjacency) of load-order positions, by the restatements alone."""
    rec, counts = sr.whole(nr.from_triangles(pos), planes)
    return rec, np.concatenate([[0], np.cumsum(counts.astype(np.int64))]), cr.adjacency(pos)


def rows(slots):
    return [tuple(int(x) for x in s) for s in slots]


def test_hand_adjacency_and_chains_of_the_tetrahedron():
    """Faces 0 (V0, V2, V1), 1 (V0, V1, V3), 2 (V0, V3, V2), 3 (V1, V2, V3).  Half-edge 0 runs V0 -> V2 and its twin is face 2's edge 2,
    V2 -> V0 = 8; 1 (V2 -> V1) and face 3's edge 0 = 9; 2 (V1 -> V0) and face 1's edge 0 = 3; 4 (V1 -> V3) and face 3's edge 2 = 11;
    5 (V3 -> V0) and face 2's edge 0 = 6; 7 (V3 -> V2) and face 3's edge 1 = 10."""
    assert cr.adjacency(TETRAHEDRON).tolist() == [8, 9, 3, 2, 11, 6, 5, 10, 0, 1, 7, 4]
    # z = 2 cuts faces 1, 2 and 3, each with V3 above alone: codes 6 (apex 2), 5 (apex 1), 6.  Face 1 is left through edge 1
    # (V1 -> V3, half-edge 4), whose twin 11 is face 3's edge 2 = its entry: record 0 -> record 2.  Face 3 is left through edge 1
    # (half-edge 10), twin 7 = face 2's edge 1 = its entry: record 2 -> record 1.  Face 2 is left through edge 0 (half-edge 6), twin 5
    # = face 1's edge 2 = its entry: record 1 -> record 0.  One cycle, started at its smallest record.
    pl = sr.pack([(0, 0, 1)], [2])
    rec, splits, adj = cut(TETRAHEDRON, pl)
    assert rec["prim"].tolist() == [1, 2, 3] and rec["code"].tolist() == [6, 5, 6]
    slots, chains = cr.chain(adj, rec, splits)
    assert rows(slots) == [(0, 0, 3, 1), (2, 0, 3, 1), (1, 0, 3, 1)] and chains.tolist() == [[1, 1]]
    area, mass = cr.areas(pl, rec, slots, chains, splits)
    assert area.tolist() == [2.0] and mass[0] >= 2.0                            # the section tests' area of 2
    # the contour's vertices: each record's q is the next one's p, and the last one's q the first one's p -- bit for bit here
    order = slots["seg"]
    assert (rec["q"][order] == rec["p"][np.roll(order, -1)]).all()


def test_the_quad_is_one_open_chain_whose_head_has_no_predecessor():
    """Triangle 0 (0,0,0), (1,0,0), (1,1,0) and 1 (0,0,0), (1,1,0), (0,1,0) share the diagonal: half-edges 2 and 3.  x = 0.5: triangle 0
    has its apex 0 below (code 0: in through edge 2, out through edge 0, a boundary edge); triangle 1 its apex 1 above (code 5: in
    through edge 1, out through edge 0 = half-edge 3, whose twin 2 is triangle 0's entry).  So record 1 -> record 0: the head is
    record 1, not the smallest index."""
    assert cr.adjacency(cs.QUAD).tolist() == [-1, -1, 3, 2, -1, -1]
    rec, splits, adj = cut(cs.QUAD, sr.pack([(1, 0, 0)], [0.5]))
    assert rec["prim"].tolist() == [0, 1] and rec["code"].tolist() == [0, 5]
    slots, chains = cr.chain(adj, rec, splits)
    assert rows(slots) == [(1, 0, 2, cr.LINKED << 1), (0, 0, 2, cr.BOUNDARY << 1)] and chains.tolist() == [[1, 0]]
    assert np.isnan(cr.areas(sr.pack([(1, 0, 0)], [0.5]), rec, slots, chains, splits)[0]).all()


def test_the_book_and_the_flipped_quad_stop_at_their_bad_edge():
    # three triangles on the edge (0,0,-1) - (0,0,1): -2 on it, boundary elsewhere
    assert cr.adjacency(cs.BOOK).tolist() == [-2, -1, -1, -2, -1, -1, -2, -1, -1]
    rec, splits, adj = cut(cs.BOOK, sr.pack([(0, 0, 1)], [0]))
    assert rec["code"].tolist() == [0, 0, 1]                     # two leave through the book's edge, the third enters through it
    slots, chains = cr.chain(adj, rec, splits)
    assert rows(slots) == [(0, 0, 1, cr.NON_MANIFOLD << 1), (1, 1, 1, cr.NON_MANIFOLD << 1), (2, 2, 1, cr.BOUNDARY << 1)]
    assert chains.tolist() == [[3, 0]]
    # the quad with triangle 1 reversed: the diagonal runs (1,1,0) -> (0,0,0) in both
    assert cr.adjacency(cs.FLIPPED_QUAD).tolist() == [-1, -1, -2, -1, -1, -2]
    rec, splits, adj = cut(cs.FLIPPED_QUAD, sr.pack([(-1, 0, 0), (1, 0, 0)], [-0.5, 0.5]))
    assert rec["code"].tolist() == [4, 2, 0, 6]                  # x < 0.5 above: both leave through edge 2; x > 0.5 above: through boundary edges
    slots, chains = cr.chain(adj, rec, splits)
    assert [r[3] >> 1 for r in rows(slots)] == [cr.NON_MANIFOLD, cr.NON_MANIFOLD, cr.BOUNDARY, cr.BOUNDARY]
    assert [r[:3] for r in rows(slots)] == [(0, 0, 1), (1, 1, 1), (2, 2, 1), (3, 3, 1)] and chains.tolist() == [[2, 0], [2, 0]]


def test_a_degenerate_triangle_can_be_its_own_neighbour():
    """(A, B, A): edge 0 runs A -> B and edge 1 B -> A, a pair of twins within one triangle; edge 2 has both ends at A."""
    pos = np.float32([[[0, 0, 0], [1, 0, 0], [0, 0, 0]]])
    assert cr.adjacency(pos).tolist() == [1, 0, -2]
    # -0.0 is not +0.0: the positions differ in their bits
    pos = np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[-0.0, 0, 0], [0, 1, 0], [1, 0, 0]]])
    assert cr.adjacency(pos).tolist() == [-1, 4, -1, -1, 1, -1]


def test_ranges_are_clamped_and_miss_records_stay_behind():
    rec, splits, adj = cut(TETRAHEDRON, sr.pack([(0, 0, 1)], [2]))
    padded = np.concatenate([rec, np.repeat(sr.MISS, 2), rec[:2]])          # capacity 5 with two misses, then a truncated range of 2
    slots, chains = cr.chain(adj, padded, [0, 5, 5, 9], total=7)             # ... an empty one between, and the last clamped to total
    assert rows(slots[:5]) == [(0, 0, 3, 1), (2, 0, 3, 1), (1, 0, 3, 1), (3, 3, 1, 10), (4, 4, 1, 10)]
    # records of faces 1 and 2 alone: face 1's neighbour, face 3, is not in the list (3); face 2 -> face 1
    assert rows(slots[5:]) == [(6, 5, 2, cr.LINKED << 1), (5, 5, 2, cr.NOT_LISTED << 1)] and chains.tolist() == [[1, 1], [0, 0], [1, 0]]
    slots, chains = cr.chain(adj, padded, [3, 1, 9], total=4)                # a decreasing pair is empty; [1, 9) is clamped to [1, 4)
    assert rows(slots) == [(int(cr.UNTOUCHED),) * 4, (2, 1, 2, cr.LINKED << 1), (1, 1, 2, cr.NOT_LISTED << 1), (3, 3, 1, cr.MISS << 1)]
    assert chains.tolist() == [[0, 0], [1, 0]]


@pytest.mark.parametrize("name", cs.CPU_NAMES)
def test_the_adjacency_is_an_involution_and_the_chains_partition_every_range(name):
    sc, g = cs.scene(drt, name)
    adj = cr.adjacency(cs.tree_positions(sc))
    has = np.nonzero(adj >= 0)[0]
    assert (adj[adj[has]] == has).all() and (adj[has] != has).all() and ((adj >= -2) & (adj < len(adj))).all()
    planes = cs.planes(name, g)
    rec, counts = sr.whole(g, planes)
    splits = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    slots, chains = cr.chain(adj, rec, splits)
    for i, mine in enumerate(cr.chain_lists(slots, chains, splits)):
        members = sorted(j for m, _ in mine for j in m)
        assert members == list(range(splits[i], splits[i + 1])), (name, i)     # every record in exactly one chain
        for m, closed in mine:
            assert m[0] == min(m) or not closed
    if name in cs.EXACT_CLOSED:
        closed = slots["flags"] & 1
        assert closed.all() and (chains[:, 0] == chains[:, 1]).all() and chains.sum() > 0, name
    print("%s: %d planes, %d records, %d chains, %d closed" % (name, len(planes), len(rec), chains[:, 0].sum(), chains[:, 1].sum()))


def test_the_ring_is_one_closed_chain_of_5000_records():
    sc, g = cs.scene(drt, "ring")
    adj = cr.adjacency(cs.tree_positions(sc))
    assert (adj >= 0).sum() == 2 * cs.RING_QUADS * 2                       # two of a triangle's three edges are shared, the third is a rim
    pl = sr.pack([(0, 0, 1)], [0])
    rec, counts = sr.whole(g, pl)
    assert counts.tolist() == [2 * cs.RING_QUADS]
    slots, chains = cr.chain(adj, rec, [0, len(rec)])
    assert chains.tolist() == [[1, 1]] and (slots["first"] == 0).all() and (slots["length"] == 5000).all() and (slots["flags"] == 1).all()
    assert sorted(slots["seg"].tolist()) == list(range(5000)) and slots["seg"][0] == 0
    assert 2 ** 12 < 5000 <= 2 ** 13                                          # 13 jumping rounds
    order = slots["seg"]
    assert (rec["q"][order] == rec["p"][np.roll(order, -1)]).all()          # exact coordinates: the contour closes bit for bit


def test_hollow_box_areas_have_opposite_signs():
    sc, g = cs.scene(drt, "hollow_box")
    pl = sr.pack([(0, 0, 1)], [0])
    rec, counts = sr.whole(g, pl)
    splits = [0, len(rec)]
    slots, chains = cr.chain(cr.adjacency(cs.tree_positions(sc)), rec, splits)
    area, _ = cr.areas(pl, rec, slots, chains, splits)
    assert chains.tolist() == [[2, 2]] and sorted(area.tolist()) == [-4.0, 16.0] and sr.areas(pl, rec, counts).tolist() == [12.0]
