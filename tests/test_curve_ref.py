"""What the restatement of the intersection curves (tests/curve_ref.py) does, on the CPU: the records are intersect_ref's float32
restatement of drt_renderer_intersect_triangles on the meshes of tests/curve_scenes.py, the scene's table is the product's host table
(tests/test_contour_abi.py compares that one with a dictionary), and the walk is sequential."""
import numpy as np
import pytest

from tests import contour_scenes as cs
from tests import curve_ref as cu
from tests import curve_scenes as cv
from tests import intersect_ref as ir
from tests import nearest_ref as nr

drt = pytest.importorskip("dustraytracer_amd")

_made = {}


def made(name):
    """(adj, query_adj, prim, code, splits, n_tris, slots, counts) of a case, worked out once."""
    if name not in _made:
        pos, tris = cv.case(name)
        sc, osc = cs.flat_scene(drt, pos)
        g = nr.from_oracle(osc)
        splits, rec = ir.whole(g, tris)
        words = rec.view(np.int32)
        adj, query_adj = sc.edgeAdjacency().reshape(-1), cu.tri_adjacency(tris)
        prim, code = words[:, 3].copy(), words[:, 7].copy()
        _made[name] = (adj, query_adj, prim, code, splits, len(g.v0)) + cu.chain(adj, query_adj, prim, code, splits, len(g.v0))
    return _made[name]


def check_simple(slots, succ_of=None):
    """Every record stands in exactly one slot, the chains tile the positions, and every index is in range."""
    total = len(slots)
    assert sorted(int(s) for s in slots["seg"]) == list(range(total))
    pos = 0
    while pos < total:
        length = int(slots["length"][pos])
        assert length >= 1 and pos + length <= total and (slots["first"][pos:pos + length] == pos).all()
        pos += length
    assert pos == total


@pytest.mark.parametrize("name", cv.NAMES[:12])
def test_the_link_is_injective_and_the_chains_are_simple(name):
    adj, query_adj, prim, code, splits, n_tris, slots, counts = made(name)
    succ, status = cu.links(adj, query_adj, prim, code, splits, len(prim), n_tris)
    assert len(set(succ.values())) == len(succ), name                      # no two records claim the same successor
    assert set(succ) | set(status) == set(range(len(prim))) and not set(succ) & set(status)
    check_simple(slots)
    chains = cu.chain_lists(slots)
    assert counts[0] == len(chains) and counts[1] == sum(closed for _, closed, _ in chains) and counts[2] == 0
    for members, closed, status in chains:
        assert all(s == cu.LINKED for s in status[:-1]) and (status[-1] == cu.LINKED) == closed
        assert not closed or members[0] == min(members)                    # a cycle starts at its smallest index


@pytest.mark.parametrize("seed", cv.SPHERE_SEEDS)
def test_general_position_gives_one_closed_loop(seed):
    adj, query_adj, prim, code, splits, n_tris, slots, counts = made("spheres%d" % seed)
    assert 90 <= len(prim) <= 260
    assert counts.tolist() == [1, 1, 0]
    (members, closed, status), = cu.chain_lists(slots)
    assert closed and set(status) == {cu.LINKED} and len(members) == len(prim)
    # the owning query changes exactly at the exits through a query edge
    query = np.searchsorted(splits[1:], members, side="right")
    cq = code[members] >> 4
    changes = query != np.roll(query, -1)
    assert (changes == (cq >= 4)).all() and 0 < changes.sum() < len(members)
    # and the scene triangle exactly at the others
    assert ((prim[members] != np.roll(prim[members], -1)) == (cq < 4)).all()


@pytest.mark.parametrize("name", ["aligned_x", "aligned_z"])
def test_a_curve_through_vertices_and_along_edges_falls_into_open_chains(name):
    _, _, prim, code, splits, _, slots, counts = made(name)
    status = set((slots["flags"] >> 1).tolist())
    assert cu.NOT_LISTED in status and cu.OTHER_EDGES in status and cu.LINKED in status
    assert counts[0] > 1 and counts[1] < counts[0]
    print("%s: %d records, %d chains, %d closed" % (name, len(prim), counts[0], counts[1]))


def test_the_tube_is_one_loop_and_two_queries_share_it():
    _, _, prim, code, _, _, slots, counts = made("tube127")
    assert len(prim) == 254 and counts.tolist() == [1, 1, 0] and (code >> 4 < 4).all()
    _, _, prim, code, splits, _, slots, counts = made("tube_quad")
    assert counts.tolist() == [1, 1, 0] and len(prim) == 258 and 0 < splits[1] < splits[2] == 258
    (members, _, _), = cu.chain_lists(slots)
    query = np.searchsorted(splits[1:], members, side="right")
    assert (query != np.roll(query, -1)).sum() == 2                        # the loop changes query twice


def test_open_meshes_end_at_their_boundaries():
    _, _, prim, code, _, _, slots, counts = made("strip")                  # the scene is open: the curve leaves it through a boundary edge
    assert counts.tolist() == [1, 0, 0] and len(prim) == 4
    last = slots[-1]
    assert last["flags"] >> 1 == cu.BOUNDARY and code[last["seg"]] >> 4 < 4
    _, _, prim, code, _, _, slots, counts = made("poke")                   # the query is open: the curve leaves it through a query edge
    assert counts.tolist() == [1, 0, 0]
    last = slots[-1]
    assert last["flags"] >> 1 == cu.BOUNDARY and code[last["seg"]] >> 4 >= 4
    for name, total in (("single", 1), ("quad", 2)):
        _, _, prim, code, _, _, slots, counts = made(name)
        assert len(prim) == total and counts.tolist() == [1, 0, 0] and slots[-1]["flags"] >> 1 == cu.BOUNDARY


def test_non_manifold_and_flipped_edges_end_a_chain():
    _, _, prim, code, _, _, slots, counts = made("book")                   # three leaves on one edge
    assert len(prim) == 3 and cu.NON_MANIFOLD in (slots["flags"] >> 1).tolist() and counts[1] == 0
    adj, query_adj, prim, code, splits, _, slots, counts = made("tube_flipped")
    assert (query_adj.reshape(2, 3) == -2).sum() == 2                      # the diagonal runs the same way twice
    ends = [(int(s["seg"]), int(s["flags"]) >> 1) for s in slots if s["flags"] >> 1 != cu.LINKED]
    assert len(ends) == 2 and all(status == cu.NON_MANIFOLD and code[j] >> 4 >= 4 for j, status in ends) and counts.tolist() == [2, 0, 0]


def test_broken_input_still_gives_simple_paths():
    adj, query_adj, prim, code, splits, n_tris, want, _ = made("tube_quad")
    # a query table that is no involution: both queries' edges all name the same half-edge
    bad = np.full_like(query_adj, 3)
    slots, counts = cu.chain(adj, bad, prim, code, splits, n_tris)
    check_simple(slots)
    assert slots.tobytes() != want.tobytes() and counts[0] >= 1
    # values that name no query
    slots, _ = cu.chain(adj, np.full_like(query_adj, 3 * 2), prim, code, splits, n_tris)
    check_simple(slots)
    assert (slots["flags"] >> 1 == cu.NON_MANIFOLD).sum() == (code >> 4 >= 4).sum() == 2      # a / 3 >= n is treated as -2: the exits through the diagonal
    # a prim twice in a range: two records claim the same successor, the smallest keeps it
    twice = prim.copy()
    twice[5] = twice[4]
    slots, counts = cu.chain(adj, query_adj, twice, code, splits, n_tris)
    check_simple(slots)
    assert cu.NOT_LISTED in (slots["flags"] >> 1).tolist() or cu.OTHER_EDGES in (slots["flags"] >> 1).tolist()
    # records that are not live: a bad code digit, a prim beyond the mesh, a miss record, a record outside every range
    dead_prim, dead_code = prim.copy(), code.copy()
    dead_code[7], dead_code[8], dead_prim[9], dead_prim[splits[1] - 1] = 3, 7 << 4, n_tris, -1
    cut = np.asarray([0, splits[1], splits[2] - 3])
    slots, counts = cu.chain(adj, query_adj, dead_prim, dead_code, cut, n_tris)
    check_simple(slots)
    dead = slots[slots["flags"] >> 1 == cu.NOT_LIVE]
    assert sorted(dead["seg"].tolist()) == [7, 8, 9, int(splits[1]) - 1, 255, 256, 257] and (dead["length"] == 1).all() and counts[2] == 7
    # a record that is not live stands where its index puts it among the chains' first records
    firsts = slots["seg"][slots["first"] == np.arange(len(slots))]
    assert (np.diff(firsts.astype(np.int64)) > 0).all()


def test_the_owner_is_the_search_the_header_writes_out():
    splits = np.asarray([0, 15, 8, 20])
    owners = [cu.owner_of(splits, 18, j) for j in range(20)]
    assert owners[:15] == [0] * 15 and owners[15:18] == [2] * 3 and owners[18:] == [None, None]
    assert [cu.owner_of(np.asarray([4, 2, 6]), 10, j) for j in range(7)] == [None, None, 1, 1, 1, 1, None]


def test_the_query_table_is_the_scene_s_rule():
    """tri_adjacency on a scene's own triangles in tree order is the product's host table (which test_contour_abi.py pins)."""
    for name in ("spheres1", "book", "strip"):
        sc, _ = cs.flat_scene(drt, cv.case(name)[0])
        assert cu.tri_adjacency(cs.tree_positions(sc)).tobytes() == sc.edgeAdjacency().tobytes()
