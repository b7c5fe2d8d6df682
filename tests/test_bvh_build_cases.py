"""The catalogue of tests/bvh_build_cases.py on the CPU: the host builder (drt_scene_build_bvh) against the oracle's builder
(oracle/drt_oracle.c), two restatements of BVHBuilder.cu that share no code.  Where the catalogue says RETURNS both give the same
nodes and the same triangle order; where it says REFUSES both fail and the product's scene keeps the tree and the triangle order
it had.  tests/test_gpu_bvh_build.py then compares the device builder with something already shown to be right.

The second half computes, in numpy from the host's trees, the conditions under which the catalogue meets what it says it meets.

Not reached, by this file or the GPU one: the reference's 512-entry build stack (error bit 2 of finalize_kernel, the second BvhError
of HostScene::build_bvh) and the device builder's kMaxLevels.  A chain peels one triangle per level only with centroids in geometric
progression, and float32's exponent range ends such a chain near 250 levels: 240 are refused by both CPU builders already.
"""
import functools

import numpy as np
import pytest

from tests import bvh_build_cases as bc

drt = pytest.importorskip("dustraytracer_amd")

INT_FIELDS = ("child1", "child2", "prim_count", "prim_start", "is_leaf")


@functools.lru_cache(maxsize=None)
def host_scene(name, leaf, bins):
    """The case built by the host builder (shared by the tests below: nobody changes it)."""
    return bc.build(drt, bc.product_scene(drt, bc.cases()[name].pos), leaf, bins)


def same_floats(a, b):
    """Equal as floats, a NaN equal to a NaN."""
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("entry", bc.entries(bc.RETURNS), ids=bc.entry_id)
def test_host_builder_equals_the_oracle_builder(entry):
    name, leaf, bins, _ = entry
    sc = host_scene(name, leaf, bins)
    osc = bc.oracle_scene(bc.cases()[name].pos).build_bvh(leaf, bins)
    hn, on = sc.m_BVHNodes, osc.nodes
    assert len(hn) == len(on)
    for f in INT_FIELDS:
        assert np.array_equal(hn[f].astype(np.int32), on[f]), f
    assert same_floats(hn["bmin"], on["bmin"]) and same_floats(hn["bmax"], on["bmax"])
    # the triangles were reordered in the same way
    assert sc.m_PrimitivesBuffer["vertex"]["position"].tobytes() == osc.tris["p"].tobytes()
    leaves = hn[hn["is_leaf"] != 0]
    assert leaves["prim_count"].sum() == len(bc.cases()[name].pos) and (len(hn) == 1 or leaves["prim_count"].max() <= max(leaf, 0))


@pytest.mark.parametrize("entry", bc.entries(bc.REFUSES), ids=bc.entry_id)
def test_both_builders_refuse_and_the_scene_keeps_its_tree(entry):
    name, leaf, bins, _ = entry
    pos = bc.cases()[name].pos
    sc = bc.build(drt, bc.product_scene(drt, pos), *bc.a_returning_setting(name))
    nodes, tris, order = sc.m_BVHNodes.tobytes(), sc.m_PrimitivesBuffer.tobytes(), sc.triangleOrder().tobytes()
    assert len(nodes) > 0
    with pytest.raises(drt.DrtError) as e:
        bc.build(drt, sc, leaf, bins)
    assert e.value.code == drt.ERR_BVH
    with pytest.raises(RuntimeError):
        bc.oracle_scene(pos).build_bvh(leaf, bins)
    assert sc.m_BVHNodes.tobytes() == nodes and sc.m_PrimitivesBuffer.tobytes() == tris and sc.triangleOrder().tobytes() == order


def test_every_case_has_a_setting_that_returns_and_a_catalogue_of_the_stated_size():
    for c in bc.cases().values():
        assert any(r for _, _, r in c.settings), c.name
        assert 2 <= len(c.pos) <= 2048, c.name
    assert len(bc.cases()["hostile_x4"].pos) == 1440                       # three chunks of 512
    assert len(bc.entries(bc.REFUSES)) >= 20 and len(bc.entries(bc.RETURNS)) >= 50


# ---------------------------------------------------------------- what the catalogue meets

def _bounds(nodes):
    return np.concatenate([nodes["bmin"], nodes["bmax"]], axis=1)


def _split_nodes(nodes):
    """(prim_count, level) of the nodes that were split, and which of them is the root."""
    split = nodes["is_leaf"] == 0
    return nodes["prim_count"][split], bc.levels(nodes)[split], (np.arange(len(nodes)) == len(nodes) - 1)[split]


def test_zeros_and_flat_have_negative_zero_bounds():
    for name in ("zeros", "flat"):
        assert bc.negative_zero_bounds(host_scene(name, 4, 8).m_BVHNodes) >= 100, name


def test_one_inf_has_a_bound_that_is_not_finite_and_nan_has_none():
    for leaf, bins in ((4, 8), (20, 8)):
        assert not np.isfinite(_bounds(host_scene("one_inf", leaf, bins).m_BVHNodes)).all()
        assert np.isfinite(_bounds(host_scene("nan", leaf, bins).m_BVHNodes)).all()        # every NaN was skipped
    assert np.isnan(bc.cases()["nan"].pos).sum() == 20


def test_axis_has_only_boxes_of_zero_area():
    for leaf, bins in ((4, 8), (1, 2), (1, 3)):
        n = host_scene("axis", leaf, bins).m_BVHNodes
        d = n["bmax"] - n["bmin"]
        assert len(n) > 600 and ((2 * d[:, 2] * d[:, 1] + 2 * d[:, 2] * d[:, 0] + 2 * d[:, 0] * d[:, 1]) == 0).all()       # Bounds.cu:4-10
    n = host_scene("line", 4, 8).m_BVHNodes
    assert ((n["bmax"] - n["bmin"]) > 0).all(axis=1).any()                 # the line's boxes are not flat


def test_a_level_has_more_than_64_split_nodes():
    """decide_kernel has one thread per split node of a level and 64 threads per block."""
    widest = {}
    for name, leaf, bins in (("asc", 1, 2), ("desc", 1, 32), ("hostile_x4", 2, 16), ("soup1025", 1, 3)):
        _, level, _ = _split_nodes(host_scene(name, leaf, bins).m_BVHNodes)
        widest[name] = int(np.bincount(level).max())
    assert widest["asc"] == 1024 and min(widest.values()) > 64, widest


def test_interior_nodes_at_the_chunk_edges():
    """Nodes below the root of more than 512 triangles, of exactly 512 and of exactly 1 024 (one wave bins 512)."""
    for name in ("asc", "desc"):
        for leaf, bins in ((1, 2), (4, 8)):
            count, _, root = _split_nodes(host_scene(name, leaf, bins).m_BVHNodes)
            below = count[~root]
            assert (below == 1024).sum() == 2 and (below == 512).sum() == 4 and (below > 512).any(), (name, leaf, bins)
    count, _, root = _split_nodes(host_scene("hostile_x4", 4, 8).m_BVHNodes)
    assert ((count[~root] > 512) & (count[~root] % 512 != 0)).any()       # and one that ends inside a chunk


def test_the_chains_are_deep_and_only_the_right_one_fills_the_stack():
    for name in ("chain_left", "chain_right"):
        sc = host_scene(name, 1, 2)
        n = sc.m_BVHNodes
        assert len(n) == 2 * bc.CHAIN - 1 and bc.levels(n).max() == bc.CHAIN - 1 >= 100 and sc.bvh_depth == bc.CHAIN
        # the big child of every split node: the left one in chain_left, the right one in chain_right
        split = n[n["is_leaf"] == 0]
        big = n["prim_count"][split["child1"]] > n["prim_count"][split["child2"]]
        assert (big[split["prim_count"] > 2] == (name == "chain_left")).all(), name


def _root_swaps(name, leaf, bins):
    """What std::partition swaps at the root: the elements among the first n_left in load order that fail the predicate, which
    are those the tree does not have in the root's left child."""
    sc = host_scene(name, leaf, bins)
    n = sc.m_BVHNodes
    left = n[int(n[-1]["child1"])]
    assert left["prim_start"] == 0
    n_left = int(left["prim_count"])
    in_left = np.zeros(len(bc.cases()[name].pos), bool)
    in_left[sc.triangleOrder()[:n_left]] = True
    return int((~in_left[:n_left]).sum())


def test_the_root_partition_of_desc_swaps_across_chunks_and_that_of_asc_swaps_nothing():
    for leaf, bins in ((1, 2), (4, 8), (1, 32)):
        assert _root_swaps("desc", leaf, bins) > 512, (leaf, bins)
        assert _root_swaps("asc", leaf, bins) == 0, (leaf, bins)
    assert _root_swaps("desc", 1, 2) == 1024
    assert 0 < _root_swaps("soup1025", 1, 3) < 512                          # an ordinary partition, for comparison
    # no swap anywhere in asc: the triangles are still in load order
    for leaf, bins in ((1, 2), (4, 8), (1, 32)):
        assert (host_scene("asc", leaf, bins).triangleOrder() == np.arange(2048)).all()


def _centroids_on_planes(sc, bins):
    """Per axis: the number of (split node, candidate plane) pairs in which a centroid of the node equals the plane bit for bit
    (the planes as BVHBuilder.cu:275-279 computes them, in float32)."""
    n, tris = sc.m_BVHNodes, sc.m_PrimitivesBuffer
    on = np.zeros(3, np.int64)
    for node in n[n["is_leaf"] == 0]:
        s, c = int(node["prim_start"]), int(node["prim_count"])
        p = tris["vertex"]["position"][s:s + c].reshape(-1, 3)
        lo, hi = p.min(axis=0), p.max(axis=0)
        delta = ((hi - lo) / np.float32(bins)).astype(np.float32)
        for i in range(1, bins):
            plane = (lo + (np.float32(i) * delta).astype(np.float32)).astype(np.float32)
            on += (tris["centroid"][s:s + c].view(np.uint32) == plane.view(np.uint32)[None, :]).any(axis=0)
    return on


def test_centroids_of_asc_lie_exactly_on_candidate_planes():
    """`c < plane` is false there: the triangle goes right."""
    for leaf, bins in ((1, 2), (4, 8), (1, 32)):
        on = _centroids_on_planes(host_scene("asc", leaf, bins), bins)
        n_split = int((host_scene("asc", leaf, bins).m_BVHNodes["is_leaf"] == 0).sum())
        assert on[1] == n_split, (leaf, bins, on)                           # y: -0.25 + (bins / 2) * (0.5 / bins) = 0, every centroid's y
    assert _centroids_on_planes(host_scene("asc", 1, 32), 32)[0] > 0        # and on x, the axis that is split


def test_where_the_scaled_cases_are_refused():
    """(n - 1, 8) splits the root and nothing else.  It returns where the catalogue says that the refusal of (4, 8) comes from a
    node below the root, and is refused where the catalogue says that the root's own partition fails."""
    n = len(bc.cases()["hostile_x4"].pos)
    for k in bc.SCALES_REFUSED_BELOW_THE_ROOT:
        c = bc.cases()["hostile_x4_scaled(%d)" % k]
        assert (4, 8, bc.REFUSES) in c.settings and (n - 1, 8, bc.RETURNS) in c.settings
        assert len(host_scene(c.name, n - 1, 8).m_BVHNodes) == 3
    assert len(host_scene("hostile_x4_scaled(-78)", 700, 8).m_BVHNodes) == 9                 # three levels down
    for k in bc.SCALES_REFUSED_AT_THE_ROOT:
        c = bc.cases()["hostile_x4_scaled(%d)" % k]
        assert (4, 8, bc.REFUSES) in c.settings and (n - 1, 8, bc.REFUSES) in c.settings
    for name in ("many_inf", "many_minus_inf"):
        assert (4, 8, bc.REFUSES) in bc.cases()[name].settings
    assert len(host_scene("many_inf", 1499, 8).m_BVHNodes) == 3             # many_inf is refused below the root as well
    for k in bc.SCALES_IN_RANGE:
        assert len(host_scene("hostile_x4_scaled(%d)" % k, 4, 8).m_BVHNodes) == 961
    # the areas at 2^-72 are subnormal: the root's is, and so is every other
    nodes = host_scene("hostile_x4_scaled(-72)", 4, 8).m_BVHNodes
    d = (nodes["bmax"] - nodes["bmin"]).astype(np.float32)
    area = (2 * d[:, 2] * d[:, 1] + 2 * d[:, 2] * d[:, 0] + 2 * d[:, 0] * d[:, 1]).astype(np.float32)
    assert 0 < area[-1] < np.finfo(np.float32).tiny and (area < np.finfo(np.float32).tiny).all()


def test_wide_and_tiny_settings():
    assert len(host_scene("soup1500", 4, 256).m_BVHNodes) == 979 and len(host_scene("soup1500", 1499, 2).m_BVHNodes) == 3
    assert [len(host_scene("soup%d" % n, 1, 3).m_BVHNodes) for n in bc.SIZES] == [2 * n - 1 for n in bc.SIZES]
