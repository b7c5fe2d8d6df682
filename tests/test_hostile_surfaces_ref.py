"""The catalogue of tests/hostile_surfaces.py on the restatements alone (CPU only, no product library): that the capped meshes are what
they say, that the cuts, curves, contours and topology of tests/test_gpu_hostile_surfaces.py meet the hard cases -- every exit status
from geometry, ties in the interval test, vertices exactly on a query's plane, rotations that end on a -2 edge -- and in which range
of scales the intersection records keep, lose and have lost their digits.  The counts pinned here are what the restatements give."""
import numpy as np
import pytest

from tests import contour_ref as cr
from tests import curve_ref as cu
from tests import hostile_meshes as hm
from tests import hostile_surfaces as hs
from tests import topology_ref as tr
from tests.test_hostile_meshes_ref import OUT_OF_RANGE, SEED

FULL = ("plain", "offset", "scaled(20)", "scaled(-20)")

# Intersection records left at each scale 2^k, per mesh (of the plain count, first).  Inside 2^-24 .. 2^32 nothing changes
# (tests/test_intersect_ref.py); in the fringe records are lost one by one -- going down nq, nt and D = cross(nq, nt), a fourth power of
# the lengths, pass through the subnormals to zero, going up they overflow to infinities and the NaNs of inf - inf; out of range little or
# nothing is left.  The band's coordinates reach 16 and its tool triangles 150, the spheres' 1.3: their ranges are shifted accordingly.
RECORDS = {"capped_sparse": (857, {-32: 770, -36: 0, 36: 602, 42: 426, -40: 0, 50: 0}),
           "capped_dense": (1684, {-32: 1436, -36: 0, 36: 1285, 42: 744, -40: 0, 50: 1}),
           "capped_band": (2521, {-32: 2521, -36: 2420, 36: 2521, 42: 794, -40: 1714, 50: 0}),
           "soup": (229, {-32: 213, -36: 68, 36: 161, 42: 125, -40: 0, 50: 4})}
# shells, open half-edges, bad half-edges
TOPOLOGY = {("soup", "plain"): [345, 858, 192], ("soup", "offset"): [345, 846, 196], ("capped_sparse", "plain"): [1, 0, 0],
            ("capped_dense", "plain"): [22, 77, 159], ("capped_band", "plain"): [1, 800, 0]}


def test_the_constants_are_the_hostile_meshes():
    assert hs.SEED == SEED and hs.OUT_OF_RANGE == OUT_OF_RANGE


@pytest.mark.parametrize("variant", FULL)
def test_capped_sparse_is_one_watertight_shell(variant):
    c = hs.case("capped_sparse", variant)
    A = hs.restate(c, ("topology",))
    assert A["counts"].tolist() == [1, 0, 0] and len(A["loops"][0]) == 0
    flat = hs.zero_area(c.tree)
    print("capped_sparse %s: %d caps, %d of exactly zero area" % (variant, c.is_cap.sum(), flat[c.is_cap].sum()))
    assert c.is_cap.sum() == 24 and not flat[~c.is_cap].any() and flat[c.is_cap].sum() >= 1
    if variant != "offset":                                                    # (moved and rounded, nearly every cap is a sliver)
        made = hs.mesh("capped_sparse")
        assert made.exact.sum() == flat[c.is_cap].sum() >= 1 and (~made.exact).sum() >= 10


def test_capped_dense_falls_apart_and_its_holes_rotate_into_bad_edges():
    c = hs.case("capped_dense", "plain")
    A = hs.restate(c, ("topology",))
    assert A["counts"][0] > 1 and A["counts"][2] >= 50 and A["counts"][1] > 0
    adj = A["adj"]
    ends = [tr.successor(adj, h) for h in np.nonzero(adj == -1)[0]]
    bad = sorted(steps for _, why, steps in ends if why == cr.NON_MANIFOLD)
    good = max(steps for _, why, steps in ends if why == cr.LINKED)
    print("capped_dense: rotations of %d boundary half-edges; %d end on a -2 edge, after %r steps; the longest that ends on a boundary takes %d" % (len(ends), len(bad), bad, good))
    assert sum(1 for s in bad if s >= 1) >= 3 and bad[-1] >= 29 and good >= 5   # a -2 edge deep inside the rotation round a pole
    assert ((A["loops"][0]["flags"] >> 1) == cr.NON_MANIFOLD).sum() == len(bad) and A["loops"][1][2] < A["loops"][1][1]


def test_every_exit_status_comes_from_geometry():
    contour, curve, on_caps, into_caps = {}, {}, np.zeros(6, np.int64), 0
    for name in hs.MESHES:
        for variant in ("plain", "offset"):
            c = hs.case(name, variant)
            A = hs.restate(c, ("curve", "contour"))
            contour[name, variant], curve[name, variant] = hs.contour_status(c), hs.curve_status(c)
            print("%s %s: contour statuses %s, curve statuses %s" % (name, variant, contour[name, variant].tolist(), curve[name, variant].tolist()))
            if name != "soup":
                slots, (splits, rec) = A["curve"][0], A["cut"]
                w = rec.view(np.int32)
                prim, cq, status = w[slots["seg"], 3], w[slots["seg"], 7] >> 4, slots["flags"] >> 1
                on_caps += np.bincount(status[c.is_cap[prim]], minlength=6)
                # a record that leaves through a scene edge whose twin is a cap of exactly zero area: the cap has no record (its nt is
                # zero, so the query's three vertices are in one class), and the curve ends there as "not listed"
                leaves = cq < 4
                twin = A["adj"][3 * prim[leaves] + cq[leaves]]
                flat = (twin >= 0) & (c.is_cap & hs.zero_area(c.tree))[np.maximum(twin, 0) // 3]
                assert (status[leaves][flat] == cu.NOT_LISTED).all()
                into_caps += int(flat.sum())
    total = lambda table, names: sum(table[k] for k in table if k[0] in names)
    assert (total(contour, hs.MESHES) > 0).all() and (total(curve, hs.MESHES) > 0).all()
    capped = total(curve, hs.CAPPED_MESHES)
    assert (capped[[0, 2, 3, 4]] > 0).all() and curve["soup", "plain"][1] > 0 and curve["soup", "offset"][1] > 0
    # statuses 3 and 4: from offset variants, on the caps themselves (slivers: they have records) and at the exactly flat ones
    assert all(curve[name, "offset"][3] > 0 and curve[name, "offset"][4] > 0 for name in hs.CAPPED_MESHES) and curve["soup", "offset"][4] > 0
    print("curve statuses of records ON caps %s; records that leave into an exactly flat cap: %d" % (on_caps[:5].tolist(), into_caps))
    assert on_caps[3] > 0 and on_caps[4] > 0 and into_caps >= 10
    plain = contour["capped_sparse", "plain"] + contour["capped_dense", "plain"]
    assert plain[3] >= 4 and plain[4] >= 2 and contour["capped_sparse", "plain"][4] > 0 and contour["capped_dense", "plain"][2] >= 50


@pytest.mark.parametrize("variant", ["plain", "offset"])
def test_the_band_s_sections_close_through_zero_length_records(variant):
    """drt.h, "section contours": the successor of a record is an integer question -- prim, code and the adjacency -- and no
    coordinate is compared.  A cap (a, b, m) with a at z = -1, b at z = +1 and m = (a + b) / 2 is cut by every plane z = h, -1 < h < 1
    (at h = 0, s(m) = 0 counts as above): its apex is alone in its class, both cut points lie on the line a b at height h, and with
    the band's exact coordinates they are the same bits: a record of zero length, P = Q.  It is entered through one of the cap's
    edges and left through another like any record, and the halves (a, m, c), (m, b, c) and the neighbour across a b classify a, b
    and m as the cap does, so each is left and entered through the twin edge: the chain is CLOSED THROUGH the zero-length records, not
    broken at the caps.  In a band of one row every level crosses every cap; the level through the midpoints is h = 0."""
    c = hs.case("capped_band", variant)
    A = hs.restate(c, ("contour",))
    rec, totals = A["section"]
    slots, chains = A["contour"]
    splits = np.concatenate([[0], np.cumsum(totals.astype(np.int64))])
    caps = int(c.is_cap.sum())
    assert caps == 120 and hs.zero_area(c.tree)[c.is_cap].all()
    for i in range(5):                                                         # z = 0, 0.5, -0.25, and two with the normal reversed
        mine = slice(splits[i], splits[i + 1])
        r = rec[mine]
        flat = (r["p"] == r["q"]).all(axis=1)
        assert chains[i].tolist() == [1, 1] and (slots["flags"][mine] == 1).all(), (variant, i)
        assert c.is_cap[r["prim"]].sum() == caps and flat[c.is_cap[r["prim"]]].all(), (variant, i)
        assert totals[i] >= 2 * hs.BAND_QUADS + caps
    areas, mass = A["areas"]
    assert (np.abs(areas[:5] - np.pi * 256) < 0.1).all()                       # a 400-gon of radius 16, whichever way the normal points
    # ... while the tool triangle in the plane z = 0 gets no record from a cap at all, and its curve breaks at every one
    splits, cut = A["cut"] if "cut" in A else hs.restate(c, ("cut",))["cut"]
    big = cut.view(np.int32)[:splits[1]]
    assert len(big) > hs.BAND_QUADS and not c.is_cap[big[:, 3]].any()
    chains = [ch for ch in cu.chain_lists(hs.restate(c, ("curve",))["curve"][0]) if ch[0][0] < splits[1]]
    assert len(chains) >= caps and not any(closed for _, closed, _ in chains)


def test_the_tool_curve_on_capped_sparse():
    """Plain: the 24 caps lie off the tool sphere's curve, which stays the one closed loop of tests/test_curve_ref.py.  Offset by
    (4096, -8192, 16384) neighbouring triangles no longer agree on the side of a shared vertex, and the loop falls into open chains that
    end with status 4."""
    found = {}
    for variant in ("plain", "offset"):
        c = hs.case("capped_sparse", variant)
        A = hs.restate(c, ("curve",))
        tool = int(A["cut"][0][c.q.n_tool])
        found[variant] = [(len(m), closed, status[-1]) for m, closed, status in cu.chain_lists(A["curve"][0]) if m[0] < tool]
        print("capped_sparse %s: the tool mesh's chains (records, closed, last exit status): %r" % (variant, found[variant]))
    assert found["plain"] == [(186, True, cu.LINKED)]
    assert found["offset"] == [(58, False, cu.OTHER_EDGES), (123, False, cu.OTHER_EDGES), (8, False, cu.OTHER_EDGES)]


@pytest.mark.parametrize("name", hs.CAPPED_MESHES)
@pytest.mark.parametrize("variant", ["plain", "offset"])
def test_the_aimed_triangles_meet_ties(name, variant):
    endpoint, tied, on_plane = hs.ties(hs.case(name, variant))
    print("%s %s: aimed records with a query-edge endpoint %d, tied on the interval axis %d, with a scene vertex on the query's plane %d" % (name, variant, endpoint, tied, on_plane))
    assert endpoint >= 20 and tied >= 10 and on_plane >= 10


def _same_tree(a, b):
    return all((a.osc.nodes[f] == b.osc.nodes[f]).all() for f in ("is_leaf", "child1", "child2", "prim_start", "prim_count"))


@pytest.mark.parametrize("name", hs.MESHES)
def test_scaling_by_2_to_the_20_changes_nothing(name):
    plain = hs.case(name, "plain")
    A = hs.restate(plain, ("cut", "curve", "section", "contour", "topology"))
    assert len(A["cut"][1]) == RECORDS[name][0]
    for k in (20, -20):
        c = hs.case(name, "scaled(%d)" % k)
        assert _same_tree(plain, c)
        B = hs.restate(c, ("cut", "curve", "section", "contour", "topology"))
        assert (A["cut"][0] == B["cut"][0]).all() and hm.differing((hs.scaled_records(A["cut"][1], k),), (B["cut"][1],)) == 0
        assert (A["section"][1] == B["section"][1]).all()
        assert hm.differing((hs.scaled_records(A["section"][0], k),), (B["section"][0].view(np.float32).reshape(-1, 8),)) == 0
        assert (A["adj"] == B["adj"]).all() and (A["query_adj"] == B["query_adj"]).all() and (A["labels"] == B["labels"]).all()
        for kind in ("loops", "curve", "contour"):
            assert A[kind][0].tobytes() == B[kind][0].tobytes() and (A[kind][1] == B[kind][1]).all(), (name, k, kind)


@pytest.mark.parametrize("name", hs.MESHES)
def test_the_fringe_scales_lose_some_records_and_the_far_ones_nearly_all(name):
    plain = hs.case(name, "plain")
    total, pinned = RECORDS[name]
    sec = hs.restate(plain, ("section",))["section"]
    left = {}
    for k in hs.FRINGE + hs.OUT_OF_RANGE:
        c = hs.case(name, "scaled(%d)" % k)
        assert _same_tree(plain, c)
        left[k] = len(hs.restate(c, ("cut",))["cut"][1])
        if k in hs.OUT_OF_RANGE:                                               # plane sections are linear in the lengths: unchanged even there
            B = hs.restate(c, ("section",))
            assert (sec[1] == B["section"][1]).all() and hm.differing((hs.scaled_records(sec[0], k),), (B["section"][0].view(np.float32).reshape(-1, 8),)) == 0
    print("%s: intersection records left of %d at 2^k: %r" % (name, total, left))
    assert left == pinned
    if name == "soup":
        assert all(0 < left[k] < total for k in hs.FRINGE)
    assert any(0 < left[k] < total for k in hs.FRINGE) and all(left[k] < total for k in hs.OUT_OF_RANGE)


def test_the_offset_merges_vertices_of_the_soup_and_the_count_triples():
    plain, off = hs.case("soup", "plain"), hs.case("soup", "offset")
    A, B = hs.restate(plain, ("topology",)), hs.restate(off, ("topology",))
    assert (A["adj"] != B["adj"]).any()                      # the needles' vertices 2^-12 apart are one position at 16384
    for (name, variant), want in TOPOLOGY.items():
        assert hs.restate(hs.case(name, variant), ("topology",))["counts"].tolist() == want, (name, variant)


def test_the_refit_positions_change_every_table():
    c = hs.case("capped_sparse", "plain")
    new = hs.collapsed(c)
    assert new.shape == c.pos.shape and hs.zero_area(new).sum() >= hs.zero_area(c.pos).sum() + 20
    A = hs.restate(c, ("topology",))
    adj = cr.adjacency(new)                                  # (load order here; the GPU test restates the refitted tree)
    assert (adj != cr.adjacency(c.pos)).sum() >= 60 and (adj == -2).sum() >= 20 and tr.counts(adj, tr.labels(adj)).tolist() != A["counts"].tolist()
