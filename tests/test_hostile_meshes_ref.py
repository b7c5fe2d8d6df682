"""The query rules of include/drt.h on meshes that are not well behaved (tests/hostile_meshes.py), on the restatements alone (CPU
only): hand cases on a segment, a point and a v0 = v1 triangle; on the degenerate and the offset mesh each restatement against its
own all-triangles answer and against float64; the conditions under which tests/test_gpu_hostile_meshes.py meets the hard cases; and
the range of scales in which the rules work -- what the "working range" paragraph of include/drt.h states."""
import numpy as np
import pytest

import oracle
from tests import hostile_meshes as hm
from tests import inside_ref as ir
from tests import near_list_ref as nl
from tests import nearest_ref as nr
from tests import overlap_ref as ov
from tests import section_ref as sr
from tests import sweep_ref as sw
from tests import test_sweep_ref as tsr
from tests import tri_overlap_ref as tv

SEED = 11


def _run(kind, sc, g, *a):
    if kind == "nearest":
        return nr.nearest(g, *a)
    if kind == "cast":
        return sw.sphere_cast(g, *a)
    if kind == "boxes":
        return ov.overlap(g, a[0], 0)[1]
    if kind == "tris":
        return tv.overlap(g, a[0], 0)[1]
    return sr.whole(g, a[0])


def test_hand_cases_on_a_segment_a_point_and_a_triangle_beside_a_zero_area_one():
    """Every value is derived in the comments of tests/hostile_meshes.py from the header's text."""
    hm.check_hand_cases(lambda name: (None, nr.from_triangles(hm.HAND_SCENES[name], np.tile(np.float32([0, 0, 1]), (len(hm.HAND_SCENES[name]), 1)))), _run)


class Case:
    def __init__(self, name):
        self.name = name
        self.mesh = hm.degenerate() if name == "degenerate" else hm.offset(hm.degenerate())
        self.osc = hm.oracle_scene(self.mesh)
        self.g = nr.from_oracle(self.osc)
        self.kind, self.twin = hm.kinds_in_tree_order(self.osc, self.mesh)
        self.q = hm.queries(self.g, self.osc, self.kind, self.twin, SEED)
        self.answers = hm.restate(self.g, self.osc, self.q)
        # (moved and rounded, a collinear triple is a sliver: on the offset mesh it has a normal and a side)
        self.zero_area = np.isin(self.kind, hm.ZERO_AREA) & ((self.kind != hm.COLLINEAR) | (name == "degenerate"))


_cases = {}


def _case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


@pytest.fixture(scope="module", params=["degenerate", "offset"])
def case(request):
    return _case(request.param)


def test_the_mesh_is_what_it_says(case):
    g, kind = case.g, case.kind
    assert len(g.v0) == 360 and len(g.bmin) >= 200 and oracle.tree_depth(case.osc.nodes) >= 10
    cross = np.cross(g.e1.astype(np.float64), g.e2.astype(np.float64))
    assert (cross[case.zero_area] == 0).all() and (np.bincount(kind[case.zero_area], minlength=6)[1:6] == [5, 5, 5, 5 * (case.name == "degenerate"), 4]).all()
    assert (case.twin >= 0).sum() == 40 and (case.twin[case.twin[case.twin >= 0]] == np.nonzero(case.twin >= 0)[0]).all()
    # degenerate triangles share leaves with real ones
    leaf_of = np.repeat(np.nonzero(g.is_leaf)[0], g.count[g.is_leaf])[np.argsort(np.concatenate([np.arange(s, s + c) for s, c in zip(g.start[g.is_leaf], g.count[g.is_leaf])]))]
    mixed = sum(1 for leaf in set(leaf_of[case.zero_area].tolist()) if (~case.zero_area[leaf_of == leaf]).any())
    print("%s: %d triangles %r, %d nodes, depth %d, %d leaves hold zero-area and real triangles" % (case.name, len(g.v0), np.bincount(kind).tolist(), len(g.bmin),
                                                                                                  oracle.tree_depth(case.osc.nodes), mixed))
    assert mixed >= 10


def test_each_tree_answer_is_its_float32_all_triangles_answer(case):
    g, osc, q, A = case.g, case.osc, case.q, case.answers
    n = len(q.points)
    best, prim = nr.brute_force(g, q.points)
    best_r, _ = nr.brute_force(g, q.points, q.radius)
    d = {"nearest": int((A["nearest"][1].view(np.uint32) != best.view(np.uint32)).sum()), "nearest_r": int((A["nearest_r"][1].view(np.uint32) != best_r.view(np.uint32)).sum())}
    slots, counts, _ = nl.brute_force(g, q.points, np.inf, hm.K_NEAR, nl.K)
    d["k_nearest"] = int(nl.differing_points(nl.Slots(*A["k_nearest"][:6]), slots, np.full(n, hm.K_NEAR)).sum()) + int((counts != A["k_nearest"][6]).sum())
    totals = A["within"][6]
    slots, counts, _ = nl.brute_force(g, q.points, q.radius, totals, nl.GATHER)
    d["within"] = int(nl.differing_points(nl.Slots(*A["within"][:6]), slots, totals.astype(np.int64)).sum()) + int((counts != totals).sum())
    t, prim, feat = sw.brute_force(g, *q.casts)
    cast = A["cast"]
    d["cast"] = int(((cast[0].view(np.uint32) != t.view(np.uint32)) | (cast[1] != prim) | (cast[5] != feat)).sum())
    c = ir.brute_force(osc, *q.rays)
    d["crossings"] = int(((c.count != A["crossings"][0]) | (c.winding != A["crossings"][1])).sum())
    print("%s: queries that differ from the float32 all-triangles answer: %r" % (case.name, d))
    # pruning with fp32 boxes need not be exactly conservative for the distance queries and the inflated slab: counted and capped as
    # tests/test_nearest_ref.py (0.5 %) and tests/test_sweep_ref.py (1 %) cap them
    assert max(d["nearest"], d["nearest_r"], d["k_nearest"], d["within"]) <= 0.005 * n and d["cast"] <= 0.01 * len(q.casts[0]) and d["crossings"] == 0


def _pairs(prims, totals):
    return set(zip(np.repeat(np.arange(len(totals)), totals.astype(np.int64)).tolist(), np.asarray(prims).tolist()))


def test_the_overlap_and_section_lists_are_the_all_triangles_lists_less_what_the_culls_may_drop(case):
    """The tree never lists a pair the test over all triangles does not.  The other way round the header allows two things.  A node's
    stored box is (lo, lo + (hi - lo)) and a stored v0 + e1 is rounded: a query that touches a triangle in the last bit of its box
    can be culled, in every one of these queries.  And the triangle-overlap predicate is conservative for zero-area triangles: a
    segment or point query passes all seventeen axes against a point of the scene wherever it is, and the cull is what keeps such
    pairs out; every pair only the all-triangles test lists is then checked to have disjoint bounds."""
    g, q, A = case.g, case.q, case.answers
    T = len(g.v0)
    v = np.stack([g.v0, g.v0 + g.e1, g.v0 + g.e2], axis=1)
    tlo, thi = v.min(axis=1), v.max(axis=1)
    out = {}
    for name, mod, queries in (("boxes", ov, q.boxes), ("tris", tv, q.tris)):
        tree = _pairs(*A[name])
        prims, totals = mod.brute_force(g, queries, T)
        rows = prims.reshape(len(queries), T)
        brute = set((i, int(t)) for i in range(len(queries)) for t in rows[i, :totals[i]])
        extra = np.array(sorted(brute - tree), np.int64).reshape(-1, 2)
        qlo, qhi = (queries.min(axis=1), queries.max(axis=1)) if name == "tris" else ov.world_bounds(queries)
        apart = ((qlo[extra[:, 0]] > thi[extra[:, 1]]) | (tlo[extra[:, 1]] > qhi[extra[:, 0]])).any(axis=1)
        out[name] = (len(tree), len(tree - brute), len(extra), int(apart.sum()))
        assert not tree - brute and (name == "boxes" or apart.all()) and len(extra) - apart.sum() <= 0.01 * len(tree), (name, out)
        if name == "tris":
            assert np.isin(case.kind[extra[:, 1]], hm.THIN).all()                # (a sliver's fp32 normal is zero too)
    rec, totals = sr.brute_force(g, q.planes, A["planes"][4].astype(np.int64) + 8)
    start = np.concatenate([[0], np.cumsum(A["planes"][4].astype(np.int64) + 8)])
    brute = set((i, int(t)) for i in range(len(q.planes)) for t in rec["prim"][start[i]:start[i] + totals[i]])
    tree = _pairs(A["planes"][1], A["planes"][4])
    out["planes"] = (len(tree), len(tree - brute), len(brute - tree))
    print("%s: (pairs listed, listed by the tree only, by the all-triangles test only[, of those with disjoint bounds]): %r" % (case.name, out))
    assert (totals <= A["planes"][4] + 8).all() and not tree - brute and len(brute - tree) <= 0.01 * len(tree)


# The measured largest figures of the restatements on exactly these inputs (seed 11), in units of 2^-23 M, M = the largest absolute
# coordinate of the query (for a cast: of its path) and the scene.  Each bound is four times the figure; the margin covers other seeds.
#   nearest, k_nearest   |sqrt(d2) - d64| against the float64 rule over all triangles
#   contact              | |o + d t - triangle| - r | of the entering hits (tests/test_sweep_ref.py, check 1) whose triangle is no sliver
#   contact_sliver       the same on the slivers.  A finding: a sliver's den = d11 d22 - d12 d12 is a rounding error of either sign, and
#                        where it comes out positive the face test accepts on nu, nv that are rounding errors too -- a ray (r = 0)
#                        that passes a sliver 0.0095 scene units away (extent 4, M 17) is reported as a hit on its face.
#   clearance            r - the float64 distance to the mesh along the path before the contact (check 2); none is positive on
#                        the degenerate mesh
MEASURED = {"degenerate": {"nearest": 0.7511, "k_nearest": 0.8025, "contact": 23.2300, "contact_sliver": 4690.5841, "clearance": 0.0},
            "offset": {"nearest": 0.9377, "k_nearest": 0.9377, "contact": 0.4624, "contact_sliver": 0.0002, "clearance": 0.1254}}
BOUND = {name: {k: 4 * v for k, v in row.items()} for name, row in MEASURED.items()}


def _d64(g, pts, chunk=256):
    """float64 dist2 of every point to every triangle [n, T], a NaN (0 / 0 on a zero-area triangle, in float64 as in float32) as inf."""
    v0, e1, e2 = (x.astype(np.float64) for x in (g.v0, g.e1, g.e2))
    p = np.asarray(pts, np.float64)
    out = [nr.closest_on_triangle(p[s:s + chunk, None, :], v0[None], e1[None], e2[None])[0] for s in range(0, len(p), chunk)]
    d2 = np.concatenate(out)
    return np.where(np.isnan(d2), np.inf, d2)


def test_distances_against_float64_over_all_triangles(case):
    g, q, A = case.g, case.q, case.answers
    M = nr.scale_of(g, q.points)
    d64 = np.sqrt(np.sort(_d64(g, q.points), axis=1)[:, :hm.K_NEAR])
    err = np.abs(np.sqrt(A["nearest"][1].astype(np.float64)) - d64[:, 0]) / (2.0 ** -23 * M)
    kd2, kprim = A["k_nearest"][0].reshape(-1, hm.K_NEAR), A["k_nearest"][1].reshape(-1, hm.K_NEAR)
    assert (kprim >= 0).all()
    kerr = (np.abs(np.sqrt(kd2.astype(np.float64)) - d64) / (2.0 ** -23 * M[:, None])).max(axis=1)
    print("%s: largest |sqrt(d2) - d64| / (2^-23 M): nearest %.4f (bound %.4f), the %d nearest %.4f (bound %.4f)"
          % (case.name, err.max(), BOUND[case.name]["nearest"], hm.K_NEAR, kerr.max(), BOUND[case.name]["k_nearest"]))
    assert (err <= BOUND[case.name]["nearest"]).all() and (kerr <= BOUND[case.name]["k_nearest"]).all()


def test_sphere_cast_contact_and_clearance_against_float64(case):
    """The checks 1 and 2 of tests/test_sweep_ref.py on these casts."""
    g, q = case.g, case.q
    res = sw.SweepHits(*case.answers["cast"])
    o, d, r, a, b, M = tsr._ends(g, q.casts, res)
    sel = (res.prim >= 0) & (res.feature < 8)
    cc = o[sel] + d[sel] * res.t[sel].astype(np.float64)[:, None]
    err = np.abs(sw.dist_to_triangle(g, cc, res.prim[sel]) - r[sel]) / (2.0 ** -23 * M[sel])
    err = np.where(np.isnan(err), 0, err)          # (the float64 rule on a zero-area winner can divide 0 by 0 too: the clearance check covers it)
    sliver = case.kind[res.prim[sel]] == hm.SLIVER
    hit = res.prim >= 0
    rows = np.nonzero(b > a)[0]
    k = np.where(hit[rows, None], np.arange(16)[None] / 16.0, np.arange(16)[None] / 15.0)
    with np.errstate(invalid="ignore"):
        t = np.where(np.isinf(b[rows, None]), a[rows, None], a[rows, None] + (b[rows] - a[rows])[:, None] * k)
    pts = o[rows, None, :] + d[rows, None, :] * t[:, :, None]
    dist = sw.dist_to_mesh(g, pts.reshape(-1, 3)).reshape(len(rows), 16)
    deficit = ((r[rows, None] - dist) / (2.0 ** -23 * M[rows, None])).max(axis=1)
    print("%s: largest contact residual / (2^-23 M) = %.4f over %d entering hits off the slivers (bound %.4f), %.4f over %d on them (bound %.4f); "
          "largest clearance deficit %.4f over %d hits and %d misses (bound %.4f)"
          % (case.name, err[~sliver].max(), (~sliver).sum(), BOUND[case.name]["contact"], err[sliver].max(initial=0), sliver.sum(), BOUND[case.name]["contact_sliver"],
             deficit.max(), hit[rows].sum(), (~hit[rows]).sum(), BOUND[case.name]["clearance"]))
    assert sel.sum() > 100 and (err[~sliver] <= BOUND[case.name]["contact"]).all() and (err[sliver] <= BOUND[case.name]["contact_sliver"]).all()
    assert (deficit <= BOUND[case.name]["clearance"]).all()


# ---------------------------------------------------------------- what the GPU test relies on: the hard cases are met

def test_coverage_conditions(case):
    """Stated on the restatement's output for exactly the queries tests/test_gpu_hostile_meshes.py sends, so that it cannot pass by
    avoiding the hard cases."""
    A, kind, twin, za = case.answers, case.kind, case.twin, case.zero_area
    seen = np.zeros(10, np.int64)

    def note(prim):
        np.add.at(seen, kind[prim], 1)

    prim, side = A["nearest"][2], A["nearest"][5]
    won = (prim >= 0) & za[np.maximum(prim, 0)]
    assert won.sum() >= 50 and (side[won] == 1).all()
    note(prim[prim >= 0])
    tied = (prim >= 0) & (twin[np.maximum(prim, 0)] >= 0)
    assert tied.sum() >= 10 and (prim[tied] < twin[prim[tied]]).mean() > 0 and (A["nearest"][1][tied] > 0).any()
    entries = 0
    for name in ("k_nearest", "within"):
        prim, side = A[name][1], A[name][5]
        listed = (prim >= 0) & za[np.maximum(prim, 0)]
        entries += listed.sum()
        assert (side[listed] == 1).all()
        note(prim[prim >= 0])
    assert entries >= 50
    # both triangles of a duplicate pair in one list of the four nearest, in ascending prim and with equal d2
    kp, kd = A["k_nearest"][1].reshape(-1, hm.K_NEAR), A["k_nearest"][0].reshape(-1, hm.K_NEAR)
    both = 0
    for row, d2 in zip(kp, kd):
        for j in range(hm.K_NEAR - 1):
            if row[j] >= 0 and twin[row[j]] == row[j + 1]:
                assert row[j] < row[j + 1] and d2[j] == d2[j + 1]
                both += 1
                break
    prim, feature = A["cast"][1], A["cast"][5]
    on = (prim >= 0) & za[np.maximum(prim, 0)]
    assert on.sum() >= 20 and len(set(feature[on].tolist())) >= 4 and (feature[on] & 7 != 0).all()
    note(prim[prim >= 0])
    lists = {}
    for name in ("boxes", "tris"):
        prims, totals = A[name]
        owner = np.repeat(np.arange(len(totals)), totals.astype(np.int64))
        lists[name] = len(set(owner[za[prims]].tolist()))
        note(prims)
        start = np.concatenate([[0], np.cumsum(totals.astype(np.int64))])
        for i in range(len(totals)):
            row = prims[start[i]:start[i + 1]]
            if len(row) > 1 and np.isin(twin[row][twin[row] >= 0], row).any():
                assert (np.diff(row) > 0).all()
                both += 1
    records = int(za[A["planes"][1]].sum())
    note(A["planes"][1])
    print("%s: zero-area triangles win %d nearest answers of %d (all with side +1), hold %d list entries, take %d sphere-cast hits with features %r, are in %d box "
          "lists, %d triangle-overlap lists and %d section records; %d lists hold both triangles of a duplicate pair, %d nearest answers are tied between a pair; "
          "answers per kind %r" % (case.name, won.sum(), len(won), entries, on.sum(), sorted(set(feature[on].tolist())), lists["boxes"], lists["tris"], records, both,
                                   tied.sum(), dict(zip(hm.KIND_NAMES, seen.tolist()))))
    assert lists["boxes"] >= 20 and lists["tris"] >= 20 and records >= 100 and both >= 10 and (seen > 0).all()


# ---------------------------------------------------------------- the range of scales in which the rules work

SCALED = ("nearest", "nearest_r", "k_nearest", "within", "cast", "boxes", "tris", "planes")
# Casts of the degenerate mesh's query set that differ after scaling by 2^20 and 2^-20 (of 724, by field: t, prim, u, v, point,
# feature).  A finding, not a defect of the restatement: with the direction scaled as well (so that every t stays) the edge test's
# disc = ee (A r2 - det det) is an EIGHTH power of the lengths, 2^160 of the plain value at 2^20: it overflows, and at 2^-20 it
# underflows.  The sweep below gives the sphere cast's range.
CAST_DIFFERS_AT = {20: [169, 125, 134, 164, 197, 165], -20: [291, 194, 224, 237, 291, 244]}


def _scaled_case(case, k, kinds, q=None):
    mesh = hm.scaled(case.mesh, k)
    osc = hm.oracle_scene(mesh)
    for f in ("is_leaf", "child1", "child2", "prim_start", "prim_count"):       # the same tree: the builder's choices are scale-free here
        assert (osc.nodes[f] == case.osc.nodes[f]).all(), (k, f)
    g = nr.from_oracle(osc)
    return g, osc, hm.restate(g, osc, hm.scaled_queries(case.q if q is None else q, k), kinds)


@pytest.mark.parametrize("k", [20, -20])
def test_scaling_by_2_to_the_20_changes_nothing(k):
    """scaled(k) with scaled queries (radii, max_dist, plane d, box halves and cast directions included) gives the plain answer
    scaled, bit for bit on every field."""
    case = _case("degenerate")
    _, _, B = _scaled_case(case, k, SCALED)
    d = {kind: hm.differing(hm.rescale(kind, case.answers[kind], k), B[kind]) for kind in SCALED}
    by_field = [hm.differing((x,), (y,)) for x, y in zip(hm.rescale("cast", case.answers["cast"], k), B["cast"])]
    print("2^%d: entries that differ from the plain answer scaled: %r; the sphere cast by field %r" % (k, d, by_field))
    assert all(v == 0 for kind, v in d.items() if kind != "cast")
    assert by_field == CAST_DIFFERS_AT[k]


# The first scale 2^k, going down in steps of 2, at which a crossing of the plain mesh is lost, and what is left at 2^-20.  With the
# direction scaled too det = dot(e1, cross(dir, e2)) is a third power of the lengths; with the vote's fixed unit directions it is a
# second power, and the vote changes at the same step here.  Going up nothing is lost, but a vote can change: a grazing triangle whose
# |det| was below 1e-6 comes back (45 of 800 votes differ at 2^20).
RAYS_FIRST_LOSS = -4
VOTES_FIRST_CHANGE = -4


def test_the_ray_family_loses_small_triangles_to_the_absolute_epsilon():
    case = _case("degenerate")
    A = case.answers
    assert A["crossings"][0].sum() >= 100 and (A["closest"][1] >= 0).sum() >= 50 and (A["votes_parity"][0] > 0).sum() >= 100
    lost_at = changed_at = None
    for k in range(-2, -22, -2):
        _, _, B = _scaled_case(case, k, ("crossings", "votes_parity"))
        lost = int(A["crossings"][0].sum()) - int(B["crossings"][0].sum())
        changed = int((A["votes_parity"][0] != B["votes_parity"][0]).sum())
        print("2^%d: %d of %d crossings lost, %d of %d votes changed" % (k, lost, A["crossings"][0].sum(), changed, len(A["votes_parity"][0])))
        lost_at = k if lost and lost_at is None else lost_at
        changed_at = k if changed and changed_at is None else changed_at
        if lost_at is not None and changed_at is not None:
            break
    assert (lost_at, changed_at) == (RAYS_FIRST_LOSS, VOTES_FIRST_CHANGE)
    _, _, B = _scaled_case(case, -20, hm.RAY_KINDS)
    assert not B["crossings"][0].any() and not B["crossings"][1].any() and not B["votes_parity"][0].any() and not B["votes_winding"][0].any()
    assert (B["closest"][1] == -1).all() and not B["occluded"][0].any() and len(B["hits"][1]) == 0 and not B["hits"][4].any()


# The range of k, in steps of 2, over which scaled(k) with scaled queries gives the plain answer scaled on EVERY query of a set of the
# aimed queries plus about 100 of each general sweep.  nearest and the near lists: vc, vb, va are fourth powers of the lengths (edges of
# about 2^-2 to 2^4 and points up to 2^7 away here).  Box and triangle overlap: third and fourth powers, but only comparisons leave
# them, and an overflow to infinity on both sides compares like the finite values until a NaN appears.  Sphere cast: eighth powers.
# Plane sections are linear and do not change at any scale a float32 can hold.
RANGE = {"nearest": (-22, 30), "k_nearest": (-22, 30), "within": (-22, 30), "cast": (-4, 10), "boxes": (-32, 42), "tris": (-30, 30)}
OUT_OF_RANGE = (-40, 50)          # 4 steps beyond the widest ends: every rule above has left its range


def test_the_range_of_scales_in_which_the_fourth_power_rules_work():
    case = _case("degenerate")
    q = hm.queries(case.g, case.osc, case.kind, case.twin, SEED, general=100)
    kinds = tuple(RANGE)
    plain = hm.restate(case.g, case.osc, q, kinds + ("planes",))
    found = {}
    for kind in kinds:
        ends = []
        for step in (-2, 2):
            k = 0
            while abs(k) < 60:
                _, _, B = _scaled_case(case, k + step, (kind,), q)
                if hm.differing(hm.rescale(kind, plain[kind], k + step), B[kind]) != 0:
                    break
                k += step
            ends.append(k)
        found[kind] = tuple(ends)
        print("%s: scaling by 2^k changes nothing for k in [%d, %d]" % (kind, *found[kind]))
    assert found == RANGE
    assert OUT_OF_RANGE == (min(lo for lo, _ in RANGE.values()) - 8, max(hi for _, hi in RANGE.values()) + 8)
    for k in OUT_OF_RANGE:
        _, _, B = _scaled_case(case, k, kinds + ("planes",), q)
        assert all(hm.differing(hm.rescale(kind, plain[kind], k), B[kind]) != 0 for kind in kinds), k
        assert hm.differing(hm.rescale("planes", plain["planes"], k), B["planes"]) == 0, k
