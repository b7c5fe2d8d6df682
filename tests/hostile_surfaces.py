"""Connected surfaces that are not well behaved, the queries aimed at them and what the restatements say of them, for
tests/test_hostile_surfaces_ref.py (CPU) and tests/test_gpu_hostile_surfaces.py.  No tests of its own; numpy and the oracle only.

Real meshes carry their zero-area triangles linked into the edge adjacency: where an edge a b of a triangle (a, b, c) is split on one
side only, (a, b, c) becomes (a, m, c) and (m, b, c), the neighbour across a b keeps the whole edge, and the gap is closed by the cap
(a, b, m) -- a T-junction cap.  m is the fp32 midpoint of a b: where that midpoint is a float32 the cap has exactly zero area, where it
was rounded the cap is a sliver.  `capped` makes such meshes; split on both sides of one edge, the two caps and the four halves meet
in the edges a m and m b four at a time, which is non-manifold (-2).

  capped_sparse   curve_scenes.spheres(1)'s scene sphere with 24 caps that share no edge: one watertight shell
  capped_dense    the same sphere with 400 caps wherever they fall -- collisions, -2 edges, several shells -- and 26 triangles taken out,
                  one from the fan round each pole: boundary loops whose rotations meet -2 edges
  capped_band     contour_scenes.ring(400), whose coordinates are multiples of 2^-8, with 120 caps on edges from z = -1 to z = +1: every
                  midpoint is exact, lies in the plane z = 0, and every cap has exactly zero area
  soup            hostile_meshes.degenerate(), unconnected, with hostile_meshes.queries' triangles and planes unchanged

Every mesh comes as `plain`, `offset` (+ hostile_meshes.OFFSET, rounded once per coordinate, so that shared vertices stay shared),
`scaled(k)` for k = +-20 (inside the working range), the fringe scales -32, -36, 36, 42 (where the intersection records are lost one by
one to underflow and overflow) and hostile_meshes' out-of-range scales -40 and 50.  The queries of `plain` and `offset` are aimed at the
variant's own vertices; those of a scaled variant are the plain queries scaled.
"""
import collections

import numpy as np

import oracle
from tests import contour_ref as cr
from tests import contour_scenes as cs
from tests import curve_ref as cu
from tests import curve_scenes as cv
from tests import hostile_meshes as hm
from tests import intersect_ref as ix
from tests import nearest_ref as nr
from tests import refit_ref as rf
from tests import section_ref as sr
from tests import topology_ref as tr

SEED = 11                                                     # tests/test_hostile_meshes_ref.py's: the soup's queries are its queries
OUT_OF_RANGE = (-40, 50)                                      # tests/test_hostile_meshes_ref.py's (asserted there and in the CPU test here)
FRINGE = (-32, -36, 36, 42)
MESHES = ("capped_sparse", "capped_dense", "capped_band", "soup")
CAPPED_MESHES = MESHES[:3]
VARIANTS = ("plain", "offset", "scaled(20)", "scaled(-20)") + tuple("scaled(%d)" % k for k in FRINGE + OUT_OF_RANGE)
BAND_QUADS = 400
AIMED_CAPS = 48                                               # the caps the aimed queries go to (all of capped_sparse's)

Capped = collections.namedtuple("Capped", "pos cap exact")    # positions [T + 2 k, 3, 3]; the caps' indices [k]; midpoint exact [k]
Queries = collections.namedtuple("Queries", "tris n_tool planes n_aimed_planes")
ALL_KINDS = ("cut", "self", "curve", "section", "contour", "topology")


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def capped(positions, k, seed, adjacent_ok, eligible=None):
    """Split k triangle edges on one side only.  Triangle A = (a, b, c), rotated so that the chosen edge is a b, becomes (a, m, c) in
    A's place; (m, b, c) and the cap (a, b, m) are appended, m = float32((a + b) / 2).  The neighbour across a b keeps its edge b a,
    whose twin is now the cap's.  adjacent_ok=False: no chosen triangle is the neighbour of another across any edge, so no edge is
    split from both sides and a manifold mesh stays manifold.  True: k triangles wherever they fall.  eligible: bool [T, 3], the
    edges that may be chosen.  A triangle is split once at most."""
    pos = _f32(positions).reshape(-1, 3, 3)
    n = len(pos)
    rng = np.random.default_rng(seed)
    adj = cr.adjacency(pos).reshape(n, 3)
    ok = np.ones((n, 3), bool) if eligible is None else np.asarray(eligible, bool)
    taken = np.zeros(n, bool)
    chosen = []
    for t in rng.permutation(n):
        if len(chosen) == k:
            break
        edges = np.nonzero(ok[t])[0]
        if taken[t] or len(edges) == 0:
            continue
        chosen.append((int(t), int(rng.choice(edges))))
        if not adjacent_ok:
            taken[t] = True
            taken[adj[t][adj[t] >= 0] // 3] = True
    assert len(chosen) == k, "only %d of %d edges found" % (len(chosen), k)
    out, halves, caps, exact = pos.copy(), [], [], []
    for t, e in chosen:
        a, b, c = pos[t, e], pos[t, (e + 1) % 3], pos[t, (e + 2) % 3]
        mid = (a.astype(np.float64) + b.astype(np.float64)) / 2
        m = mid.astype(np.float32)
        out[t] = [a, m, c]
        halves.append([m, b, c])
        caps.append([a, b, m])
        exact.append(bool((m.astype(np.float64) == mid).all()))
    return Capped(np.concatenate([out, _f32(halves), _f32(caps)]), n + k + np.arange(k), np.array(exact))


def punched(made, count, seed):
    """A capped UV sphere of curve_scenes.uv_sphere(40, 20) without one triangle of the fan round each pole and `count` more of its
    first 1520 triangles: the holes' boundary half-edges rotate through fans that hold -2 edges, the two at the poles through up to
    39 triangles.  (A removed triangle that was split leaves its other half and its cap behind.)"""
    keep = np.ones(len(made.pos), bool)
    keep[[0, 38 * 5 + 1]] = False                                # uv_sphere lists 38 triangles per segment: the top one, the bottom one, 36
    keep[np.random.default_rng(seed).choice(1520, count, replace=False)] = False
    return Capped(made.pos[keep], (np.cumsum(keep) - 1)[made.cap], made.exact)


def _band_edges(pos):
    """The edges of the band that run from z = -1 to z = +1, either way."""
    z = pos[:, :, 2]
    return z != np.roll(z, -1, axis=1)


_meshes = {}


def mesh(name):
    """The plain mesh: a Capped (for the soup: the positions of hostile_meshes.degenerate(), no caps)."""
    if name not in _meshes:
        if name == "capped_sparse":
            made = capped(cv.spheres(1)[0], 24, 1, False)
        elif name == "capped_dense":
            made = punched(capped(cv.spheres(1)[0], 400, 2, True), 24, 4)
        elif name == "capped_band":
            band = cs.ring(quads=BAND_QUADS)
            made = capped(band, 120, 3, False, _band_edges(band))
        else:
            made = Capped(hm.degenerate().pos, np.zeros(0, np.int64), np.zeros(0, bool))
        _meshes[name] = made
    return _meshes[name]


def scale_of(variant):
    """k of "scaled(k)", None of the other variants."""
    return int(variant[len("scaled("):-1]) if variant.startswith("scaled") else None


def moved(a, variant):
    """Coordinates of the plain mesh (or of its queries) as the variant has them."""
    k = scale_of(variant)
    with np.errstate(over="ignore", under="ignore"):
        if k is not None:
            return (a * np.float32(2.0 ** k)).astype(np.float32)
        return (a + hm.OFFSET).astype(np.float32) if variant == "offset" else _f32(a)


def zero_area(pos):
    """bool [T]: the cross product of the exact edges is exactly zero (float64 holds the products of float32 differences here)."""
    p = pos.astype(np.float64)
    return ~(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]) != 0).any(axis=1)


# ---------------------------------------------------------------- the queries

def _unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def aimed_triangles(pos, cap, n_caps, seed):
    """Query triangles [8 per cap, 3, 3] at the caps (a, b, m) of pos (cap: their indices; n_caps: how many caps the mesh has), all
    through the surface there:
      two small ones (2 % and 10 % of the edge) round a point of a b
      (m, x, y), (a, x, y)         one vertex shared bit for bit with the cap: that scene vertex lies exactly on the query's plane, s = 0
      (a, b, x), (m, b, y)         a whole edge of the cap
      (c, x, y)                    a vertex of the neighbour (m, b, c) that the cap does not have
      (y', b, m)                   the cap's edge m b the other way round, as a twin has it
    x and y lie on opposite sides of the surface, about an edge length away."""
    rng = np.random.default_rng(seed)
    out = []
    for t in cap:
        a, b, m = (v.astype(np.float64) for v in pos[t])
        c = pos[t - n_caps, 2].astype(np.float64)                   # the other half (m, b, c) stands n_caps in front of its cap
        edge = np.linalg.norm(b - a)
        away = _unit(rng, 4) * edge
        x, y = m + away[0], m - away[0] + 0.3 * away[1]
        centre = a + (b - a) * rng.uniform(0.2, 0.8)
        for size in (0.02, 0.1):
            out.append(centre + rng.uniform(-1, 1, (3, 3)) * size * edge)
        out += [[m, x, y], [a, x, y], [a, b, x], [m, b, y], [c, x, y], [m, b, y - away[2]][::-1]]
    return _f32(out).reshape(-1, 3, 3)


def aimed_planes(pos, cap, seed, levels=40):
    """Planes [N, 4]: an axis plane through every cap's midpoint m (s(m) = 0 exactly), a plane that contains the cap's edge a b (n
    perpendicular to it, d = dot(n, a) in fp32), 40 axis planes through vertices anywhere on the mesh, and `levels` general levels: planes z = const through the mesh, between its vertices'
    heights.  Returns (planes, the number of aimed ones in front)."""
    rng = np.random.default_rng(seed)
    a, b, m = pos[cap, 0], pos[cap, 1], pos[cap, 2]
    axis = (np.eye(3, dtype=np.float32)[rng.integers(0, 3, len(cap))] * np.float32(rng.choice([-1, 1], len(cap)))[:, None]).astype(np.float32)
    through = sr.pack(axis, nr.dot(axis, m))
    n = _f32(np.cross((b - a).astype(np.float64), _unit(rng, len(cap))))
    along = sr.pack(n, nr.dot(n, a))
    # axis planes through 40 vertices anywhere on the mesh: the packed v0 + e1 of one triangle and the v0 of its neighbour are one
    # position but not always one float, so the two can disagree on the side of the shared vertex: exit statuses 3 and 4
    t = rng.choice(len(pos), 40, replace=False)
    axis = (np.eye(3, dtype=np.float32)[rng.integers(0, 3, 40)] * np.float32(rng.choice([-1, 1], 40))[:, None]).astype(np.float32)
    vertex = sr.pack(axis, nr.dot(axis, pos[t, rng.integers(0, 3, 40)]))
    lo, hi = float(pos[..., 2].min()), float(pos[..., 2].max())
    z = _f32(lo + (hi - lo) * (np.arange(levels) + 0.37) / levels)
    general = sr.pack(np.tile(np.float32([0, 0, 1]), (levels, 1)), z)
    return np.concatenate([through, along, vertex, general]).astype(np.float32), 2 * len(cap) + 40


def band_planes(pos, cap, seed, shift):
    """The band's planes: z = 0 (through every cap's midpoint: a vertex exactly on the plane), z = 0.5 and z = -0.25 (through every cap
    but through no vertex), the same with the normal reversed, then aimed_planes with 4 levels."""
    special = sr.pack([(0, 0, 1), (0, 0, 1), (0, 0, 1), (0, 0, -1), (0, 0, -2)], [0, 0.5, -0.25, 0, -1])
    aimed, n = aimed_planes(pos, cap, seed, levels=4)
    special[:, 3] = (special[:, 3] + special[:, 0:3] @ _f32(shift)).astype(np.float32)
    return np.concatenate([special, aimed]), len(special) + n


# ---------------------------------------------------------------- a case: a mesh in one variant, its scene, its queries, the answers

def oracle_scene(pos):
    """The oracle's scene of positions with the (4, 8) tree, as contour_scenes.flat_scene builds it -- no product library needed."""
    n = len(pos)
    nrm = np.tile(np.float32([0, 0, 1]), (n, 3, 1))
    return oracle.Scene(rf.triangles(pos, nrm, np.zeros((n, 3, 2), np.float32), np.zeros(n, np.int32)), hm.ONE_MATERIAL, []).build_bvh(hm.LEAF, hm.BINS)


class Case:
    """mesh x variant: the positions in load order, the oracle's scene (tree order), which tree triangles are caps, the queries."""

    def __init__(self, name, variant):
        self.name, self.variant = name, variant
        plain = mesh(name)
        k = scale_of(variant)
        if name == "soup":
            base = hm.degenerate()
            self.mesh = hm.scaled(base, k) if k is not None else (hm.offset(base) if variant == "offset" else base)
            self.pos = self.mesh.pos
            with np.errstate(over="ignore", under="ignore"):
                self.osc = hm.oracle_scene(self.mesh)
        else:
            self.pos = moved(plain.pos, variant)
            with np.errstate(over="ignore", under="ignore"):
                self.osc = oracle_scene(self.pos)
        self.g = nr.from_oracle(self.osc)
        self.tree = np.ascontiguousarray(self.osc.tris["p"], np.float32).reshape(-1, 3, 3)
        self.is_cap = self._caps_in_tree_order(plain)
        if k is not None:
            q = case(name, "plain").q
            planes = q.planes.copy()
            with np.errstate(over="ignore", under="ignore"):
                planes[:, 3] *= np.float32(2.0 ** k)
            self.q = Queries(moved(q.tris, variant), q.n_tool, planes, q.n_aimed_planes)
        elif name == "soup":
            kind, twin = hm.kinds_in_tree_order(self.osc, self.mesh)
            q = hm.queries(self.g, self.osc, kind, twin, SEED)
            self.q = Queries(q.tris, len(q.tris), q.planes, len(q.planes))
        else:
            aim = plain.cap[:AIMED_CAPS]
            if name == "capped_band":
                tool = np.concatenate([cv.BIG, cv.quad_queries()])
                planes, n_aimed = band_planes(self.pos, aim, SEED + 1, hm.OFFSET if variant == "offset" else np.zeros(3))
            else:
                tool = cv.spheres(1)[1]
                planes, n_aimed = aimed_planes(self.pos, aim, SEED + 1)
            tool = moved(tool, variant)
            self.q = Queries(np.concatenate([tool, aimed_triangles(self.pos, aim, len(plain.cap), SEED)]), len(tool), planes, n_aimed)
        self.answers = {}

    def _caps_in_tree_order(self, plain):
        """bool [T] in tree order: the builder reorders triangles, each is found again by its nine coordinates."""
        caps = {self.pos[t].tobytes() for t in plain.cap}
        return np.array([p.tobytes() in caps for p in self.tree], bool)


_cases = {}


def case(name, variant):
    if (name, variant) not in _cases:
        _cases[(name, variant)] = Case(name, variant)
    return _cases[(name, variant)]


def restate(c, kinds=ALL_KINDS):
    """Every expected answer of a case, computed once per kind with the existing restatements and kept in c.answers:
      adj, query_adj       contour_ref.adjacency of the tree-order positions, curve_ref.tri_adjacency of the query triangles
      cut                  (splits, records [M, 8]) of intersect_ref.whole
      self                 intersect_ref.self_cuts
      curve                (slots, counts) of curve_ref.chain on the cut
      section              (records, totals) of section_ref.whole
      contour              (slots, chains) of contour_ref.chain on the section; areas: contour_ref.areas
      labels, counts, loops, terms, measures    topology_ref's, the terms from the positions as the scene packs them"""
    A = c.answers
    with np.errstate(all="ignore"):
        if "adj" not in A:
            A["adj"], A["query_adj"] = cr.adjacency(c.tree), cu.tri_adjacency(c.q.tris)
        for kind in kinds:
            if kind in A:
                continue
            if kind == "cut":
                A["cut"] = ix.whole(c.g, c.q.tris)
            elif kind == "self":
                A["self"] = ix.self_cuts(c.g, c.tree)
            elif kind == "curve":
                splits, rec = restate(c, ("cut",))["cut"]
                w = rec.view(np.int32)
                A["curve"] = cu.chain(A["adj"], A["query_adj"], w[:, 3], w[:, 7], splits, len(c.tree))
            elif kind == "section":
                A["section"] = sr.whole(c.g, c.q.planes)
            elif kind == "contour":
                rec, totals = restate(c, ("section",))["section"]
                splits = np.concatenate([[0], np.cumsum(totals.astype(np.int64))])
                A["contour"] = cr.chain(A["adj"], rec, splits)
                A["areas"] = cr.areas(c.q.planes, rec, *A["contour"], splits)
            elif kind == "topology":
                A["labels"] = tr.labels(A["adj"])
                A["counts"] = tr.counts(A["adj"], A["labels"])
                A["loops"] = tr.loops(A["adj"])
                A["terms"] = tr.terms(*tr.packed(c.tree))
                index, tri = tr.per_shell(A["adj"], A["labels"])[:2]
                A["measures"] = tr.measures(A["terms"], index, len(tri))
                A["topology"] = True
    return A


def curve_status(c):
    """The number of live records per exit status 0..4 of the case's curves."""
    slots = restate(c, ("curve",))["curve"][0]
    return np.bincount(slots["flags"] >> 1, minlength=6)[:5]


def contour_status(c):
    slots = restate(c, ("contour",))["contour"][0]
    return np.bincount(slots["flags"] >> 1, minlength=6)[:5]


def scaled_records(rec, k):
    """Intersection or section records [M, 8] with p and q times 2^k and every integer unchanged."""
    out = np.ascontiguousarray(rec).view(np.float32).reshape(-1, 8).copy()
    with np.errstate(over="ignore", under="ignore"):
        out[:, 0:3] *= np.float32(2.0 ** k)
        out[:, 4:7] *= np.float32(2.0 ** k)
    return out


# ---------------------------------------------------------------- what the aimed triangles meet, recomputed from the header's rule

def ties(c):
    """Over the records of the case's aimed tool triangles, by intersect_ref.segment's own steps in float32: (records with a query
    edge endpoint, i.e. a code digit of 4 or more; pairs tied on the interval axis, ql[j] == tl[j] or qh[j] == th[j]; pairs with a
    scene vertex exactly on the query's plane, some s_k == 0)."""
    splits, rec = restate(c, ("cut",))["cut"]
    lo = int(splits[c.q.n_tool])
    w = rec.view(np.int32)
    owner = np.repeat(np.arange(len(c.q.tris)), np.diff(splits))[lo:]
    prim, code = w[lo:, 3], w[lo:, 7]
    q = c.q.tris[owner]
    v0, e1, e2 = c.g.v0[prim], c.g.e1[prim], c.g.e2[prim]
    with np.errstate(all="ignore"):
        w0, w1, w2 = v0, v0 + e1, v0 + e2
        nq = ix.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0])
        s = [nr.dot(nq, x - q[:, 0]) for x in (w0, w1, w2)]
        nt = ix.cross(e1, e2)
        u = [nr.dot(nt, x - v0) for x in (q[:, 0], q[:, 1], q[:, 2])]
        aD = np.abs(ix.cross(nq, nt))
        j = np.where(aD[:, 1] > aD[:, 0], 1, 0)
        j = np.where(aD[:, 2] > aD[np.arange(len(j)), j], 2, j)
        T1, _, T2, _ = ix._apex_cuts((w0, w1, w2), s)
        Q1, _, Q2, _ = ix._apex_cuts((q[:, 0], q[:, 1], q[:, 2]), u)
        on = lambda P: P[np.arange(len(j)), j]
        tl, th = np.minimum(on(T1), on(T2)), np.maximum(on(T1), on(T2))
        ql, qh = np.minimum(on(Q1), on(Q2)), np.maximum(on(Q1), on(Q2))
    endpoint = ((code & 15) >= 4) | ((code >> 4) >= 4)
    tied = (ql == tl) | (qh == th)
    on_plane = (s[0] == 0) | (s[1] == 0) | (s[2] == 0)
    return int(endpoint.sum()), int(tied.sum()), int(on_plane.sum())


# ---------------------------------------------------------------- a refit into degeneracy

def collapsed(c, seed=5):
    """Positions in LOAD order for a refit of a capped sphere: 20 further triangles collapse to zero area (v1 = v0 in that triangle
    alone, so its neighbours lose their twins there) and ten vertices move onto a neighbour along an edge, in every triangle that
    has them (the triangles on that edge get a zero-length edge, the rest share the new position)."""
    rng = np.random.default_rng(seed)
    pos = c.pos.copy()
    plain = np.nonzero(~zero_area(pos))[0]
    pick = rng.permutation(plain)
    for t in pick[:20]:
        pos[t, 1] = pos[t, 0]
    for t in pick[20:30]:
        v, w = c.pos[t, 0].copy(), c.pos[t, 1].copy()
        same = (pos.view(np.uint32) == v.view(np.uint32)).all(axis=-1)
        pos[same] = w
    return pos
