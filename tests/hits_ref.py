"""Restatement of the hit-list query (include/drt.h drt_renderer_list_hits) over the oracle's scene, for the tests.  No tests of its own.

The traversal is inside_ref.crossings', step for step (every step pops one stack entry of every ray that still has one; boxes are
oracle.kat_slab), and every listed (ray, triangle) pair is recorded as it is found: t and uvw are oracle.kat_intersect's, u, v =
uvw[1], uvw[2] as ray_query_ref.closest takes them.  The records of one ray, in the order they were found, are its ARRIVAL order; the
rule's order is ascending t, equal t by ascending prim.  A scene is anything with `.nodes` (root last) and `.tris["p"]`.
"""
import collections

import numpy as np

import oracle
from tests import inside_ref as ir

Records = collections.namedtuple("Records", "ray t prim u v")          # one entry per listed pair; per ray in arrival order
Slots = collections.namedtuple("Slots", "t prim u v")                  # one entry per slot of every ray's segment, ray after ray
INF = ir.INF


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _rays(org, dirs, tmin, tmax):
    n = len(org)
    rays6 = _f32(np.concatenate([_f32(org).reshape(-1, 3), _f32(dirs).reshape(-1, 3)], axis=1))
    return rays6, _f32(np.broadcast_to(np.float32(tmin), n)), _f32(np.broadcast_to(np.float32(tmax), n))


def _listed(osc, rays6, prim, tmin, tmax):
    """(listed, t, u, v) for (ray, triangle) pairs: the test hits, t > tmin, t < tmax."""
    out, hit = oracle.kat_intersect(rays6, osc.tris["p"][prim].reshape(-1, 9))
    t = out[:, 0]
    with np.errstate(invalid="ignore"):
        listed = (hit != 0) & (t > tmin) & (t < tmax)
    return listed, t, out[:, 2], out[:, 3]


def _collect(n, parts):
    """Chunks of (ray, t, prim, u, v) in the order they were found -> Records grouped by ray, each ray's in arrival order."""
    if not parts:
        return Records(np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.float32))
    ray, t, prim, u, v = [np.concatenate([p[k] for p in parts]) for k in range(5)]
    order = np.argsort(ray, kind="stable")
    return Records(ray[order].astype(np.int64), _f32(t[order]), prim[order].astype(np.int32), _f32(u[order]), _f32(v[order]))


def records(osc, org, dirs, tmin=0.0, tmax=INF):
    """drt.h "hit list of a ray", the listed pairs: inside_ref.crossings' traversal, every listed triangle recorded where it counts one."""
    n = len(org)
    rays6, tmin, tmax = _rays(org, dirs, tmin, tmax)
    parts = []
    if len(osc.nodes) == 0 or n == 0:
        return _collect(n, parts)
    root = len(osc.nodes) - 1
    with np.errstate(invalid="ignore"):
        d = ir._slab(osc, rays6, np.full(n, root))
        sp = np.where((d < 0) | (d > tmax), 0, 1)                               # the root is skipped if d < 0 || d > tmax
    st = np.zeros((n, ir.MAX_STACK), np.int64)
    st[:, 0] = root
    while True:
        act = np.nonzero(sp > 0)[0]
        if len(act) == 0:
            break
        sp[act] -= 1
        node = st[act, sp[act]]
        leaf = osc.nodes["is_leaf"][node] != 0
        la, ln = act[leaf], node[leaf]
        start, cnt = osc.nodes["prim_start"][ln], osc.nodes["prim_count"][ln]
        for k in range(int(cnt.max()) if len(ln) else 0):                      # the leaf's triangles in order: the arrival order
            sel = cnt > k
            r, prim = la[sel], (start[sel] + k).astype(np.int64)
            listed, t, u, v = _listed(osc, rays6[r], prim, tmin[r], tmax[r])
            if listed.any():
                parts.append((r[listed], t[listed], prim[listed], u[listed], v[listed]))
        ia, inode = act[~leaf], node[~leaf]
        if len(ia):
            c1, c2 = osc.nodes["child1"][inode], osc.nodes["child2"][inode]
            with np.errstate(invalid="ignore"):
                h1, h2 = ir._slab(osc, rays6[ia], c1), ir._slab(osc, rays6[ia], c2)
                p1 = (h1 >= 0) & ~(h1 > tmax[ia])                               # a child is pushed iff d >= 0 && !(d > tmax)
                p2 = (h2 >= 0) & ~(h2 > tmax[ia])
                far1 = h1 > h2                                                  # the farther child first
            for push, c in ((np.where(far1, p1, p2), np.where(far1, c1, c2)), (np.where(far1, p2, p1), np.where(far1, c2, c1))):
                r = ia[push]
                st[r, sp[r]] = c[push]
                sp[r] += 1
    return _collect(n, parts)


def brute_records(osc, org, dirs, tmin=0.0, tmax=INF, chunk=512):
    """The per-pair rule over ALL triangles, no boxes (a ray's records in triangle order)."""
    n, T = len(org), len(osc.tris)
    rays6, tmin, tmax = _rays(org, dirs, tmin, tmax)
    parts = []
    for s in range(0, n if T else 0, chunk):
        m = len(rays6[s:s + chunk])
        r, prim = np.repeat(np.arange(s, s + m), T), np.tile(np.arange(T), m)
        listed, t, u, v = _listed(osc, rays6[r], prim, tmin[r], tmax[r])
        parts.append((r[listed], t[listed], prim[listed], u[listed], v[listed]))
    return _collect(n, parts)


def ranks(n, rec):
    """(arrival rank, sorted rank, totals): the position of every record among its ray's records as found, and under the rule's order
    (ascending t, equal t by ascending prim)."""
    totals = np.bincount(rec.ray, minlength=n).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(totals)])[:-1]
    idx = np.arange(len(rec.ray))
    arrival = idx - first[rec.ray]
    order = np.lexsort((rec.prim, rec.t, rec.ray))                               # by ray, then t, then prim
    srank = np.empty(len(idx), np.int64)
    srank[order] = idx - first[rec.ray[order]]
    return arrival, srank, totals


def list_hits(osc, org, dirs, tmin, tmax, caps, rec=None):
    """drt.h "segments": (Slots of sum(caps) entries, ray i's at [cumsum(caps)[i-1], cumsum(caps)[i]); totals uint32 [n]).  Slot j of a ray
    holds its j-th listed triangle in order for j < min(cap, total), the miss record {tmax, -1, 0, 0} beyond.  rec: records(...) by
    default, or brute_records(...)."""
    n = len(org)
    caps = np.broadcast_to(np.asarray(caps, np.int64), n)
    _, _, tmax_n = _rays(org, dirs, tmin, tmax)
    rec = records(osc, org, dirs, tmin, tmax) if rec is None else rec
    _, srank, totals = ranks(n, rec)
    base = np.concatenate([[0], np.cumsum(caps)])
    t, prim = np.repeat(tmax_n, caps), np.full(base[-1], -1, np.int32)            # the ray's own tmax word
    u, v = np.zeros(base[-1], np.float32), np.zeros(base[-1], np.float32)
    keep = srank < caps[rec.ray]
    dest = base[rec.ray[keep]] + srank[keep]
    t[dest], prim[dest], u[dest], v[dest] = rec.t[keep], rec.prim[keep], rec.u[keep], rec.v[keep]
    return Slots(_f32(t), prim, u, v), totals.astype(np.uint32)


def out_of_order_rays(n, rec):
    """bool [n]: the ray's arrival order is not the rule's order (an insert in the middle of the list)."""
    arrival, srank, _ = ranks(n, rec)
    out = np.zeros(n, bool)
    out[rec.ray[arrival != srank]] = True
    return out


def evicting_rays(n, rec, k):
    """bool [n]: at capacity k a later arrival replaces a stored record -- one of the k first in order arrives after k others."""
    arrival, srank, _ = ranks(n, rec)
    out = np.zeros(n, bool)
    out[rec.ray[(arrival >= k) & (srank < k)]] = True
    return out


def tied_rays(n, rec):
    """bool [n]: two of the ray's records have the same t (and different prim: a triangle is listed once)."""
    order = np.lexsort((rec.prim, rec.t, rec.ray))
    r, t = rec.ray[order], rec.t[order]
    same = (r[1:] == r[:-1]) & (t[1:] == t[:-1])
    out = np.zeros(n, bool)
    out[r[1:][same]] = True
    return out


# ---------------------------------------------------------------- scenes and ray sets shared by the CPU and GPU tests

SCENE_NAMES = ["doubled_cube", "soup", "chain", "torus", "cornell_box"]
# (streams, leaf size, bins): the doubled cube has every triangle twice, so every hit ties with its copy (leaf 2 does not build: the
# oracle's builder refuses coincident triangles at that leaf size); the soup has long, unordered lists and an RGBA cut-out material;
# the chain's tree is deeper than the 16 stack levels in LDS and a ray along it passes through most of its triangles
GEOMETRY = {"doubled_cube": (lambda: ir.streams(np.concatenate([ir.cube(), ir.cube()])), 4, 8),
            "soup": (lambda: _rq().soup(1500, 3, half=1.0), 6, 8),
            "chain": (lambda: _rq().degenerate_chain(62), 1, 2),
            "torus": (lambda: ir.streams(ir.torus()), 4, 8)}
CORNELL_TREE = (20, 8)
_osc = {}


def _rq():
    from tests import ray_query_ref
    return ray_query_ref


def oracle_scene(name):
    """The oracle's scene and tree of `name` (cached)."""
    if name not in _osc:
        if name == "cornell_box":
            from tests.scenes import scene_path
            _osc[name] = oracle.Scene.load_glb(scene_path(name)).build_bvh(*CORNELL_TREE)
        else:
            make, leaf, bins = GEOMETRY[name]
            s = make()
            from tests import refit_ref
            _osc[name] = oracle.Scene(refit_ref.triangles(*s[:4]), s[4], s[5]).build_bvh(leaf, bins)
    return _osc[name]


def ray_set(name, osc):
    """(org, dirs, tmin, tmax, n_plain): the scene's n_plain rays -- 500 surface rays and 700 rays with random intervals (seed 7), the
    soup's 600 rays from inside boxes (seed 5), the chain's 400 rays along it in both directions -- and behind them six rays with a
    NaN origin, a NaN direction or a NaN interval."""
    rq = _rq()
    if name == "soup":
        org, dirs = rq.box_rays(osc, 600, np.random.default_rng(5))
        tmin, tmax = np.zeros(600, np.float32), np.full(600, np.inf, np.float32)
    elif name == "chain":
        # towards -x the near leaves are the farther children, so they wait on the stack
        k = 200
        rng = np.random.default_rng(7)
        org = np.concatenate([np.tile(np.float32([-3, 0, 0]), (k, 1)), np.tile(np.float32([2.0 ** 62, 0, 0]), (k, 1))])
        dirs = np.concatenate([np.ones((2 * k, 1), np.float32), rng.normal(scale=0.02, size=(2 * k, 2)).astype(np.float32)], axis=1)
        dirs[k:, 0] = -1
        tmin, tmax = np.zeros(2 * k, np.float32), np.full(2 * k, np.inf, np.float32)
    else:
        rng = np.random.default_rng(7)
        o1, d1 = rq.surface_rays(osc, 500, rng)
        o2, d2, tmin2, tmax2 = rq.interval_rays(osc, 700, rng)
        org, dirs = np.concatenate([o1, o2]), np.concatenate([d1, d2])
        tmin, tmax = np.concatenate([np.zeros(500, np.float32), tmin2]), np.concatenate([np.full(500, np.inf, np.float32), tmax2])
    n_plain = len(org)
    o4, d4 = _f32(org[:6]).copy(), _f32(dirs[:6]).copy()
    o4[0, 0] = o4[1, 2] = d4[2, 1] = d4[3, 0] = np.nan
    tmin4, tmax4 = np.float32([0, 0, 0, 0, np.nan, 0]), np.float32([np.inf, np.inf, np.inf, np.inf, np.inf, np.nan])
    return (_f32(np.concatenate([org, o4])), _f32(np.concatenate([dirs, d4])), _f32(np.concatenate([tmin, tmin4])),
            _f32(np.concatenate([tmax, tmax4])), n_plain)
