"""Restatement of the crossing-count queries (include/drt.h drt_renderer_crossings / drt_renderer_inside /
drt_renderer_signed_distance) over the oracle's scene, for the tests.  No tests of its own.

The traversal is ray_query_ref.occluded's without the early exit and without the alpha test, vectorised over rays: every step pops
one stack entry of every ray that still has one.  Boxes are oracle.kat_slab, a triangle's hit and t are oracle.kat_intersect; only
det = dot(e1, cross(dir, e2)) is restated, in float32 numpy in device_math.hpp's operation order (numpy rounds every operation on
its own).  A scene is anything with `.nodes` (root last) and `.tris["p"]`: the oracle's, or product_scene() of a host scene.
"""
import collections
import types

import numpy as np

import oracle
from tests import nearest_ref as nr
from tests import refit_ref as rf

Crossings = collections.namedtuple("Crossings", "count winding")
MAX_STACK = 64
INF = np.float32(np.inf)
# drt.h "inside vote": the three directions, used as given
DIRS = np.float32([[0.6180340, 0.4142136, 0.6687403], [-0.7320508, 0.2360680, 0.6403124], [0.3166248, -0.8660254, 0.3872983]])
RULES = {"parity": 0, "winding": 1}


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def det_of(dirs, p):
    """det of Intersection.cu for (direction, triangle p [k, 3, 3]) pairs: e1 = v1 - v0, e2 = v2 - v0, pvec = cross(dir, e2) =
    (d.y e.z - d.z e.y, d.z e.x - d.x e.z, d.x e.y - d.y e.x), det = (e1.x pvec.x + e1.y pvec.y) + e1.z pvec.z."""
    d, p = _f32(dirs), _f32(p)
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    with np.errstate(all="ignore"):
        px = d[:, 1] * e2[:, 2] - d[:, 2] * e2[:, 1]
        py = d[:, 2] * e2[:, 0] - d[:, 0] * e2[:, 2]
        pz = d[:, 0] * e2[:, 1] - d[:, 1] * e2[:, 0]
        return ((e1[:, 0] * px + e1[:, 1] * py) + e1[:, 2] * pz).astype(np.float32)


def _pairs(osc, rays6, prim, tmin, tmax):
    """(counted, +1 / -1) for (ray, triangle) pairs: the test hits, t > tmin, t < tmax; det < 0 ? +1 : -1."""
    p = osc.tris["p"][prim]
    out, hit = oracle.kat_intersect(rays6, p.reshape(-1, 9))
    t = out[:, 0]
    with np.errstate(invalid="ignore"):
        counted = (hit != 0) & (t > tmin) & (t < tmax)
        sign = np.where(det_of(rays6[:, 3:6], p) < 0, 1, -1).astype(np.int32)
    return counted, sign


def _slab(osc, rays6, node):
    nd = osc.nodes[node]
    return oracle.kat_slab(rays6, np.concatenate([nd["bmin"], nd["bmax"]], axis=1))


def crossings(osc, org, dirs, tmin=0.0, tmax=INF, depth=None):
    """drt.h "crossings of a ray": Crossings(count uint32 [n], winding int32 [n]).  depth: an int64 [n] array that receives the largest
    number of stack entries each ray held."""
    n = len(org)
    rays6 = _f32(np.concatenate([_f32(org).reshape(-1, 3), _f32(dirs).reshape(-1, 3)], axis=1))
    tmin, tmax = _f32(np.broadcast_to(np.float32(tmin), n)), _f32(np.broadcast_to(np.float32(tmax), n))
    count, winding = np.zeros(n, np.uint32), np.zeros(n, np.int32)
    if len(osc.nodes) == 0 or n == 0:
        return Crossings(count, winding)
    root = len(osc.nodes) - 1
    with np.errstate(invalid="ignore"):
        d = _slab(osc, rays6, np.full(n, root))
        sp = np.where((d < 0) | (d > tmax), 0, 1)                               # the root is skipped if d < 0 || d > tmax
    st = np.zeros((n, MAX_STACK), np.int64)
    st[:, 0] = root
    while True:
        if depth is not None:
            np.maximum(depth, sp, out=depth)
        act = np.nonzero(sp > 0)[0]
        if len(act) == 0:
            break
        sp[act] -= 1
        node = st[act, sp[act]]
        leaf = osc.nodes["is_leaf"][node] != 0
        la, ln = act[leaf], node[leaf]
        start, cnt = osc.nodes["prim_start"][ln], osc.nodes["prim_count"][ln]
        for k in range(int(cnt.max()) if len(ln) else 0):                      # every triangle of the leaf: no early exit
            sel = cnt > k
            r, prim = la[sel], (start[sel] + k).astype(np.int64)
            counted, sign = _pairs(osc, rays6[r], prim, tmin[r], tmax[r])
            np.add.at(count, r[counted], 1)
            np.add.at(winding, r[counted], sign[counted])
        ia, inode = act[~leaf], node[~leaf]
        if len(ia):
            c1, c2 = osc.nodes["child1"][inode], osc.nodes["child2"][inode]
            with np.errstate(invalid="ignore"):
                h1, h2 = _slab(osc, rays6[ia], c1), _slab(osc, rays6[ia], c2)
                p1 = (h1 >= 0) & ~(h1 > tmax[ia])                               # a child is pushed iff d >= 0 && !(d > tmax)
                p2 = (h2 >= 0) & ~(h2 > tmax[ia])
                far1 = h1 > h2                                                  # the farther child first
            for push, c in ((np.where(far1, p1, p2), np.where(far1, c1, c2)), (np.where(far1, p2, p1), np.where(far1, c2, c1))):
                r = ia[push]
                st[r, sp[r]] = c[push]
                sp[r] += 1
    return Crossings(count, winding)


def brute_force(osc, org, dirs, tmin=0.0, tmax=INF, chunk=512):
    """The per-pair rule over ALL triangles, no boxes: Crossings(count, winding)."""
    n, T = len(org), len(osc.tris)
    count, winding = np.zeros(n, np.uint32), np.zeros(n, np.int32)
    if T == 0:
        return Crossings(count, winding)
    rays6 = _f32(np.concatenate([_f32(org).reshape(-1, 3), _f32(dirs).reshape(-1, 3)], axis=1))
    tmin, tmax = _f32(np.broadcast_to(np.float32(tmin), n)), _f32(np.broadcast_to(np.float32(tmax), n))
    for s in range(0, n, chunk):
        m = len(rays6[s:s + chunk])
        counted, sign = _pairs(osc, np.repeat(rays6[s:s + chunk], T, axis=0), np.tile(np.arange(T), m), np.repeat(tmin[s:s + chunk], T),
                               np.repeat(tmax[s:s + chunk], T))
        counted, sign = counted.reshape(m, T), sign.reshape(m, T)
        count[s:s + chunk] = counted.sum(axis=1)
        winding[s:s + chunk] = np.where(counted, sign, 0).sum(axis=1)
    return Crossings(count, winding)


def votes(osc, points, rule="parity", count_rays=crossings):
    """drt.h "inside vote": uint8 [n], the number of the three rays that vote inside.  count_rays: crossings or brute_force."""
    p = _f32(points)[:, :3]
    out = np.zeros(len(p), np.uint8)
    for d in DIRS:
        c = count_rays(osc, p, np.tile(d, (len(p), 1)), np.float32(0), INF)
        out += ((c.winding != 0) if RULES[rule] else (c.count & 1) != 0).astype(np.uint8)
    return out


def inside(osc, points, rule="parity", count_rays=crossings):
    return votes(osc, points, rule, count_rays) >= 2


def signed_distance(osc, points, max_dist=np.inf, rule="parity", g=None):
    """drt.h "signed distance": nearest_ref.nearest's record with side = -1 inside, +1 outside, miss records included."""
    near = nr.nearest(nr.from_oracle(osc) if g is None else g, points, max_dist)
    return near._replace(side=np.where(inside(osc, points, rule), np.float32(-1), np.float32(1)).astype(np.float32))


# ---------------------------------------------------------------- scenes shared by the CPU and GPU tests

def product_scene(sc):
    """A product host scene (after a build, after a refit) as a scene of this module: its nodes and its triangles' positions."""
    tris = np.zeros(len(sc.m_PrimitivesBuffer), [("p", "<f4", (3, 3))])
    tris["p"] = sc.m_PrimitivesBuffer["vertex"]["position"]
    return types.SimpleNamespace(nodes=rf.oracle_tree(sc.m_BVHNodes), tris=tris)


def streams(pos):
    """(pos, nrm, uv, mat, materials, textures) of triangles pos [n, 3, 3], as ray_query_ref.soup gives them: geometric normals,
    one material."""
    pos = _f32(pos).reshape(-1, 3, 3)
    fn = np.cross(pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0])
    fn = (fn / np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-30)).astype(np.float32)
    n = len(pos)
    return pos, np.repeat(fn[:, None], 3, axis=1), np.zeros((n, 3, 2), np.float32), np.zeros(n, np.int32), [((0.8, 0.8, 0.8), -1)], []


def oracle_scene(pos, leaf, bins=8):
    s = streams(pos)
    return oracle.Scene(rf.triangles(*s[:4]), s[4], s[5]).build_bvh(leaf, bins)


def _quads(grid):
    """Triangles of a [m, n, 3] grid of points closed in both directions (a torus's topology): (a, b, c), (a, c, d) per quad."""
    a, b = grid, np.roll(grid, -1, axis=0)
    c, d = np.roll(b, -1, axis=1), np.roll(grid, -1, axis=1)
    return np.concatenate([np.stack([a, b, c], axis=2).reshape(-1, 3, 3), np.stack([a, c, d], axis=2).reshape(-1, 3, 3)])


def cube(h=1.0):
    """[-h, h]^3, 12 triangles, outward oriented (e1 x e2 points out)."""
    v = np.float32([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)])         # index = 4 x + 2 y + z
    faces = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return _f32([v[[q[i] for i in idx]] for q in faces for idx in ((0, 1, 2), (0, 2, 3))])


def torus(R=1.0, r=0.4, nu=32, nv=16):
    """Axis z, nu x nv quads (1 024 triangles by default), outward oriented."""
    u = (np.arange(nu) * (2 * np.pi / nu))[:, None]
    v = (np.arange(nv) * (2 * np.pi / nv))[None, :]
    grid = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v) + 0 * u], axis=2)
    return _f32(_quads(grid))


def torus_distance(p, R=1.0, r=0.4):
    """Signed analytic distance (float64): negative inside."""
    p = np.asarray(p, np.float64)
    return np.hypot(np.hypot(p[:, 0], p[:, 1]) - R, p[:, 2]) - r


def sphere(levels=3):
    """An octahedron subdivided `levels` times onto the unit sphere (8 x 4^levels triangles), outward oriented."""
    x, y, z = np.eye(3)
    tris = [(sx * x, sy * y, sz * z) if sx * sy * sz > 0 else (sx * x, sz * z, sy * y) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    t = np.array(tris, np.float64)
    for _ in range(levels):
        a, b, c = t[:, 0], t[:, 1], t[:, 2]
        ab, bc, ca = [(m / np.linalg.norm(m, axis=1, keepdims=True)) for m in (a + b, b + c, c + a)]
        t = np.concatenate([np.stack(q, axis=1) for q in ((a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca))])
    return _f32(t)


def sphere_distance(p):
    return np.linalg.norm(np.asarray(p, np.float64), axis=1) - 1.0


def wedge():
    """A thin prism with dyadic coordinates: faces y = +x/8 and y = -x/8 meet in an edge on the z axis (x = 0 .. 1, z = 0 .. 1),
    closed by the back face x = 1 and two caps; outward oriented.  The two long faces come first: their four triangles are the
    ones the edge belongs to."""
    a0, a1 = (0, 0, 0), (0, 0, 1)                                   # the edge
    t0, t1 = (1, 0.125, 0), (1, 0.125, 1)                           # top face y = x/8
    b0, b1 = (1, -0.125, 0), (1, -0.125, 1)                         # bottom face y = -x/8
    tris = [(a0, a1, t1), (a0, t1, t0),                             # top: normal (-1/8, 1, 0) up to scale
            (a0, b1, a1), (a0, b0, b1),                             # bottom: normal (-1/8, -1, 0)
            (t0, t1, b1), (t0, b1, b0),                             # back: +x
            (a0, t0, b0), (a1, b1, t1)]                             # caps: -z, +z
    return _f32(tris)


WEDGE_POINTS = np.float32([[-1 / 16, 1 / 64, 1 / 2], [-1 / 16, -1 / 64, 1 / 2]])      # outside, just beyond the edge, mirror images


def mesh_is_closed_and_outward(pos):
    """Every directed edge has its reverse exactly once, and the signed volume is positive."""
    pos = np.asarray(pos, np.float64)
    keys = {}
    for t in pos:
        for i in range(3):
            e = (tuple(t[i]), tuple(t[(i + 1) % 3]))
            keys[e] = keys.get(e, 0) + 1
    closed = all(n == 1 and keys.get((b, a), 0) == 1 for (a, b), n in keys.items())
    volume = np.einsum("ij,ij->i", pos[:, 0], np.cross(pos[:, 1], pos[:, 2])).sum() / 6
    return closed and volume > 0
