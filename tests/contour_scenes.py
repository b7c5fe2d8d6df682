"""The meshes of the section-contour tests (tests/test_contour_ref.py, tests/test_contour_abi.py, tests/test_gpu_contour.py), all small
and built through ray_query_ref.programmatic_scene, and the planes that cut them.

  single, quad, tetrahedron   the section tests' (one open chain of one, one of two, closed chains of three)
  cube                        models/cube.gltf
  two_cubes                   two disjoint boxes: a plane across both gives two closed chains
  hollow_box                  an outward box round an inward one: two closed chains in one plane whose areas have opposite signs
  book                        three triangles on one edge: that edge is non-manifold (status 2)
  flipped_quad                the quad with one triangle's winding reversed: the shared edge runs the same way twice (status 2)
  ring                        a band of 2 500 quads (5 000 triangles) between a ring at z = -1 and one at z = +1, in shuffled load order:
                              the plane z = 0 gives ONE closed chain of 5 000 records, which takes 13 jumping rounds.  Its coordinates
                              are multiples of 2^-8 below 32, so e1 = v1 - v0 and v0 + e1 are exact and neighbours classify alike.
  soup, fan, cornell_box      the section tests' (mostly chains of one; a fan whose triangles share no edge; a real scene)
  degenerate                  hostile_meshes.degenerate(): duplicates, zero-length edges, shared edges
"""
import os

import numpy as np

import oracle
from tests import hostile_meshes as hm
from tests import nearest_ref as nr
from tests import ray_query_ref as rq
from tests import section_ref as sr
from tests.scenes import MODELS, scene_path
from tests.tri_overlap_scenes import TETRAHEDRON

ONE_MATERIAL = [((0.8, 0.8, 0.8), -1)]
SINGLE = np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
QUAD = np.float32([[[0, 0, 0], [1, 0, 0], [1, 1, 0]], [[0, 0, 0], [1, 1, 0], [0, 1, 0]]])
FLIPPED_QUAD = np.float32([[[0, 0, 0], [1, 0, 0], [1, 1, 0]], [[0, 0, 0], [0, 1, 0], [1, 1, 0]]])
BOOK = np.float32([[[0, 0, -1], [0, 0, 1], [1, 0, 0]], [[0, 0, -1], [0, 0, 1], [-1, 1, 0]], [[0, 0, 1], [0, 0, -1], [-1, -1, 0]]])
EXACT_CLOSED = ("tetrahedron", "two_cubes", "hollow_box", "ring")          # closed meshes with exact coordinates: every chain closes
CPU_NAMES = ("single", "quad", "tetrahedron", "cube", "two_cubes", "hollow_box", "book", "flipped_quad", "ring")
ALL_NAMES = CPU_NAMES + ("cornell_box", "soup", "fan", "degenerate")
RING_QUADS = 2500
_cache = {}


def box(lo, hi, inward=False):
    """The twelve triangles of an axis box, faces outward (counter-clockwise seen from outside) or inward: [12, 3, 3]."""
    lo, hi = np.float32(lo), np.float32(hi)
    c = np.float32([[x, y, z] for z in (lo[2], hi[2]) for y in (lo[1], hi[1]) for x in (lo[0], hi[0])])      # corner = x + 2 y + 4 z
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]              # -z +z -y +y -x +x
    tris = []
    for a, b, cc, d in quads:
        tris += [[c[a], c[b], c[cc]], [c[a], c[cc], c[d]]]
    tris = np.float32(tris)
    return tris[:, ::-1].copy() if inward else tris


def ring(quads=RING_QUADS, radius=16.0, seed=7):
    """The band, in shuffled load order: [2 * quads, 3, 3], every coordinate a multiple of 2^-8."""
    a = np.arange(quads) * (2 * np.pi / quads)
    xy = (np.round(np.stack([radius * np.cos(a), radius * np.sin(a)], axis=1) * 256) / 256).astype(np.float32)
    assert len({p.tobytes() for p in xy}) == quads                           # the ring's points are distinct
    nxt = np.roll(xy, -1, axis=0)
    low = lambda p: np.concatenate([p, np.full((quads, 1), -1, np.float32)], axis=1)
    top = lambda p: np.concatenate([p, np.full((quads, 1), 1, np.float32)], axis=1)
    pos = np.concatenate([np.stack([low(xy), low(nxt), top(nxt)], axis=1), np.stack([low(xy), top(nxt), top(xy)], axis=1)]).astype(np.float32)
    return pos[np.random.default_rng(seed).permutation(len(pos))]


def fan(n=300):
    """n triangles round the z axis that share no edge: the plane z = 0 cuts every one of them (the section tests' fan)."""
    a = (np.arange(n, dtype=np.float32) * np.float32(2 * np.pi / n)).astype(np.float32)
    b = (a + np.float32(np.pi / n)).astype(np.float32)
    r = np.float32(1) + (np.arange(n) % 7).astype(np.float32) * np.float32(0.25)
    pos = np.zeros((n, 3, 3), np.float32)
    pos[:, 0] = np.stack([r * np.cos(a), r * np.sin(a), np.full(n, -1, np.float32)], axis=1)
    pos[:, 1] = np.stack([r * np.cos(b), r * np.sin(b), np.full(n, -1, np.float32)], axis=1)
    pos[:, 2] = np.stack([(r + 1) * np.cos(a), (r + 1) * np.sin(a), np.full(n, 1, np.float32)], axis=1)
    return pos


def positions(name):
    """The load-order positions of a programmatic mesh."""
    return {"single": lambda: SINGLE, "quad": lambda: QUAD, "tetrahedron": lambda: TETRAHEDRON, "flipped_quad": lambda: FLIPPED_QUAD,
            "book": lambda: BOOK, "two_cubes": lambda: np.concatenate([box((0, 0, 0), (1, 1, 1)), box((2, 0.25, 0.5), (3, 1.25, 2))]),
            "hollow_box": lambda: np.concatenate([box((-2, -2, -2), (2, 2, 2)), box((-1, -1, -1), (1, 1, 1), inward=True)]),
            "ring": ring, "fan": fan}[name]()


def flat_scene(drt, pos, leaf=4):
    n = len(pos)
    nrm = np.tile(np.float32([0, 0, 1]), (n, 3, 1))
    return rq.programmatic_scene(drt, pos, nrm, np.zeros((n, 3, 2), np.float32), np.zeros(n, np.int32), ONE_MATERIAL, [], leaf, 8)


def scene(drt, name):
    """(product scene, Geometry with the same tree), built once."""
    if name not in _cache:
        if name in ("cube", "cornell_box"):
            sc = drt.Scene()
            sc.loadGLTFmodel(os.path.join(MODELS, "cube.gltf") if name == "cube" else scene_path(name))
            b = drt.BVHBuilder()
            b.m_TargetLeafPrimitivesCount, b.m_BinCount = (4, 8) if name == "cube" else (20, 8)
            b.buildIterative(sc)
            g = nr.from_product(sc) if name == "cube" else nr.from_oracle(oracle.Scene.load_glb(scene_path(name)).build_bvh(20, 8))
        elif name == "soup":
            sc, osc = rq.programmatic_scene(drt, *rq.soup(3000, 5), 2, 8)
            g = nr.from_oracle(osc)
        elif name == "degenerate":
            sc, osc = hm.scene_pair(drt, hm.degenerate())
            g = nr.from_oracle(osc)
        else:
            sc, osc = flat_scene(drt, positions(name), leaf=2 if name == "fan" else 4)
            g = nr.from_oracle(osc)
        _cache[name] = (sc, g)
    return _cache[name]


def tree_positions(sc):
    """[n, 3, 3]: the positions the host scene holds, in tree order."""
    return np.ascontiguousarray(sc.m_PrimitivesBuffer["vertex"]["position"], np.float32).reshape(-1, 3, 3)


def planes(name, g, count=40, seed=13):
    """Planes [N, 4] for a scene: the ones its test is about first (z = 0 and the like), then axis planes through vertices (ties:
    a vertex on the plane counts as above), random planes through the scene, a far one and n = 0."""
    rng = np.random.default_rng(seed)
    lo, hi = nr.bounds(g)
    mid = ((lo + hi) / 2).astype(np.float32)
    special = {"tetrahedron": sr.pack([(0, 0, 1), (1, 0, 0), (1, 1, 1)], [2, 1, 4]), "ring": sr.pack([(0, 0, 1), (0, 0, -1), (0, 0, 2)], [0, 0, 1]),
               "fan": sr.pack([(0, 0, 1)], [0]), "hollow_box": sr.pack([(0, 0, 1), (1, 0, 0), (0, 0, 1)], [0, 0.5, 1.5]),
               "two_cubes": sr.pack([(0, 0, 1), (0, 1, 0), (0, 0, 1)], [0.75, 0.5, 1.5]), "book": sr.pack([(0, 0, 1)], [0]),
               "quad": sr.pack([(1, 0, 0), (0, 1, 0)], [0.5, 0.25]), "flipped_quad": sr.pack([(1, 0, 0), (0, 1, 0)], [0.5, 0.25]),
               "single": sr.pack([(1, 0, 0)], [0.5])}.get(name, np.zeros((0, 4), np.float32))
    across = sr.pack([(0, 0, 1), (0.3, 1, -0.2)], [mid[2], nr.dot(np.float32([0.3, 1, -0.2]), mid)])
    if name == "ring":
        return special                                                       # (5 000 records a plane, and a band closes only across its axis)
    k = max(count // 4, 2)
    v = nr.tie_points(g, k, rng)
    axis = (np.eye(3, dtype=np.float32)[rng.integers(0, 3, k)] * np.float32(rng.choice([-1, 1], k))[:, None]).astype(np.float32)
    through = sr.pack(axis, nr.dot(axis, v))
    nn = rng.normal(size=(count - k, 3)).astype(np.float32)
    rand = sr.pack(nn, nr.dot(nn, nr.box_points(g, count - k, rng)))
    far = sr.pack([(0, 0, 1)], [hi[2] + np.float32(100)])
    return np.concatenate([special, across, through, rand, far, sr.pack([(0, 0, 0)], [0])]).astype(np.float32)


def degenerate_planes(count=150, seed=5):
    """hostile_meshes.aimed_planes for the degenerate mesh (axis planes through the thin triangles' vertices, planes that contain
    their segments and planes across them), thinned to about `count`."""
    mesh = hm.degenerate()
    osc = hm.oracle_scene(mesh)
    g = nr.from_oracle(osc)
    kind, _ = hm.kinds_in_tree_order(osc, mesh)
    aimed = hm.aimed_planes(g, kind, seed)
    return np.ascontiguousarray(aimed[::max(len(aimed) // count, 1)], np.float32)
