"""The meshes of the intersection-curve tests (tests/test_curve_ref.py, tests/test_curve_abi.py, tests/test_gpu_curve.py): a scene mesh
and a query mesh that cuts it, all small and built through contour_scenes.flat_scene.

  spheres(seed)        two UV spheres in general position: 40 x 20 segments of radius 1 as the scene, 32 x 16 of radius 0.9 at
                       (0.4, 0.3, 0.2) as the queries, a QR-random rotation on each; the poles are single shared vertices
  aligned(offset)      a 24 x 12 sphere cut by an axis-aligned displaced copy of itself: the curve runs through vertices and along edges
  tube(m)              contour_scenes.ring: a band of m quads between z = -1 and z = +1 with exact coordinates, in shuffled load order
  BIG, quad_queries()  one large triangle in the plane z = 0 (the band's section is a single loop of 2 m records) and a two-triangle
                       quad there whose diagonal crosses the band twice (the loop changes query twice)
"""
import numpy as np

from tests import contour_scenes as cs

BIG = np.float32([[[-100, -100, 0], [100, -100, 0], [0, 150, 0]]])
TUBE_SIZES = (127, 128, 129, 511, 512, 513, 1537)       # 2 m records: round a workgroup (256), a scan block (1024), three scan blocks
assert [2 * m for m in TUBE_SIZES] == [254, 256, 258, 1022, 1024, 1026, 3074] and 3074 > 3 * 1024


def uv_sphere(nu, nv, radius=1.0):
    """(vertices float64 [V, 3], triangles int [F, 3]) of a UV sphere with nu segments round the axis and nv from pole to pole, faces
    outward; each pole is one vertex."""
    rings = []
    for i in range(1, nv):
        theta = np.pi * i / nv
        phi = 2 * np.pi * np.arange(nu) / nu
        rings.append(np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.full(nu, np.cos(theta))], axis=1))
    verts = np.concatenate([[[0, 0, 1.0]]] + rings + [[[0, 0, -1.0]]]) * radius
    ring = lambda i, j: 1 + i * nu + j % nu
    top, bottom = 0, len(verts) - 1
    tris = []
    for j in range(nu):
        tris.append((top, ring(0, j), ring(0, j + 1)))
        tris.append((bottom, ring(nv - 2, j + 1), ring(nv - 2, j)))
        for i in range(nv - 2):
            a, b, c, d = ring(i, j), ring(i, j + 1), ring(i + 1, j + 1), ring(i + 1, j)
            tris += [(a, d, c), (a, c, b)]
    return verts, np.asarray(tris)


def placed(verts, tris, rotation=None, offset=(0, 0, 0)):
    """float32 [F, 3, 3]: the vertices rotated and moved in float64, rounded once, then gathered -- a shared vertex is the same bits in
    every triangle that has it."""
    v = verts if rotation is None else verts @ rotation.T
    return np.ascontiguousarray((v + np.asarray(offset, np.float64)).astype(np.float32)[tris])


def rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def spheres(seed):
    """(scene positions [1520, 3, 3], query triangles [960, 3, 3]) in general position."""
    rng = np.random.default_rng(seed)
    return placed(*uv_sphere(40, 20), rotation(rng)), placed(*uv_sphere(32, 16, 0.9), rotation(rng), (0.4, 0.3, 0.2))


def aligned(offset):
    """(scene positions, query triangles): a 24 x 12 sphere and its displaced copy."""
    v, t = uv_sphere(24, 12)
    return placed(v, t), placed(v, t, None, offset)


def tube(m):
    return cs.ring(quads=m)


def quad_queries(flip_second=False):
    """[2, 3, 3]: a quad in the plane z = 0 round the band, split along a diagonal that misses the band's vertices."""
    a, b, c, d = np.float32([[-100, -90, 0], [100, -90, 0], [100, 110, 0], [-100, 110, 0]])
    second = [a, d, c] if flip_second else [a, c, d]
    return np.float32([[a, b, c], second])


def poke():
    """[1, 3, 3]: a triangle that enters the unit sphere with one corner: the curve ends on two query edges without a twin."""
    return np.float32([[[0.1, 0.05, 0.02], [3, 0.4, 1.0], [3, -0.3, -1.1]]])


def strip():
    """(positions [4, 3, 3], query [1, 3, 3]): an open strip of two quads in the plane z = 0 and a triangle across all of it."""
    p = lambda x, y: [x, y, 0]
    pos = np.float32([[p(0, 0), p(1, 0), p(1, 1)], [p(0, 0), p(1, 1), p(0, 1)], [p(1, 0), p(2, 0), p(2, 1)], [p(1, 0), p(2, 1), p(1, 1)]])
    return pos, np.float32([[[-5, 0.375, -4], [7, 0.625, -4], [1, 0.5, 9]]])


def book_query():
    """[1, 3, 3]: a triangle across the spine of contour_scenes.BOOK, cutting all three leaves."""
    return np.float32([[[-6, -7, 0.25], [7, -6, 0.25], [0, 9, 0.125]]])


def needle():
    """[1, 3, 3]: a small triangle through the plane z = 0 whose section lies inside contour_scenes.SINGLE and across the diagonal of
    contour_scenes.QUAD: one record there, two here."""
    return np.float32([[[0.2, 0.1, -1], [0.3, 0.2, 1], [0.1, 0.4, 1]]])


SPHERE_SEEDS = (1, 2, 3)
NAMES = tuple("spheres%d" % s for s in SPHERE_SEEDS) + ("aligned_x", "aligned_z", "tube_quad", "tube_flipped", "poke", "strip", "book", "single",
                                                        "quad") + tuple("tube%d" % m for m in TUBE_SIZES)
_cache = {}


def case(name):
    """(scene positions in load order [T, 3, 3], query triangles [N, 3, 3]) of a named case, made once."""
    if name not in _cache:
        if name.startswith("spheres"):
            made = spheres(int(name[7:]))
        elif name.startswith("aligned"):
            made = aligned({"x": (0.5, 0, 0), "z": (0, 0, 0.25)}[name[-1]])
        elif name in ("tube_quad", "tube_flipped"):
            made = tube(128), quad_queries(name == "tube_flipped")
        elif name.startswith("tube"):
            made = tube(int(name[4:])), BIG
        else:
            made = {"poke": lambda: (placed(*uv_sphere(24, 12)), poke()), "strip": strip, "book": lambda: (cs.BOOK, book_query()),
                    "single": lambda: (cs.SINGLE, needle()), "quad": lambda: (cs.QUAD, needle())}[name]()
        _cache[name] = made
    return _cache[name]
