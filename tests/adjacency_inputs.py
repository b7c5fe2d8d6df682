"""The triangle soups the edge-adjacency tests share (tests/test_adjacency_ref.py on the CPU, tests/test_gpu_adjacency.py on the
device): half-edge counts around a wave, a workgroup and a trip of the scan's offsets, crowded lattices, copies of one triangle, fans
round one edge, zero-length edges, every special bit pattern, and an isosurface with and without holes."""
import numpy as np

from tests import isosurface_ref as iso

# in half-edges: 63 | 66 straddle a wave, 255 | 258 a workgroup, 4 098 sixteen workgroups, 65 535 | 65 538 one trip of the offsets
COUNTS = (1, 2, 21, 22, 85, 86, 1366, 21845, 21846)
ONE = np.float32([[0.25, -3.5, 1e-40], [1.5, 2.0, -0.0], [-7.0, 0.125, 3.0]])
_cache = {}


def distinct_soup(n, seed):
    """n triangles whose 3 n positions all differ: every entry of the table is -1"""
    t = np.random.default_rng(seed).standard_normal((n, 3, 3)).astype(np.float32)
    t[:, :, 0] += 4 * np.arange(3 * n, dtype=np.float32).reshape(n, 3)
    assert len(np.unique(t.reshape(-1, 3), axis=0)) == 3 * n
    return t


def lattice_soup(n, side, seed):
    """crowded: many triangles share an edge, and some have two or three equal corners"""
    return np.random.default_rng(seed).integers(0, side, (n, 3, 3)).astype(np.float32)


def copies(n):
    """one triangle n times: three groups of n half-edges that run the same way"""
    return np.repeat(ONE[None], n, axis=0)


def pair(reverse):
    """the triangle and itself again: reversed (twins) or the same way (-2)"""
    return np.stack([ONE, ONE[::-1] if reverse else ONE])


def fan(n):
    """n triangles round the edge (0, 0, 0) - (0, 0, 1), all running along it the same way"""
    a = np.arange(n, dtype=np.float32)
    t = np.zeros((n, 3, 3), np.float32)
    t[:, 1, 2] = 1
    t[:, 2, 0], t[:, 2, 1] = np.cos(a), np.sin(a)
    return t


def zero_length():
    """a triangle with two equal corners between two whole ones, and one with three"""
    two = ONE.copy()
    two[1] = two[0]
    return np.stack([ONE, two, ONE[::-1], np.repeat(ONE[:1], 3, axis=0)])


def special_soup(n=700, seed=9):
    """zeros of both signs, NaNs with different payloads, infinities, denormals (tests/test_gpu_weld.py's pool)"""
    pool = np.array([0x00000000, 0x80000000, 0x7FC00000, 0x7FC00001, 0xFFC00000, 0x7F800001, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001,
                     0x007FFFFF, 0x3F800000, 0x7F7FFFFF], np.uint32)
    return pool[np.random.default_rng(seed).integers(0, len(pool), (n, 3, 3))].view(np.float32)


def special_line(n=60, seed=10):
    """... in x alone, so that the 13 positions share edges: twins, boundaries and crowds that differ in a sign or a payload only"""
    t = special_soup(n, seed)
    t[:, :, 1:] = 0
    return t


def special_edges():
    """hand-made: an edge between +0 and -0 has a length in bits, NaNs of different payloads are different ends, the same NaN is one"""
    w = np.zeros((3, 3, 3), np.uint32)
    w[0, 1, 0], w[0, 2, 0] = 0x80000000, 0x3F800000                          # (+0, -0, 1): no zero-length edge
    w[1, 0, 0], w[1, 1, 0], w[1, 2, 0] = 0x80000000, 0x00000000, 0x7FC00000   # (-0, +0, NaN): the twin of the first edge
    w[2, 0, 0], w[2, 1, 0], w[2, 2, 0] = 0x7FC00000, 0x7FC00000, 0x7FC00001   # (NaN, NaN, NaN'): one zero-length edge
    return w.view(np.float32)


def sphere(res=16):
    """the restatement's isosurface of one sphere on a res^3 grid: closed, oriented, genus 0"""
    if res not in _cache:
        lo, hi = np.float32([-1.03, -1.01, -1.02]), np.float32([1.01, 1.04, 1.02])
        f, cell = iso.sphere_sdf(res, lo, hi, 0.8)
        _cache[res] = iso.triangles(iso.isosurface(f, 0.0, lo, cell)[1])
    return _cache[res].copy()


def holed_sphere(res=16, seed=5):
    """... with 10 % of its triangles removed"""
    t = sphere(res)
    keep = np.random.default_rng(seed).random(len(t)) >= 0.1
    return t[keep]


def families():
    """(name, [N, 3, 3] float32) of every family"""
    for n in COUNTS:
        yield "distinct(%d)" % n, distinct_soup(n, n)
        yield "lattice(%d)" % n, lattice_soup(n, 5, n + 1)
    for n in (64, 4096):
        yield "copies(%d)" % n, copies(n)
    yield "reversed pair", pair(True)
    yield "same-way pair", pair(False)
    for n in (3, 4, 65):
        yield "fan(%d)" % n, fan(n)
    yield "zero length", zero_length()
    yield "special", special_soup()
    yield "special line", special_line()
    yield "special edges", special_edges()
    yield "sphere", sphere()
    yield "holed sphere", holed_sphere()
