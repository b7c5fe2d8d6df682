"""The meshes of the mesh-topology tests (tests/test_topology_ref.py, tests/test_topology_abi.py, tests/test_gpu_topology.py): the
smallest ones on which each phase can go wrong.  tests/contour_scenes.py's meshes are used as they are; the new ones:

  corner_pair   two triangles that share one vertex only: two shells, and two loops of three that must not merge (the rotation about
                the shared vertex has to stay inside its own triangle)
  two_fans      two fans of three triangles that meet at their common centre and nowhere else: two shells, two loops of five that both
                pass through the centre
  open_fan      a closed fan of valence 16 with one triangle removed: the record that ends at the centre rotates through 14 twins
  strip         a straight strip of 4 096 triangles in shuffled load order: one shell of the largest diameter a mesh of its size can
                have, and one closed loop of 4 098 records
and from contour_scenes: single, quad, tetrahedron, cube, two_cubes, hollow_box (sides 4 and 2: volumes +64 and -8), book,
flipped_quad, ring (the band of 2 500 quads: one shell, two closed loops of 2 500 records), cornell_box, soup, degenerate.
"""
import numpy as np

from tests import contour_scenes as cs

FAN_VALENCE = 16
STRIP_QUADS = 2048
CORNER_PAIR = np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 0, 0], [-1, 0, 0], [0, -1, 0]]])
NEW_NAMES = ("corner_pair", "two_fans", "open_fan", "strip")
CPU_NAMES = ("single", "quad", "tetrahedron", "cube", "two_cubes", "hollow_box", "book", "flipped_quad", "corner_pair", "two_fans", "open_fan",
             "ring", "strip")
ALL_NAMES = CPU_NAMES + ("cornell_box", "soup", "degenerate")
_cache = {}


def fan(centre, rim):
    """The triangles (centre, rim[i], rim[i + 1]): [len(rim) - 1, 3, 3]."""
    centre, rim = np.float32(centre), np.float32(rim)
    return np.float32([[centre, rim[i], rim[i + 1]] for i in range(len(rim) - 1)])


def two_fans():
    up = fan((0, 0, 0), [(2, 1, 0), (1, 2, 0), (-1, 2, 0), (-2, 1, 0)])
    down = fan((0, 0, 0), [(-2, -1, 0), (-1, -2, 0), (1, -2, 0), (2, -1, 0)])
    return np.concatenate([up, down])


def open_fan(valence=FAN_VALENCE):
    a = np.arange(valence) * (2 * np.pi / valence)
    rim = np.stack([4 * np.cos(a), 4 * np.sin(a), np.zeros(valence)], axis=1).astype(np.float32)
    return fan((0, 0, 1), rim)                                               # valence - 1 triangles: the one back to rim[0] is missing


def strip(quads=STRIP_QUADS, seed=11):
    """Quad i is (i, 0, 0), (i + 1, 0, 0), (i + 1, 1, 0), (i, 1, 0) as two counter-clockwise triangles; shuffled load order."""
    i = np.arange(quads, dtype=np.float32)
    at = lambda x, y: np.stack([x, np.full(quads, y, np.float32), np.zeros(quads, np.float32)], axis=1)
    pos = np.concatenate([np.stack([at(i, 0), at(i + 1, 0), at(i, 1)], axis=1), np.stack([at(i + 1, 0), at(i + 1, 1), at(i, 1)], axis=1)]).astype(np.float32)
    return pos[np.random.default_rng(seed).permutation(len(pos))]


def positions(name):
    """The load-order positions of a programmatic mesh."""
    new = {"corner_pair": lambda: CORNER_PAIR, "two_fans": two_fans, "open_fan": open_fan, "strip": strip}
    return new[name]() if name in new else cs.positions(name)


def scene(drt, name):
    """The product scene with its tree, built once."""
    if name not in NEW_NAMES:
        return cs.scene(drt, name)[0]
    if name not in _cache:
        _cache[name] = cs.flat_scene(drt, positions(name), leaf=2 if name in ("corner_pair", "two_fans") else 4)[0]
    return _cache[name]


def empty_scene(drt):
    sc = drt.Scene()
    sc.addMaterial(*cs.ONE_MATERIAL[0])
    sc.setGeometry(np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 2), np.float32), np.zeros(0, np.int32))
    drt.BVHBuilder().buildIterative(sc)
    return sc


tree_positions = cs.tree_positions
