"""Two small meshes for the self-intersection tests (tests/test_tri_overlap_ref.py, tests/test_gpu_tri_overlap.py), with the expected
pairs derived by hand.  Integer coordinates: every product of the rule is exact.  No tests of its own.

CROSSING_QUADS, in load order:
  0: A0 = (-2, -2, 0), (2, -2, 0), (2, 2, 0)       the square [-2, 2]^2 in the plane z = 0, below its diagonal: y <= x
  1: A1 = (-2, -2, 0), (2, 2, 0), (-2, 2, 0)       ... above its diagonal: y >= x
  2: B0 = (1, -1, -1), (1, 1, -1), (1, 1, 1)       the square y, z in [-1, 1] in the plane x = 1, below its diagonal: z <= y
  3: B1 = (1, -1, -1), (1, 1, 1), (1, -1, 1)       ... above its diagonal: z >= y
The two planes meet in the line x = 1, z = 0; the square B crosses z = 0 in the segment S: x = 1, -1 <= y <= 1.
  B0 holds the part of S with 0 <= y (z = 0 <= y), B1 the part with y <= 0.
  A0 holds all of S (y <= 1 = x).  A1 holds only its end (1, 1, 0), on A's diagonal (y >= x = 1): a touch, and touching counts.
  (1, 1, 0) lies on B0's edge y = 1 and not in B1 (z = 0 >= y = 1 fails).
So A0-B0 cut, A0-B1 cut, A1-B0 touch, A1-B1 are apart; A0-A1 and B0-B1 touch along their diagonals but share two vertex positions
and are dropped: the pairs are (0, 2), (0, 3), (1, 2).

TETRAHEDRON: the four faces of a closed tetrahedron.  Any two faces share an edge, so every touching pair shares vertex positions
and none is reported.
"""
import numpy as np

CROSSING_QUADS = np.float32([[[-2, -2, 0], [2, -2, 0], [2, 2, 0]], [[-2, -2, 0], [2, 2, 0], [-2, 2, 0]],
                             [[1, -1, -1], [1, 1, -1], [1, 1, 1]], [[1, -1, -1], [1, 1, 1], [1, -1, 1]]])
CROSSING_PAIRS = [(0, 2), (0, 3), (1, 2)]

_V = np.float32([[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 4]])
TETRAHEDRON = np.float32([[_V[0], _V[2], _V[1]], [_V[0], _V[1], _V[3]], [_V[0], _V[3], _V[2]], [_V[1], _V[2], _V[3]]])
