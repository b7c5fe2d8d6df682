"""include/drt.h "device edge adjacency" restated in numpy, independent of the device code: one routine over [N, 3, k] integer words
for both kinds of end (k = 3: the words of a position, k = 1: a vertex index), the numbering of the undirected edges and the boundary
vertices.  The device results are compared with these byte for byte (tests/test_gpu_adjacency.py); the restatement is checked against
the host routine in tests/test_adjacency_ref.py."""
import numpy as np


def position_words(tris):
    """uint32 [N, 3, 3]: the words of the corners of [N, 3, 3] float32 or packed [N, 12] (drt_tri) triangles."""
    t = np.ascontiguousarray(tris, np.float32)
    if t.ndim == 2 and t.shape[1] == 12:
        t = np.ascontiguousarray(t[:, 0:9])
    return t.reshape(-1, 3, 3).view(np.uint32)


def index_words(faces):
    """uint32 [N, 3, 1]: the words of an int32 [N, 3] index buffer."""
    return np.ascontiguousarray(faces, np.int32).reshape(-1, 3, 1).view(np.uint32)


def adjacency(words):
    """(adj int32 [N, 3], edge int32 [N, 3], half_edge int32 [E]) of uint32 [N, 3, k] words.  Half-edge h = 3 t + e runs from end e to
    end (e + 1) % 3.  Zero length: adj -2, edge -1.  Half-edges with the same unordered pair of ends are a group: one member gives -1,
    two that run in opposite directions are twins, everything else is -2.  A group is an edge; its representative is its smallest
    half-edge; edges are numbered in ascending representative."""
    words = np.ascontiguousarray(words, np.uint32)
    n, k = words.shape[0], words.shape[2]
    adj = np.full(3 * n, -2, np.int32)
    edge = np.full(3 * n, -1, np.int32)
    if n == 0:
        return adj.reshape(0, 3), edge.reshape(0, 3), np.zeros(0, np.int32)
    a = words.reshape(3 * n, k)
    b = np.roll(words, -1, axis=1).reshape(3 * n, k)
    differ = a != b
    live = np.flatnonzero(differ.any(axis=1))                                 # both ends the same: no group
    a, b = a[live], b[live]
    at = differ[live].argmax(axis=1)                                          # the first word that differs orders the two ends
    rows = np.arange(len(live))
    forward = a[rows, at] < b[rows, at]
    lo, hi = np.where(forward[:, None], a, b), np.where(forward[:, None], b, a)
    keys = np.ascontiguousarray(np.concatenate([lo, hi], axis=1)).view(np.dtype((np.void, 8 * k))).reshape(-1)
    _, first, inverse, counts = np.unique(keys, return_index=True, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    size = counts[inverse]
    adj[live[size == 1]] = -1
    pairs = np.flatnonzero(size == 2)
    order = pairs[np.argsort(inverse[pairs], kind="stable")]                  # the two members of a group side by side
    x, y = order[0::2], order[1::2]
    twins = forward[x] != forward[y]
    adj[live[x[twins]]], adj[live[y[twins]]] = live[y[twins]], live[x[twins]]
    by_rep = np.argsort(first, kind="stable")                                 # first: the smallest member of every group (live ascends)
    rank = np.empty(len(by_rep), np.int64)
    rank[by_rep] = np.arange(len(by_rep))
    edge[live] = rank[inverse]
    return adj.reshape(n, 3), edge.reshape(n, 3), live[first[by_rep]].astype(np.int32)


def by_position(tris):
    return adjacency(position_words(tris))


def by_index(faces):
    return adjacency(index_words(faces))


def euler(n_vertices, n_edges, n_tris):
    return int(n_vertices) - int(n_edges) + int(n_tris)


def boundary_vertices(faces, adj, n_vertices, bad=False):
    """bool [V]: a half-edge with adj == -1 (bad: or -2) starts or ends at the vertex; a triangle with an index outside [0, V) is
    skipped."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    adj = np.asarray(adj, np.int64).reshape(-1, 3)
    out = np.zeros(n_vertices, bool)
    ok = ((faces >= 0) & (faces < n_vertices)).all(axis=1)
    hit = ((adj == -1) | ((adj == -2) if bad else False)) & ok[:, None]
    out[faces[hit]] = True
    out[np.roll(faces, -1, axis=1)[hit]] = True
    return out
