"""Restatement of the mesh topology (include/drt.h "mesh topology": drt_renderer_shell_labels, drt_renderer_boundary_loops and
drt_renderer_shell_terms) for the tests: a union-find over the twin pairs of tests/contour_ref.py's dictionary adjacency, a sequential
walk for the loops, and the term expression in numpy.  No tests of its own (tests/test_topology_ref.py asserts what it does).  Written
from the header; it shares no code with the product.
"""
import math

import numpy as np

from tests.contour_ref import LINKED, NON_MANIFOLD

SLOT = np.dtype([("half_edge", "<u4"), ("first", "<u4"), ("length", "<u4"), ("flags", "<u4")])     # drt_loop_slot, 16 bytes
assert SLOT.itemsize == 16
TERM = np.dtype([("c", "<f8", 3), ("w", "<f8")])                                                   # drt_shell_term, 32 bytes
assert TERM.itemsize == 32
UNTOUCHED = np.uint32(0xFFFFFFB3)                                                                   # (-77: what the tests fill buffers with)


def labels(adj):
    """drt.h "shells": int32 [n], the smallest triangle index of each triangle's component under the twin pairs of adj [3 n]."""
    adj = np.asarray(adj).reshape(-1)
    n = len(adj) // 3
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for h in np.nonzero(adj >= 0)[0]:
        a, b = find(int(h) // 3), find(int(adj[h]) // 3)
        if a != b:
            parent[max(a, b)] = min(a, b)                                  # the smaller root stays a root: a root is its component's minimum
    return np.array([find(t) for t in range(n)], np.int32)


def counts(adj, label):
    """uint32 [3]: shells, open half-edges, bad half-edges."""
    adj = np.asarray(adj).reshape(-1)
    return np.array([(label == np.arange(len(label))).sum(), (adj == -1).sum(), (adj == -2).sum()], np.uint32)


def per_shell(adj, label):
    """(index int32 [n], triangles, open_edges, bad_edges int32 [S], watertight bool [S]): the dense shell numbers in ascending order of
    label and the per-shell counts."""
    adj = np.asarray(adj).reshape(-1, 3)
    roots = np.unique(label)
    index = np.searchsorted(roots, label).astype(np.int32)
    tri = np.bincount(index, minlength=len(roots)).astype(np.int32)
    open_edges = np.bincount(index, weights=(adj == -1).sum(axis=1), minlength=len(roots)).astype(np.int32)
    bad_edges = np.bincount(index, weights=(adj == -2).sum(axis=1), minlength=len(roots)).astype(np.int32)
    return index, tri, open_edges, bad_edges, (open_edges == 0) & (bad_edges == 0)


def successor(adj, h):
    """drt.h "successor": (the boundary half-edge that follows h, LINKED) or (None, NON_MANIFOLD); the number of steps is returned too."""
    t, e = divmod(int(h), 3)
    g = 3 * t + (e + 1) % 3
    steps = 0
    while adj[g] >= 0:
        t2, e2 = divmod(int(adj[g]), 3)
        g = 3 * t2 + (e2 + 1) % 3
        steps += 1
        assert steps <= len(adj), "the rotation cycles: the twins do not pair half-edges one to one"
    return (g, LINKED, steps) if adj[g] == -1 else (None, NON_MANIFOLD, steps)


def loops(adj):
    """drt.h "boundary loops": (slots SLOT [records], counts uint32 [3] = records, loops, closed loops)."""
    adj = np.asarray(adj).reshape(-1)
    records = [int(h) for h in np.nonzero(adj == -1)[0]]
    succ, status, pred = {}, {}, {}
    for h in records:
        g, why, _ = successor(adj, h)
        status[h] = why
        if g is not None:
            assert g not in pred                                           # succ is injective
            succ[h], pred[g] = g, h
    found, seen = [], set()

    def walk(h, closed):
        members = []
        while h is not None and h not in seen:
            seen.add(h)
            members.append(h)
            h = succ.get(h)
        found.append((members, closed))

    for h in records:                                                      # a path starts at its record without a predecessor
        if h not in pred:
            walk(h, False)
    for h in records:                                                      # what is left lies on cycles: each starts at its smallest h
        if h not in seen:
            walk(h, True)
    found.sort(key=lambda c: c[0][0])                                      # by the first record
    slots = np.zeros(len(records), SLOT)
    pos = 0
    for members, closed in found:
        first = pos
        for h in members:
            slots[pos] = (h, first, len(members), int(closed) | (status[h] << 1))
            pos += 1
    return slots, np.array([len(records), len(found), sum(1 for _, c in found if c)], np.uint32)


def loop_lists(slots):
    """[(half-edges in order, closed)] read off the slots."""
    out, pos = [], 0
    while pos < len(slots):
        length = int(slots["length"][pos])
        assert slots["first"][pos] == pos and (slots["first"][pos:pos + length] == pos).all()
        out.append(([int(h) for h in slots["half_edge"][pos:pos + length]], bool(slots["flags"][pos] & 1)))
        pos += length
    return out


def hot_words(hot):
    """(v0, e1, e2) float32 [n, 3] each, from TriHot records uint8 [n, 48] (Scene.debugPack / Renderer.debugReadDeviceScene)."""
    f = np.ascontiguousarray(hot).view(np.float32).reshape(-1, 12)
    return f[:, 0:3], f[:, 3:6], f[:, 6:9]


def terms(v0, e1, e2):
    """drt.h "measure terms": TERM [n] from float32 v0, e1, e2 [n, 3], every product and sum a float64 operation of its own."""
    v0, e1, e2 = (np.asarray(a, np.float32).astype(np.float64) for a in (v0, e1, e2))
    out = np.zeros(len(v0), TERM)
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    out["c"][:, 0], out["c"][:, 1], out["c"][:, 2] = cx, cy, cz
    out["w"] = (v0[:, 0] * cx + v0[:, 1] * cy) + v0[:, 2] * cz
    return out


def packed(pos):
    """(v0, e1, e2) as the scene packs positions [n, 3, 3]: e1 = v1 - v0 and e2 = v2 - v0 in float32."""
    pos = np.asarray(pos, np.float32)
    return pos[:, 0], (pos[:, 1] - pos[:, 0]).astype(np.float32), (pos[:, 2] - pos[:, 0]).astype(np.float32)


def measures(term, index, n_shells):
    """(area, volume, area_vector, area mass, volume mass, vector mass) per shell in float64, shell by shell: area = 0.5 * sum |c|,
    volume = sum w / 6, area_vector = 0.5 * sum c; the masses are the same sums over absolute values.  Every sum is math.fsum: the
    exact sum of the terms, rounded once."""
    area, volume, vector = np.zeros(n_shells), np.zeros(n_shells), np.zeros((n_shells, 3))
    m_volume, m_vector = np.zeros(n_shells), np.zeros((n_shells, 3))
    c, w = term["c"], term["w"]
    length = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
    order = np.argsort(index, kind="stable")
    at = np.concatenate([[0], np.cumsum(np.bincount(index, minlength=n_shells))])
    for s in range(n_shells):
        mine = order[at[s]:at[s + 1]]
        area[s] = 0.5 * math.fsum(length[mine])
        volume[s] = math.fsum(w[mine]) / 6.0
        m_volume[s] = math.fsum(np.abs(w[mine])) / 6.0
        for k in range(3):
            vector[s, k] = 0.5 * math.fsum(c[mine, k])
            m_vector[s, k] = 0.5 * math.fsum(np.abs(c[mine, k]))
    return area, volume, vector, area.copy(), m_volume, m_vector
