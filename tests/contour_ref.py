"""Restatement of the section contours (include/drt.h "section contours": drt_scene_edge_adjacency and drt_renderer_chain_sections) for
the tests: a dictionary for the adjacency and a sequential walk for the chains.  No tests of its own (tests/test_contour_ref.py asserts
what it does).  Written from the header; it shares no code with the product.
"""
import numpy as np

SLOT = np.dtype([("seg", "<u4"), ("first", "<u4"), ("length", "<u4"), ("flags", "<u4")])           # drt_chain_slot, 16 bytes
assert SLOT.itemsize == 16
LINKED, BOUNDARY, NON_MANIFOLD, NOT_LISTED, OTHER_EDGES, MISS = range(6)                           # a record's exit status
UNTOUCHED = np.uint32(0xFFFFFFB3)                                                                   # (-77: what the tests fill buffers with)


def adjacency(positions):
    """drt.h "edge adjacency" for positions [n, 3, 3] float32 in tree order: int32 [3 n].  Half-edge 3 t + e runs from vertex e to
    vertex (e + 1) % 3; positions are the same iff their bytes are."""
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3, 3)
    groups = {}
    for t in range(len(pos)):
        for e in range(3):
            a, b = pos[t, e].tobytes(), pos[t, (e + 1) % 3].tobytes()
            groups.setdefault(frozenset((a, b)), []).append((3 * t + e, a))
    adj = np.full(3 * len(pos), -2, np.int32)
    for ends, members in groups.items():
        if len(ends) == 1:
            continue                                                       # both ends the same position: -2
        if len(members) == 1:
            adj[members[0][0]] = -1                                        # a boundary edge
        elif len(members) == 2 and members[0][1] != members[1][1]:         # two that run in opposite directions: twins
            adj[members[0][0]], adj[members[1][0]] = members[1][0], members[0][0]
    return adj


def plane_range(splits, i, total):
    """drt.h "inputs": the clamped range of plane i."""
    lo, end = int(splits[i]), int(splits[i + 1])
    cap = end - lo if end > lo else 0
    cap = 0 if lo >= total else min(cap, total - lo)
    return lo, lo + cap


def edges(code):
    """(in, out): the edges a record with this code is entered and left through."""
    k, up = code & 3, code >> 2
    return (k, (k + 2) % 3) if up else ((k + 2) % 3, k)


def successors(adj, rec, lo, hi):
    """drt.h "link" for the records lo:hi of one plane: (succ {j: m}, status {j: 1..5} of the records without a successor)."""
    where = {int(rec["prim"][m]): m for m in range(lo, hi) if rec["prim"][m] >= 0}
    succ, status = {}, {}
    for j in range(lo, hi):
        prim = int(rec["prim"][j])
        if prim < 0:
            status[j] = MISS
            continue
        a = int(adj[3 * prim + edges(int(rec["code"][j]))[1]])
        if a == -1:
            status[j] = BOUNDARY
        elif a == -2:
            status[j] = NON_MANIFOLD
        elif a // 3 not in where:
            status[j] = NOT_LISTED
        else:
            m = where[a // 3]
            if 3 * (a // 3) + edges(int(rec["code"][m]))[0] == a:
                succ[j] = m
            else:
                status[j] = OTHER_EDGES
    return succ, status


def chain(adj, rec, splits, total=None):
    """drt.h "canonical order": (slots SLOT [total], chains uint32 [n, 2]) for section records `rec` (prim and code are read) whose
    plane i owns rec[splits[i]:splits[i + 1]].  Slots outside every range hold UNTOUCHED in every word."""
    total = len(rec) if total is None else total
    n = len(splits) - 1
    slots = np.zeros(total, SLOT)
    for f in SLOT.names:
        slots[f] = UNTOUCHED
    chains = np.zeros((n, 2), np.uint32)
    for i in range(n):
        lo, hi = plane_range(splits, i, total)
        succ, status = successors(adj, rec, lo, hi)
        pred = {}
        for j, m in succ.items():
            assert m not in pred                                           # the link is injective
            pred[m] = j
        found, seen = [], set()

        def walk(j, closed):
            members = []
            while j is not None and j not in seen:
                seen.add(j)
                members.append(j)
                j = succ.get(j)
            found.append((members, closed))

        live = [j for j in range(lo, hi) if status.get(j) != MISS]
        for j in live:                                                     # a path starts at its record without a predecessor
            if j not in pred:
                walk(j, False)
        for j in live:                                                     # what is left lies on cycles: each starts at its smallest index
            if j not in seen:
                walk(j, True)
        found.sort(key=lambda c: c[0][0])                                  # by the ascending index of the first record
        pos = lo
        for members, closed in found:
            first = pos
            for j in members:
                slots[pos] = (j, first, len(members), int(closed) | (status.get(j, LINKED) << 1))
                pos += 1
        chains[i] = (len(found), sum(1 for _, closed in found if closed))
        for j in range(lo, hi):                                            # miss records stay where they are, after all chains
            if status.get(j) == MISS:
                assert j >= pos, "a miss record in front of a cut triangle: not what a fill writes"
                slots[j] = (j, j, 1, MISS << 1)
    return slots, chains


def chain_lists(slots, chains, splits, total=None):
    """The chains as lists: [plane][chain] = (record indices in order, closed)."""
    total = len(slots) if total is None else total
    out = []
    for i in range(len(splits) - 1):
        lo, hi = plane_range(splits, i, total)
        mine, pos = [], lo
        while pos < hi and (slots["flags"][pos] >> 1) != MISS:
            length = int(slots["length"][pos])
            assert slots["first"][pos] == pos
            mine.append(([int(s) for s in slots["seg"][pos:pos + length]], bool(slots["flags"][pos] & 1)))
            pos += length
        assert len(mine) == chains[i][0] and sum(c for _, c in mine) == chains[i][1]
        out.append(mine)
    return out


def areas(planes, rec, slots, chains, splits):
    """drt.h: 0.5 * sum dot(n / |n|, cross(p, q)) over every closed chain, in float64, chain by chain; NaN for an open one.  Also the
    mass 0.5 * sum |products| of every chain."""
    out, mass = [], []
    for i, mine in enumerate(chain_lists(slots, chains, splits)):
        nn = np.asarray(planes[i][0:3], np.float64)
        length = np.sqrt((nn * nn).sum())
        unit = nn / length if length > 0 else np.zeros(3)
        for members, closed in mine:
            terms = np.cross(rec["p"][members].astype(np.float64), rec["q"][members].astype(np.float64)) * unit
            out.append(0.5 * terms.sum(axis=1).sum() if closed else np.nan)
            mass.append(0.5 * np.abs(terms).sum())
    return np.array(out, np.float64), np.array(mass, np.float64)
