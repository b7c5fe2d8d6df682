"""Restatement of the intersection curves (include/drt.h "intersection curves": drt_tri_edge_adjacency and
drt_renderer_chain_intersections) for the tests: dictionaries for the two tables and the lookups, and a sequential walk for the chains.
No tests of its own (tests/test_curve_ref.py asserts what it does).  Written from the header; it shares no code with the product.
"""
import numpy as np

from tests.contour_ref import SLOT, UNTOUCHED, plane_range  # noqa: F401  (drt_chain_slot and the clamped range are the contours')

LINKED, BOUNDARY, NON_MANIFOLD, NOT_LISTED, OTHER_EDGES, NOT_LIVE = range(6)                       # a record's exit status
EDGE_CODES = (0, 1, 2, 4, 5, 6)


def tri_adjacency(tris):
    """drt.h "edge adjacency of a query mesh" for vertices [n, 3, 3] (or packed [n, 12]) float32 in the caller's order: int32 [3 n].
    Half-edge 3 i + e runs from vertex e to vertex (e + 1) % 3; positions are the same iff their bytes are."""
    t = np.ascontiguousarray(tris, np.float32)
    pos = t[:, 0:9].reshape(-1, 3, 3) if t.ndim == 2 else t.reshape(-1, 3, 3)
    groups = {}
    for i in range(len(pos)):
        for e in range(3):
            a, b = pos[i, e].tobytes(), pos[i, (e + 1) % 3].tobytes()
            groups.setdefault(frozenset((a, b)), []).append((3 * i + e, a))
    adj = np.full(3 * len(pos), -2, np.int32)
    for ends, members in groups.items():
        if len(ends) == 1:
            continue                                                       # both ends the same position: -2
        if len(members) == 1:
            adj[members[0][0]] = -1                                        # a boundary edge
        elif len(members) == 2 and members[0][1] != members[1][1]:         # two that run in opposite directions: twins
            adj[members[0][0]], adj[members[1][0]] = members[1][0], members[0][0]
    return adj


def owner_of(splits, total, j):
    """drt.h "ranges": the binary search as if splits ascended, then the clamped range is checked.  None: no owner."""
    lo, hi = 0, len(splits) - 1
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if int(splits[mid]) <= j:
            lo = mid + 1
        else:
            hi = mid
    if lo == 0:
        return None
    a, b = plane_range(splits, lo - 1, total)
    return lo - 1 if a <= j < b else None


class _Ranges:
    """The lookups of "link": the first record of a query's range with a given prim.  A range whose prims (as unsigned) ascend is a
    dictionary; any other range is searched as the header writes the search out."""

    def __init__(self, prim, splits, total):
        self.key = np.asarray(prim, np.int64) & 0xFFFFFFFF
        self.splits, self.total = splits, total
        self.made = {}

    def first(self, i, target):
        lo, hi = plane_range(self.splits, i, self.total)
        if i not in self.made:
            keys = self.key[lo:hi]
            table = None
            if (np.diff(keys) >= 0).all():
                table = {}
                for m in range(hi - 1, lo - 1, -1):
                    table[int(self.key[m])] = m                            # the first record of every prim
            self.made[i] = table
        table = self.made[i]
        if table is not None:
            return table.get(target)
        while lo < hi:                                                     # (an unsorted range: the search as written)
            mid = lo + (hi - lo) // 2
            if self.key[mid] < target:
                lo = mid + 1
            else:
                hi = mid
        end = plane_range(self.splits, i, self.total)[1]
        return lo if lo < end and self.key[lo] == target else None


def links(adj, query_adj, prim, code, splits, total, n_tris):
    """drt.h "live records" and "link": (succ {j: m} before the claims are settled, status {j: 1..5} of the records without one)."""
    n = len(splits) - 1
    prim, code = np.asarray(prim, np.int64), np.asarray(code, np.int64)
    owner = [owner_of(splits, total, j) for j in range(total)]
    live = [owner[j] is not None and 0 <= prim[j] < n_tris and (code[j] & 15) in EDGE_CODES and (code[j] >> 4) in EDGE_CODES for j in range(total)]
    ranges = _Ranges(prim[:total], splits, total)
    succ, status = {}, {}
    for j in range(total):
        if not live[j]:
            status[j] = NOT_LIVE
            continue
        i, T, cq = owner[j], int(prim[j]), int(code[j] >> 4)
        if cq < 4:
            a = int(adj[3 * T + cq])
            query, target, entry = i, a // 3, a % 3
        else:
            a = int(query_adj[3 * i + cq - 4])
            if a >= 0 and a // 3 >= n:
                a = -2
            query, target, entry = a // 3, T, 4 + a % 3
        if a == -1:
            status[j] = BOUNDARY
        elif a < 0:
            status[j] = NON_MANIFOLD
        else:
            m = ranges.first(query, target)
            if m is None or not live[m] or owner[m] != query:
                status[j] = NOT_LISTED
            elif int(code[m] & 15) != entry:
                status[j] = OTHER_EDGES
            else:
                succ[j] = m
    return succ, status


def chain(adj, query_adj, prim, code, splits, n_tris, total=None):
    """drt.h "canonical order": (slots SLOT [total], counts uint32 [3]) for intersection records (prim and code are read) whose
    query i owns [splits[i], splits[i + 1])."""
    total = len(prim) if total is None else total
    succ, status = links(adj, query_adj, prim, code, splits, total, n_tris)
    pred = {}
    for j in sorted(succ):                                                 # of the records that claim a successor the smallest keeps it
        m = succ[j]
        if m in pred:
            status[j] = NOT_LISTED
            del succ[j]
        else:
            pred[m] = j
    found, seen = [], set()

    def walk(j, closed):
        members = []
        while j is not None and j not in seen:
            seen.add(j)
            members.append(j)
            j = succ.get(j)
        found.append((members, closed))

    for j in range(total):                                                 # a path starts at its record without a predecessor
        if j not in pred:
            walk(j, False)
    for j in range(total):                                                 # what is left lies on cycles: each starts at its smallest index
        if j not in seen:
            walk(j, True)
    found.sort(key=lambda c: c[0][0])                                      # by the ascending index of the first record
    slots = np.zeros(total, SLOT)
    pos = 0
    for members, closed in found:
        first = pos
        for j in members:
            slots[pos] = (j, first, len(members), int(closed) | (status.get(j, LINKED) << 1))
            pos += 1
    assert pos == total
    dead = sum(1 for members, _ in found if status.get(members[0]) == NOT_LIVE)
    counts = np.uint32([len(found) - dead, sum(1 for _, closed in found if closed), dead])
    return slots, counts


def chain_lists(slots):
    """The chains of live records as lists: [(record indices in order, closed, exit statuses)]."""
    out, pos = [], 0
    while pos < len(slots):
        length = int(slots["length"][pos])
        assert slots["first"][pos] == pos and (slots["first"][pos:pos + length] == pos).all() and (slots["length"][pos:pos + length] == length).all()
        status = [int(f) >> 1 for f in slots["flags"][pos:pos + length]]
        if status[0] != NOT_LIVE:
            out.append(([int(s) for s in slots["seg"][pos:pos + length]], bool(slots["flags"][pos] & 1), status))
        else:
            assert length == 1
        pos += length
    return out
