"""tests/subdivide_ref.py, the numpy restatement of include/drt.h "mesh subdivision", without a GPU: against a second, plain
dictionary-of-edges float64 Loop written here, and against what the scheme promises -- the counts, the Euler characteristic, closed
stays closed, orientation and volume, the midpoint scheme's copies, planes, parents, the crease rule on boundaries, corners and darts."""
import numpy as np
import pytest

from tests import adjacency_ref as ar
from tests import subdivide_ref as sr


def icosahedron():
    g = (1 + 5 ** 0.5) / 2
    v = np.float32([[-1, g, 0], [1, g, 0], [-1, -g, 0], [1, -g, 0], [0, -1, g], [0, 1, g], [0, -1, -g], [0, 1, -g], [g, 0, -1], [g, 0, 1],
                    [-g, 0, -1], [-g, 0, 1]]) * np.float32(0.37) + np.float32([0.11, -0.23, 0.05])
    f = np.int32([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]])
    return v, f


def octahedron():
    v = np.float32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]) * np.float32([1.3, 0.7, 2.1]) + np.float32(0.3)
    f = np.int32([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    return v, f


def tetrahedron():
    v = np.float32([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]) * np.float32(5.3)
    f = np.int32([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
    return v, f


def grid(nx=5, ny=4, z=None, seed=3):
    """an open nx x ny grid of quads, two triangles each; z: a constant height, or None for a bumpy one"""
    x, y = np.meshgrid(np.arange(nx + 1, dtype=np.float32), np.arange(ny + 1, dtype=np.float32), indexing="ij")
    h = np.full(x.shape, z, np.float32) if z is not None else np.random.default_rng(seed).standard_normal(x.shape).astype(np.float32)
    v = np.stack([x * np.float32(1.5), y * np.float32(0.75), h], axis=-1).reshape(-1, 3)
    i = (np.arange(nx)[:, None] * (ny + 1) + np.arange(ny)[None, :]).reshape(-1)
    f = np.concatenate([np.stack([i, i + ny + 1, i + ny + 2], axis=1), np.stack([i, i + ny + 2, i + 1], axis=1)]).astype(np.int32)
    return v, f


MESHES = {"icosahedron": icosahedron, "octahedron": octahedron, "tetrahedron": tetrahedron, "grid": grid}
CLOSED = ("icosahedron", "octahedron", "tetrahedron")


def plain_loop(vertices, faces):
    """Loop subdivision with a dictionary of edges, float64 throughout, for manifold meshes with or without a boundary:
    {(a, b) with a < b: position of the edge's new vertex} and the new positions of the old vertices."""
    p = vertices.astype(np.float64)
    opposite = {}
    for a, b, c in faces.tolist():
        for u, v, w in ((a, b, c), (b, c, a), (c, a, b)):
            opposite.setdefault((min(u, v), max(u, v)), []).append(w)
    odd = {}
    ring = [[] for _ in p]
    border = [[] for _ in p]
    for (a, b), opp in opposite.items():
        assert len(opp) in (1, 2)
        if len(opp) == 2:
            odd[(a, b)] = 0.375 * (p[a] + p[b]) + 0.125 * (p[opp[0]] + p[opp[1]])
            ring[a].append(b), ring[b].append(a)
        else:
            odd[(a, b)] = 0.5 * (p[a] + p[b])
            border[a].append(b), border[b].append(a)
    even = p.copy()
    for v in range(len(p)):
        if border[v]:
            assert len(border[v]) == 2
            even[v] = 0.75 * p[v] + 0.125 * (p[border[v][0]] + p[border[v][1]])
        elif ring[v]:
            n = len(ring[v])
            beta = 0.1875 if n == 3 else 0.375 / n
            even[v] = (1 - n * beta) * p[v] + beta * sum(p[j] for j in ring[v])
    return odd, even


@pytest.mark.parametrize("name", sorted(MESHES))
def test_the_restatement_agrees_with_a_plain_loop(name):
    v, f = MESHES[name]()
    out, faces, parents = sr.subdivide(v, f, sr.LOOP)
    odd, even = plain_loop(v, f)
    m = float(np.abs(v).max())
    # The bound, from the rule.  An even vertex is p + beta (S - n p) with S the sum of n terms trunc(x 2^k) 2^-k: each term is short by
    # less than 2^-k = 2^(e - 27) <= M 2^-27, so S by less than n M 2^-27, and beta n <= 0.5625 (n = 3; 0.375 otherwise, 0.25 on a
    # crease): less than 0.5625 M 2^-27.  The result has magnitude at most M and is rounded once to fp32: M 2^-24.  The float64
    # operations on both sides, a dozen on magnitudes up to n M with n <= 8 here, add less than M 2^-45.  An odd vertex has the
    # rounding and the float64 terms only.
    bound_even = m * (2.0 ** -24 + 0.5625 * 2.0 ** -27 + 2.0 ** -45)
    bound_odd = m * (2.0 ** -24 + 2.0 ** -45)
    nv = len(v)
    assert np.abs(out[:nv].astype(np.float64) - even).max() <= bound_even
    assert len(out) == nv + len(odd)
    for i in range(nv, len(out)):
        a, b = (int(x) for x in parents[i])
        assert np.abs(out[i].astype(np.float64) - odd[(min(a, b), max(a, b))]).max() <= bound_odd
    if name != "grid":
        assert not (out[:nv] == v).all(axis=1).any()                            # every vertex of a closed curved mesh moves


@pytest.mark.parametrize("scheme", [sr.MIDPOINT, sr.LOOP])
@pytest.mark.parametrize("name", sorted(MESHES))
def test_counts_euler_closedness_and_parents(name, scheme):
    v, f = MESHES[name]()
    adj, edge, half_edge = ar.by_index(f)
    out, faces, parents = sr.subdivide(v, f, scheme)
    assert faces.shape == (4 * len(f), 3) and faces.dtype == np.int32           # F' = 4 F
    assert out.shape == (len(v) + len(half_edge), 3) and out.dtype == np.float32 and parents.shape == (len(out), 2)      # V' = V + E
    adj2, edge2, half_edge2 = ar.by_index(faces)
    assert ar.euler(len(out), len(half_edge2), len(faces)) == ar.euler(len(v), len(half_edge), len(f))
    assert len(half_edge2) == 2 * len(half_edge) + 3 * len(f)
    if name in CLOSED:
        assert (adj >= 0).all() and (adj2 >= 0).all() and ar.euler(len(out), len(half_edge2), len(faces)) == 2
    else:
        assert (adj2 == -1).sum() == 2 * (adj == -1).sum() and (adj2 == -2).sum() == 0      # a boundary stays one
    assert (parents[:len(v)] == np.arange(len(v))[:, None]).all()
    flat = f.reshape(-1)
    h = half_edge.astype(np.int64)
    assert (parents[len(v):, 0] == flat[h]).all() and (parents[len(v):, 1] == flat[3 * (h // 3) + (h % 3 + 1) % 3]).all()
    # the child order: child k < 3 starts at corner k, the last one is the three new vertices
    kids = faces.reshape(len(f), 4, 3)
    assert (kids[:, [0, 1, 2], 0] == f).all() and (kids[:, 3] >= len(v)).all()
    assert (kids[:, 0, 1] == kids[:, 3, 0]).all() and (kids[:, 1, 1] == kids[:, 3, 1]).all() and (kids[:, 2, 1] == kids[:, 3, 2]).all()


def volume(v, f):
    p = v.astype(np.float64)[f]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6)


def area(v, f):
    p = v.astype(np.float64)[f]
    return float(0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1).sum())


@pytest.mark.parametrize("name", CLOSED)
def test_orientation_and_volume(name):
    v, f = MESHES[name]()
    before = volume(v, f)
    assert before > 0
    out, faces, _ = sr.subdivide(v, f, sr.MIDPOINT)
    assert out[:len(v)].tobytes() == v.tobytes()                               # midpoint leaves the even vertices' bytes alone
    # every child lies in its parent's plane with the parent's orientation: the normals point the same way
    n0 = np.cross(v[f][:, 1] - v[f][:, 0], v[f][:, 2] - v[f][:, 0]).astype(np.float64)
    p = out[faces].astype(np.float64)
    n1 = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert (np.einsum("ij,ij->i", n1, np.repeat(n0, 4, axis=0)) > 0).all()
    # a new vertex is off its exact midpoint by one fp32 rounding, at most M 2^-24 per coordinate, sqrt(3) M 2^-24 in length; moving
    # the vertices of a closed surface of area A by at most d changes its volume by at most A d (to first order; the factor 2 is slack)
    m = float(np.abs(v).max())
    assert abs(volume(out, faces) - before) <= 2 * area(v, f) * 3 ** 0.5 * m * 2.0 ** -24
    smooth, faces2, _ = sr.subdivide(v, f, sr.LOOP)
    assert 0 < volume(smooth, faces2) < before                                  # a closed convex mesh's volume does not grow under Loop
    n2 = np.cross(*(smooth[faces2].astype(np.float64)[:, k] - smooth[faces2].astype(np.float64)[:, 0] for k in (1, 2)))
    assert (np.einsum("ij,ij->i", n2, np.repeat(n0, 4, axis=0)) > 0).all()


def test_a_flat_grid_stays_flat_and_its_boundary_follows_the_crease_rule():
    v, f = grid(5, 4, z=0.75)
    detail = {}
    out, faces, parents = sr.subdivide(v, f, sr.LOOP, detail)
    assert (out[:, 2] == np.float32(0.75)).all()                                # exactly: 0.75 2^k is an integer, so no sum is truncated
    n_int, n_cr = detail["n_int"], detail["n_cr"]
    border = ar.boundary_vertices(f, detail["adj"], len(v))
    assert set(n_cr.tolist()) == {0, 2} and ((n_cr == 2) == border).all()
    # boundary vertices: 1/8 6/8 1/8 along the boundary, whatever lies inside
    p = v.astype(np.float64)
    flat, h = f.reshape(-1), detail["half_edge"].astype(np.int64)
    ends = np.stack([flat[h], flat[3 * (h // 3) + (h % 3 + 1) % 3]], axis=1)[~detail["interior"]]
    m = float(np.abs(v).max())
    for i in np.flatnonzero(border):
        others = [int(a if b == i else b) for a, b in ends if i in (a, b)]
        assert len(others) == 2
        want = 0.75 * p[i] + 0.125 * (p[others[0]] + p[others[1]])
        assert np.abs(out[i].astype(np.float64) - want).max() <= m * (2.0 ** -24 + 0.25 * 2.0 ** -27 + 2.0 ** -45)
    corners = [0, 4, 5 * 5, 5 * 5 + 4]
    assert all(n_cr[c] == 2 and (out[c] != v[c]).any() for c in corners)        # a grid corner has two boundary edges: it moves
    straight = [i for i in np.flatnonzero(border) if i not in corners]
    assert all((out[i, 0] == v[i, 0]) or (out[i, 1] == v[i, 1]) for i in straight)      # ... and a vertex on a straight side slides along it


def test_darts_and_crowded_vertices_keep_their_bits():
    v, f = icosahedron()
    f = np.concatenate([f, np.int32([[0, 11, 0]])])                            # a degenerate triangle makes edge (0, 11) a group of four
    detail = {}
    out, faces, parents = sr.subdivide(v, f, sr.LOOP, detail)
    n_cr = detail["n_cr"]
    assert n_cr[0] == 1 and n_cr[11] == 1 and n_cr.sum() == 2                   # two darts
    assert out[0].tobytes() == v[0].tobytes() and out[11].tobytes() == v[11].tobytes()
    others = [i for i in range(len(v)) if i not in (0, 11)]
    assert not (out[others] == v[others]).all(axis=1).any()
    assert detail["edge"][-1].tolist() == [detail["edge"][0][0], detail["edge"][0][0], -1]
    assert faces[-4:].tolist()[0][2] == 0 and faces[-1][2] == 0                 # m of the zero-length edge is the vertex itself
    # a corner where three creases meet: three triangles round one edge, each end has n_cr = 4 (the shared edge and three open ones)
    fan_v = np.float32([[0, 0, 0], [0, 0, 1], [1, 0, 0], [0, 1, 0], [-1, -1, 0]])
    fan_f = np.int32([[0, 1, 2], [0, 1, 3], [0, 1, 4]])
    d2 = {}
    o2, f2, _ = sr.subdivide(fan_v, fan_f, sr.LOOP, d2)
    assert d2["n_cr"].tolist() == [4, 4, 2, 2, 2] and d2["n_int"].sum() == 0
    assert o2[:2].tobytes() == fan_v[:2].tobytes() and (o2[2:5] != fan_v[2:5]).any(axis=1).all()
    assert len(o2) == 5 + 7 and (ar.by_index(f2)[0] == -2).sum() == 2 * 3       # the fan's edge counts once, and stays a fan


def test_two_levels_are_the_restatement_twice_and_hostile_values_pass_through():
    v, f = grid()
    once = sr.subdivide(v, f, sr.LOOP)
    twice = sr.subdivide(once[0], once[1], sr.LOOP)
    got = sr.levels(v, f, 2, sr.LOOP)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, twice)) and sr.levels(v, f, 0)[2] is None
    w = v.copy()
    w.view(np.uint32)[3, 1] = 0x7FC00001                                       # a NaN with a payload
    w[7, 0] = np.inf
    g = f.copy()
    g[2, 1], g[5, 2] = -1, len(v)
    for scheme in (sr.MIDPOINT, sr.LOOP):
        d = {}
        out, faces, parents = sr.subdivide(w, g, scheme, d)
        assert out[3].tobytes() == w[3].tobytes() and out[7].tobytes() == w[7].tobytes()
        bad = ~d["usable"]
        assert bad.sum() > 4 and (out[len(w):].view(np.uint32)[bad] == sr.NAN_WORD).all()
        assert not np.isnan(out[len(w):][~bad]).any()
        assert (faces == -1).sum() == 1 and (faces == len(v)).sum() >= 1       # the children copy the index
    assert sr.shift(np.zeros((3, 3), np.float32)) == 0 and sr.shift(np.float32([[1.5, -3, np.inf]])) == 26
    assert sr.shift(np.float32([[1e-45, 0, 0]])) == 27 + 149 and sr.shift(np.float32([[3e38, 0, 0]])) == 27 - 127
