"""Isosurface extraction, restated in float32 numpy from the rule in include/drt.h ("isosurface extraction"): marching tetrahedra on the
six-tetrahedron Kuhn split of every cube, the same 16-row table, the same interpolation order (always from the corner with the smaller
number) and the same record order as kernel_isosurface.hip.  Every * + - / below is one float32 operation on float32 operands, so
numpy rounds exactly where the kernel does.  Vectorised per tetrahedron, case and triangle: a 32^3 field takes well under a second."""
import numpy as np

# the tetrahedra of a cube, corners numbered c = dx + 2 dy + 4 dz, and which of them are mirror images (negative orientation)
TETS = ((0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7))
MIRROR = (0, 1, 1, 0, 0, 1)
# the edges of a tetrahedron by local vertex (p < q: the interpolation runs from p to q)
EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
# case (bit j set iff local vertex j is above) -> triangles of edge numbers, for a tetrahedron of positive orientation
TABLE = ((),
         ((0, 2, 1),),
         ((0, 3, 4),),
         ((1, 3, 4), (1, 4, 2)),
         ((1, 5, 3),),
         ((2, 5, 3), (2, 3, 0)),
         ((0, 1, 5), (0, 5, 4)),
         ((2, 5, 4),),
         ((2, 4, 5),),
         ((0, 4, 5), (0, 5, 1)),
         ((3, 5, 2), (3, 2, 0)),
         ((1, 3, 5),),
         ((1, 2, 4), (1, 4, 3)),
         ((0, 4, 3),),
         ((0, 1, 2),),
         ())

RECORD = np.dtype([("v", np.float32, (3, 3)), ("cube", np.uint32), ("code", np.uint32), ("zero", np.uint32)])   # drt_iso_tri, 48 B
MISS_CUBE = 0xFFFFFFFF
FLT_MAX = np.float32(3.402823466e+38)


def cell_of(lo, hi, res):
    """cell = (hi - lo) / res per component in float32, as Renderer.sdfGrid lays its samples out; res = (X, Y, Z)."""
    lo, hi = np.asarray(lo, np.float32).reshape(3), np.asarray(hi, np.float32).reshape(3)
    return ((hi - lo) / np.asarray(res, np.float32)).astype(np.float32)


def cube_dims(dims, border):
    """Cubes per axis (x, y, z): dims - 1 without a border, dims + 1 with one."""
    return tuple(int(d) + (1 if border else -1) for d in dims)


def positions(lo, cell, n, first):
    """float32 [n]: lo + ((float)idx + 0.5f) * cell for the lattice indices first .. first + n - 1, each operation rounded on its own."""
    idx = np.arange(first, first + n).astype(np.float32)
    return (np.float32(lo) + (idx + np.float32(0.5)) * np.float32(cell)).astype(np.float32)


def isosurface(field, level, lo, cell, flip=False, border=None):
    """(counts uint32 [rows], records RECORD [M]) of a float32 field [Z, Y, X]: every triangle of the rule in record order, and the
    number of them per row (the cubes along x of one (y, z))."""
    f = np.ascontiguousarray(field, np.float32)
    assert f.ndim == 3
    level = np.float32(level)
    lo, cell = np.asarray(lo, np.float32).reshape(3), np.asarray(cell, np.float32).reshape(3)
    has_border = border is not None and not np.isnan(border)
    first = 0
    if has_border:                                   # (the restatement may materialise the padded field; the kernel does not)
        f = np.pad(f, 1, constant_values=np.float32(border))
        first = -1
    Z, Y, X = f.shape
    nz, ny, nx = Z - 1, Y - 1, X - 1
    if min(nx, ny, nz) < 1:
        return np.zeros(max(ny, 0) * max(nz, 0), np.uint32), np.zeros(0, RECORD)
    px, py, pz = positions(lo[0], cell[0], X, first), positions(lo[1], cell[1], Y, first), positions(lo[2], cell[2], Z, first)
    corner = [f[dz:dz + nz, dy:dy + ny, dx:dx + nx].reshape(-1) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]   # c = dx + 2 dy + 4 dz
    with np.errstate(invalid="ignore"):
        above = [c >= level for c in corner]
        finite = [np.abs(c) <= FLT_MAX for c in corner]
    cz, cy, cx = np.unravel_index(np.arange(nx * ny * nz), (nz, ny, nx))
    parts = []
    for t, tet in enumerate(TETS):
        case = sum(above[c].astype(np.uint32) << j for j, c in enumerate(tet))
        ok = finite[tet[0]] & finite[tet[1]] & finite[tet[2]] & finite[tet[3]]
        case = np.where(ok, case, 0)
        swap = bool(MIRROR[t]) != bool(flip)
        for k in range(1, 15):
            sel = np.nonzero(case == k)[0]
            if len(sel) == 0:
                continue
            for j, tri in enumerate(TABLE[k]):
                rec = np.zeros(len(sel), RECORD)
                order = (tri[0], tri[2], tri[1]) if swap else tri
                for slot, e in enumerate(order):
                    ca, cb = tet[EDGES[e][0]], tet[EDGES[e][1]]
                    fa, fb = corner[ca][sel], corner[cb][sel]
                    with np.errstate(all="ignore"):
                        tt = (level - fa) / (fb - fa)
                        for axis, (p, i) in enumerate(((px, cx), (py, cy), (pz, cz))):
                            pa, pb = p[i[sel] + ((ca >> axis) & 1)], p[i[sel] + ((cb >> axis) & 1)]
                            rec["v"][:, slot, axis] = pa + (pb - pa) * tt
                rec["cube"] = sel
                rec["code"] = t | (k << 4)
                parts.append((sel.astype(np.int64) * 12 + t * 2 + j, rec))
    if parts:
        key = np.concatenate([p[0] for p in parts])
        recs = np.concatenate([p[1] for p in parts])[np.argsort(key, kind="stable")]
    else:
        recs = np.zeros(0, RECORD)
    counts = np.bincount(recs["cube"].astype(np.int64) // nx, minlength=ny * nz).astype(np.uint32)
    return counts, recs


def miss_record():
    m = np.zeros(1, RECORD)
    m["cube"] = MISS_CUBE
    return m[0]


def fill(counts, recs, offsets, capacity, out=None):
    """The fill pass's CSR rule on the restatement's list: row r owns out[offsets[r] .. offsets[r + 1]), cap_r = the difference if it is
    positive, else 0, clamped so that offsets[r] + cap_r <= capacity; the first cap_r records of the row are stored and the rest of
    the cap_r slots hold the miss record.  Slots nobody owns keep what `out` held."""
    out = np.zeros(capacity, RECORD) if out is None else out.copy()
    starts = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    for r in range(len(counts)):
        o0, o1 = int(offsets[r]), int(offsets[r + 1])
        cap = o1 - o0 if o1 > o0 else 0
        cap = min(cap, capacity - o0 if o0 < capacity else 0)
        n = min(cap, int(counts[r]))
        out[o0:o0 + n] = recs[starts[r]:starts[r] + n]
        out[o0 + n:o0 + cap] = miss_record()
    return out


def triangles(recs):
    """float32 [M, 3, 3] of the records."""
    return np.ascontiguousarray(recs["v"])


def signed_volume(tris):
    """float64 sum of dot(v0, cross(v1, v2)) / 6."""
    v = np.asarray(tris, np.float64)
    return float((v[:, 0] * np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def euler(tris):
    """(V, E, F) by unique bit patterns of positions: vertices are distinct 12-byte positions, edges unordered pairs of them."""
    t = np.ascontiguousarray(tris, np.float32)
    bits = (t + np.float32(0.0)).view(np.uint32).reshape(-1, 3)              # (-0.0 + 0.0 = +0.0: the adjacency's equality is IEEE ==)
    _, vid = np.unique(bits, axis=0, return_inverse=True)
    vid = vid.reshape(-1, 3)
    e = np.concatenate([vid[:, [0, 1]], vid[:, [1, 2]], vid[:, [2, 0]]])
    e.sort(axis=1)
    return int(vid.max() + 1) if len(vid) else 0, len(np.unique(e, axis=0)), len(t)


def sphere_sdf(res, lo, hi, radius):
    """(field [Z, Y, X] float32, cell) of |x| - radius at the sample positions."""
    return _field(res, lo, hi, lambda x, y, z: np.sqrt(x * x + y * y + z * z) - radius)


def torus_sdf(res, lo, hi, R, r):
    return _field(res, lo, hi, lambda x, y, z: np.sqrt((np.sqrt(x * x + y * y) - R) ** 2 + z * z) - r)


def _field(res, lo, hi, fn):
    res = (res,) * 3 if isinstance(res, int) else tuple(res)
    cell = cell_of(lo, hi, res)
    ax = [positions(np.float32(lo[k]), cell[k], res[k], 0).astype(np.float64) for k in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return fn(x, y, z).astype(np.float32), cell
