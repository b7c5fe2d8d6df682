"""Isosurface extraction on the GPU (drt_renderer_isosurface, kernel_isosurface.hip): the counts, every record's 48 bytes and the miss
fill bit-equal to the restatement in tests/isosurface_ref.py at the smallest shapes where the kernel can go wrong -- one cube, rows
around the 63-cube step of a wave, dense and empty fields, a border, flip, NaN and infinities, a level that hits samples, offsets near
4096, pure counts, truncated and gapped segments, numpy and tensor input, a side stream -- then the records as queries of the existing
calls, the mesh as a scene through shells / shellMeasures, and the case the feature exists for: a torus with a tenth of its triangles
missing, remeshed into one watertight shell that classifies points as the winding numbers of the damaged mesh do."""
import ctypes

import numpy as np
import pytest

from tests import inside_ref as ir
from tests import isosurface_ref as iso
from tests import ray_query_ref as rq

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
_cache = {}


@pytest.fixture(scope="module")
def renderer():
    return drt.Renderer(0)


def grid_of(field, lo, cell):
    g = drt._Grid()
    g.lo[:], g.cell[:] = [float(v) for v in np.float32(lo)], [float(v) for v in np.float32(cell)]
    g.dims[:] = field.shape[::-1]
    return g


def raw(renderer, field, level, lo, cell, flip=False, border=None, offsets=None, capacity=0, sentinel=None, counts=True):
    """One call of the entry point: (counts uint32 [rows] or None, out RECORD [capacity] or None).  out starts as `sentinel` bytes
    (default 0xA5), counts as 0xffffffff."""
    f = torch.from_numpy(np.ascontiguousarray(field, np.float32)).to(DEV)
    pad = 0 if border is None else 2
    rows = (field.shape[1] - 1 + pad) * (field.shape[0] - 1 + pad)
    cnt = torch.full((rows,), -1, dtype=torch.int32, device=DEV) if counts else None
    off = torch.from_numpy(np.asarray(offsets, np.uint32).view(np.int32)).to(DEV) if offsets is not None else None
    out = None
    if capacity:
        start = np.full(capacity * 48, 0xA5, np.uint8) if sentinel is None else np.frombuffer(sentinel.tobytes(), np.uint8)
        out = torch.from_numpy(start.copy()).to(DEV)
    rc = drt._lib.drt_renderer_isosurface(renderer._h, f.data_ptr(), ctypes.byref(grid_of(field, lo, cell)), float(level),
                                          NAN if border is None else float(border), 1 if flip else 0,
                                          off.data_ptr() if off is not None else None, out.data_ptr() if out is not None else None, capacity,
                                          cnt.data_ptr() if cnt is not None else None, torch.cuda.current_stream().cuda_stream)
    assert rc == drt.OK, drt._lib.drt_last_error()
    torch.cuda.synchronize()
    return (cnt.cpu().numpy().view(np.uint32) if cnt is not None else None,
            np.frombuffer(out.cpu().numpy().tobytes(), iso.RECORD) if out is not None else None)


def same_records(got, ref, what):
    """Bit-equal records, a NaN coordinate equal to any NaN (the sign of one that arithmetic makes is the hardware's)."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    g, r = np.frombuffer(got.tobytes(), np.uint32).reshape(-1, 12), np.frombuffer(ref.tobytes(), np.uint32).reshape(-1, 12)
    eq = g == r
    eq[:, 0:9] |= np.isnan(g[:, 0:9].view(np.float32)) & np.isnan(r[:, 0:9].view(np.float32))
    bad = np.nonzero(~eq.all(axis=1))[0]
    assert len(bad) == 0, "%s: %d of %d records differ, first %d: %r vs %r" % (what, len(bad), len(g), bad[0], got[bad[0]], ref[bad[0]])


def check(renderer, field, level, lo, cell, what, **kw):
    """The count pass, the exact two-pass fill and a fill with counts against the restatement; returns (counts, records)."""
    counts, recs = iso.isosurface(field, level, lo, cell, **kw)
    got_counts, none = raw(renderer, field, level, lo, cell, **kw)                      # a pure count: no offsets, no out
    assert none is None and got_counts.tolist() == counts.tolist(), what
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    if len(recs):
        _, out = raw(renderer, field, level, lo, cell, offsets=offsets, capacity=len(recs), counts=False, **kw)
        same_records(out, recs, what)
        again_counts, again = raw(renderer, field, level, lo, cell, offsets=offsets, capacity=len(recs), **kw)
        assert again_counts.tolist() == counts.tolist() and again.tobytes() == out.tobytes(), what   # the same bytes from two runs
    return counts, recs


def normal_field(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


ROW_CUBES = (62, 63, 64, 65, 126, 127, 128)                       # the seams of a 63-cube step, and of a 64-cube one


@pytest.mark.parametrize("dims", [(2, 2, 2), (3, 2, 2), (2, 3, 2), (2, 2, 3)])
def test_single_cubes_and_the_smallest_grids(renderer, dims):
    f = normal_field(dims[::-1], 7)
    for kw in ({}, dict(flip=True), dict(border=-3.0), dict(border=3.0, flip=True)):
        counts, _ = check(renderer, f, 0.05, (0.25, -1.5, 3.0), (0.5, 0.75, 1.25), "%r %r" % (dims, kw), **kw)
        assert counts.sum() > 0


@pytest.mark.parametrize("cubes", ROW_CUBES)
@pytest.mark.parametrize("border", [None, -2.0])
def test_rows_around_the_wave_step(renderer, cubes, border):
    x = cubes + 1 if border is None else cubes - 1
    f = normal_field((2, 3, x), cubes)                            # dense: nearly every cube emits, the running base carries over
    kw = {} if border is None else dict(border=border)
    counts, recs = check(renderer, f, 0.1, (-1.0, 0.5, 2.0), (0.125, 0.25, 0.5), "%d cubes, border %r" % (cubes, border), **kw)
    assert len(counts) == (2 * 1 if border is None else 4 * 3)
    assert counts.sum() > 2 * cubes * len(counts)


def test_a_dense_random_field(renderer):
    f = normal_field((5, 7, 9), 1)
    counts, recs = check(renderer, f, 0.1, (0, 0, 0), (1, 1, 1), "dense")
    assert counts.min() > 0
    check(renderer, f, 0.1, (0, 0, 0), (1, 1, 1), "dense flip", flip=True)
    check(renderer, f, 0.1, (0, 0, 0), (1, 1, 1), "dense border", border=-1.0)


def shape20(name):
    if name not in _cache:
        if name == "sphere":
            lo, hi = (-1.03, -1.1, -1.07), (1.05, 1.02, 1.09)
            f, cell = iso.sphere_sdf(20, lo, hi, 0.8)
        else:
            lo, hi = (-1.13, -1.1, -0.57), (1.15, 1.12, 0.59)
            f, cell = iso.torus_sdf(20, lo, hi, 0.7, 0.25)
        _cache[name] = (f, np.float32(lo), np.float32(hi), cell)
    return _cache[name]


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_sphere_and_torus_fields(renderer, name):
    f, lo, hi, cell = shape20(name)
    for kw in ({}, dict(flip=True), dict(border=1.0), dict(border=1.0, flip=True)):
        counts, recs = check(renderer, f, 0.0, lo, cell, "%s %r" % (name, kw), **kw)
        assert (drt.triEdgeAdjacency(iso.triangles(recs)) >= 0).all()
        assert (counts == 0).sum() > 0                            # empty rows too


def test_nan_and_infinities_sprinkled_in(renderer):
    f = normal_field((6, 7, 70), 11)
    rng = np.random.default_rng(12)
    for value in (np.nan, np.inf, -np.inf):
        f.reshape(-1)[rng.choice(f.size, 40, replace=False)] = value
    clean = iso.isosurface(np.nan_to_num(f, nan=0.0, posinf=1.0, neginf=-1.0), 0.1, (0, 0, 0), (1, 1, 1))[1]
    for kw in ({}, dict(border=-1.0)):
        _, recs = check(renderer, f, 0.1, (0, 0, 0), (1, 1, 1), "non-finite %r" % kw, **kw)
        assert np.isfinite(recs["v"]).all()
    assert 0 < len(iso.isosurface(f, 0.1, (0, 0, 0), (1, 1, 1))[1]) < len(clean)


def test_a_level_that_hits_samples_exactly(renderer):
    f = np.random.default_rng(5).integers(-2, 3, (4, 5, 66)).astype(np.float32)
    counts, recs = check(renderer, f, 1.0, (0, 0, 0), (1, 1, 1), "level on samples")
    t = iso.triangles(recs)
    e = t[:, [1, 2, 0]] - t
    assert (np.abs(e).max(axis=2) == 0).any()                     # zero-length edges, as documented
    check(renderer, f, 1.0, (0, 0, 0), (1, 1, 1), "level on samples, border", border=1.0)


def test_all_below_and_all_above_give_nothing(renderer):
    for value in (-1.0, 1.0):
        f = np.full((3, 4, 70), value, np.float32)
        counts, recs = check(renderer, f, 0.0, (0, 0, 0), (1, 1, 1), "constant %r" % value)
        assert counts.sum() == 0 and len(recs) == 0
        # an empty fill: no row owns a slot, the buffer survives
        zero = np.zeros(len(counts) + 1, np.uint32)
        got_counts, out = raw(renderer, f, 0.0, (0, 0, 0), (1, 1, 1), offsets=zero, capacity=4)
        assert got_counts.sum() == 0 and (np.frombuffer(out.tobytes(), np.uint8) == 0xA5).all()
        res = renderer.isosurface(f, 0.0, (0, 0, 0), (70, 4, 3))
        assert res.tris.shape == (0, 3, 3) and res.splits.tolist() == [0] * (len(counts) + 1) and res.cube.shape == (0,)


def test_coordinates_near_4096(renderer):
    f, _, _, _ = shape20("sphere")
    lo, cell = np.float32([4095.3, -4097.9, 4090.1]), np.float32([0.37, 0.11, 0.73])
    counts, recs = check(renderer, f, 0.0, lo, cell, "offset")
    assert np.abs(recs["v"]).min() > 4080
    # an ulp is 2^-11 here: vertices close to a sample collapse onto one position, and the adjacency marks their edges -2; the
    # surface still has no boundary, because both sides of a lattice edge compute the same bits
    adj = drt.triEdgeAdjacency(iso.triangles(recs))
    assert (adj == -1).sum() == 0 and 0 < (adj == -2).sum() < len(recs) // 50


def test_truncated_capacities(renderer):
    f = normal_field((3, 4, 130), 21)
    counts, recs = iso.isosurface(f, 0.1, (0, 0, 0), (1, 1, 1))
    rows = len(counts)
    assert counts.min() > 70                                      # every row is longer than its segment below, over more than one step
    for per_row, capacity in ((2, 2 * rows), (70, 70 * rows), (70, 70 * rows - 100), (70, 35)):
        offsets = (np.arange(rows + 1) * per_row).astype(np.uint32)
        got_counts, out = raw(renderer, f, 0.1, (0, 0, 0), (1, 1, 1), offsets=offsets, capacity=capacity)
        assert got_counts.tolist() == counts.tolist()             # the total, stored or not
        same_records(out, iso.fill(counts, recs, offsets, capacity), "per row %d, capacity %d" % (per_row, capacity))
    # segments longer than the lists: miss records behind them
    f = shape20("sphere")[0]
    counts, recs = iso.isosurface(f, 0.0, (0, 0, 0), (1, 1, 1))
    offsets = (np.arange(len(counts) + 1) * 90).astype(np.uint32)
    _, out = raw(renderer, f, 0.0, (0, 0, 0), (1, 1, 1), offsets=offsets, capacity=int(offsets[-1]), counts=False)
    ref = iso.fill(counts, recs, offsets, int(offsets[-1]))
    same_records(out, ref, "padded")
    assert (ref["cube"] == iso.MISS_CUBE).sum() > 0 and not ref[ref["cube"] == iso.MISS_CUBE]["v"].any()


def test_offsets_that_leave_gaps_keep_the_sentinel(renderer):
    f = normal_field((3, 4, 40), 23)
    counts, recs = iso.isosurface(f, 0.1, (0, 0, 0), (1, 1, 1), border=-1.0)
    rows = len(counts)
    # a decreasing pair owns nothing: the even rows own 200 slots each, laid out downwards -- row 0 [4700, 4900), row 2 [4400, 4600), .. --
    # so every odd row's pair decreases, and [4900, 5000), the 100 slots between two segments and [0, 2000) belong to nobody
    offsets = np.zeros(rows + 1, np.uint32)
    offsets[0::2] = 4700 - 300 * np.arange(len(offsets[0::2]))
    offsets[1::2] = offsets[0::2][:len(offsets[1::2])] + 200
    assert rows == 20 and offsets.min() == 1700
    capacity = 5000
    sentinel = np.zeros(capacity, iso.RECORD)
    sentinel["cube"], sentinel["code"], sentinel["v"] = 0x5E5E5E5E, 77, 1.5
    got_counts, out = raw(renderer, f, 0.1, (0, 0, 0), (1, 1, 1), border=-1.0, offsets=offsets, capacity=capacity, sentinel=sentinel)
    ref = iso.fill(counts, recs, offsets, capacity, out=sentinel)
    assert got_counts.tolist() == counts.tolist()
    same_records(out, ref, "gaps")
    untouched = ref["cube"] == 0x5E5E5E5E
    assert 0 < untouched.sum() < capacity and (ref["cube"] == iso.MISS_CUBE).sum() > 0


def test_numpy_in_tensor_in_and_a_side_stream(renderer):
    f, lo, hi, cell = shape20("torus")
    counts, recs = iso.isosurface(f, 0.0, lo, cell, border=1.0)
    splits = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    host = renderer.isosurface(f, 0.0, lo, hi, border=1.0)
    assert all(isinstance(x, np.ndarray) for x in host)
    assert host.splits.tolist() == splits.tolist() and host.tris.tobytes() == iso.triangles(recs).tobytes()
    assert host.cube.tolist() == recs["cube"].tolist() and host.code.tolist() == recs["code"].tolist()
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        dev = renderer.isosurface(torch.from_numpy(f).to(DEV, non_blocking=True), 0.0, lo, hi, border=1.0)
    side.synchronize()
    assert all(torch.is_tensor(x) and x.is_cuda for x in dev)
    assert dev.tris.shape == (len(recs), 3, 3) and dev.tris.stride() == (12, 3, 1)
    assert dev.tris.cpu().numpy().tobytes() == host.tris.tobytes() and dev.splits.cpu().tolist() == splits.tolist()
    assert dev.records().cpu().numpy().tobytes() == recs.tobytes() == host.records().tobytes()
    # face normals, on the device and on the host, against float64.  In fp32 the edges carry eps = 2^-24 each and every component of
    # the cross product up to 3 eps |e1| |e2|, so a unit normal is off by at most 16 eps |e1| |e2| / |c| + 8 eps per component: the
    # condition number of a sliver's normal times the rounding, doubled for the normalisation of a perturbed vector, plus its own
    t64 = host.tris.astype(np.float64)
    e1, e2 = t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0]
    c = np.cross(e1, e2)
    length = np.linalg.norm(c, axis=1, keepdims=True)
    bound = 16 * 2.0 ** -24 * np.linalg.norm(e1, axis=1, keepdims=True) * np.linalg.norm(e2, axis=1, keepdims=True) / length + 8 * 2.0 ** -24
    for n in (dev.faceNormals().cpu().numpy(), host.faceNormals()):
        assert n.shape == (len(recs), 3) and n.dtype == np.float32
        assert (np.abs(n - c / length) <= bound).all(), np.abs(n - c / length).max()
    flipped = renderer.isosurface(f, 0.0, lo, hi, border=1.0, flip=True)
    assert flipped.tris[:, [0, 2, 1]].tobytes() == host.tris.tobytes()


def torus_scene():
    if "torus_scene" not in _cache:
        _cache["torus_scene"] = rq.programmatic_scene(drt, *ir.streams(ir.torus()), 4, 8)
    return _cache["torus_scene"]


def test_the_records_are_triangle_queries_as_they_stand(renderer):
    sc, _ = torus_scene()
    lo, hi = np.float32([-1.45, -1.43, -0.47]), np.float32([1.47, 1.44, 0.45])
    res = 20
    cell = iso.cell_of(lo, hi, (res,) * 3)
    ax = [iso.positions(lo[k], cell[k], res, 0).astype(np.float64) for k in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    f = ir.torus_distance(np.stack([x, y, z], axis=-1).reshape(-1, 3)).reshape(res, res, res).astype(np.float32)
    surf = renderer.isosurface(torch.from_numpy(f).to(DEV), 0.0, lo, hi)
    rec = surf.records()
    assert rec.data_ptr() == surf.tris.data_ptr() and rec.shape[1] == 12      # the fill's own output
    as_records = renderer.overlapTriangles(sc, rec)
    as_copies = renderer.overlapTriangles(sc, surf.tris.contiguous())
    assert torch.equal(as_records.splits, as_copies.splits) and torch.equal(as_records.prim, as_copies.prim)
    assert as_records.prim.shape[0] > surf.tris.shape[0] // 4                 # the surfaces hug each other


def test_the_mesh_is_one_watertight_shell_with_the_restatements_volume(renderer):
    f, lo, hi, cell = shape20("torus")
    surf = renderer.isosurface(f, 0.0, lo, hi)
    sc = surf.toScene()
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = 4, 8
    b.buildIterative(sc)
    sh = renderer.shells(sc)
    assert sh.count == 1 and sh.watertight.tolist() == [True] and sh.open_edges.tolist() == [0] and sh.bad_edges.tolist() == [0]
    assert sh.triangles.tolist() == [surf.tris.shape[0]]
    # the float64 divergence sum of the restatement's triangles in the stored form (v0, e1 = v1 - v0, e2 = v2 - v0 in fp32), as the
    # shell terms of include/drt.h are defined; the device sums the same terms in another order
    t = iso.triangles(iso.isosurface(f, 0.0, lo, cell)[1])
    v0, e1, e2 = t[:, 0].astype(np.float64), (t[:, 1] - t[:, 0]).astype(np.float64), (t[:, 2] - t[:, 0]).astype(np.float64)
    w = (v0 * np.cross(e1, e2)).sum(axis=1)
    volume = float(renderer.shellMeasures(sc).volume[0])
    bound = 4.0 * len(w) * 2.0 ** -53 * np.abs(w).sum() / 6.0      # 4 n eps sum |term|: any order of n float64 additions
    print("volume %.17g, restatement %.17g, difference %.3g, bound %.3g" % (volume, w.sum() / 6.0, volume - w.sum() / 6.0, bound))
    assert abs(volume - w.sum() / 6.0) <= bound
    assert volume == pytest.approx(2.0 * np.pi ** 2 * 0.7 * 0.25 ** 2, rel=0.03)


def open_torus(seed=17):
    pos = ir.torus()
    keep = np.ones(len(pos), bool)
    keep[np.random.default_rng(seed).choice(len(pos), len(pos) // 10, replace=False)] = False
    return pos[keep]


def test_end_to_end_a_damaged_torus_comes_out_closed_and_classifies_alike(renderer):
    """tests/test_isosurface_ref.py checks the same on the references alone, with the same 218 points."""
    damaged, _ = rq.programmatic_scene(drt, *ir.streams(open_torus()), 4, 8)
    surf = renderer.remesh(damaged, 24)
    assert surf.splits.shape[0] == 27 * 27 + 1                    # 26^3 samples and a border
    t = surf.tris.cpu().numpy()
    assert (drt.triEdgeAdjacency(t) >= 0).all()
    V, E, F = iso.euler(t)
    assert V - E + F == 0
    sc = surf.toScene()
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = 4, 8
    b.buildIterative(sc)
    sh = renderer.shells(sc)
    assert sh.count == 1 and sh.watertight.tolist() == [True]
    assert float(renderer.shellMeasures(sc).volume[0]) > 0
    root = damaged.m_BVHNodes[-1]
    cell = iso.cell_of(root["bmin"], root["bmax"], (24,) * 3).max()            # the widest cell of remesh's grid
    p = np.random.default_rng(5).uniform((-1.6, -1.6, -0.5), (1.6, 1.6, 0.5), (600, 3)).astype(np.float32)
    p = p[np.abs(ir.torus_distance(p)) >= 2.0 * float(cell) + 0.01]           # at least two cells (and the facets' sag) from the surface
    assert len(p) == 218
    inside_new = renderer.inside(sc, p, rule="parity")
    inside_old = renderer.windingInside(damaged, p)
    assert inside_old.any() and (~inside_old).any()
    assert (inside_new == inside_old).all()
