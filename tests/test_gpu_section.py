"""Plane sections on the GPU (drt_renderer_plane_sections, kernel_section.hip; Renderer.planeSections / cutsAny / slices / sectionAreas):
every slot of every segment and every count bit-equal to the restatement in tests/section_ref.py, miss records included -- over one
triangle, the quad, the tetrahedron, the cube, a soup whose lists take many 64-entry chunks, a tree deeper than any list is wide,
cornell_box, a fan whose every leaf emits and a tree whose leaves are longer than a wave; both modes, planes through vertices, on faces,
far away, scaled, with zero and negative-zero components and invalid ones, capacities, few waves, a refitted device copy, the torch and
the numpy path -- nothing written outside the segments, the renderer's state untouched, and the error codes of include/drt.h.
tests/test_section_ref.py asserts what the restatement does."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from tests import nearest_ref as nr
from tests import ray_query_ref as rq
from tests import refit_ref as rf
from tests import section_ref as sr
from tests.scenes import MODELS, ROOT, SCENES, scene_path
from tests.tri_overlap_scenes import TETRAHEDRON

drt = pytest.importorskip("dustraytracer_amd")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -77
ONE_MATERIAL = [((0.8, 0.8, 0.8), -1)]
SINGLE = np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
QUAD = np.float32([[[0, 0, 0], [1, 0, 0], [1, 1, 0]], [[0, 0, 0], [1, 1, 0], [0, 1, 0]]])
SCENE_NAMES = ["single", "quad", "tetrahedron", "cube", "soup", "chain", "cornell_box", "fan", "long_leaves"]
_cache = {}


@pytest.fixture(scope="module")
def renderer():
    return drt.Renderer(0)


def flat_scene(pos, leaf=20):
    n = len(pos)
    nrm = np.tile(np.float32([0, 0, 1]), (n, 3, 1))
    return rq.programmatic_scene(drt, pos, nrm, np.zeros((n, 3, 2), np.float32), np.zeros(n, np.int32), ONE_MATERIAL, [], leaf, 8)


def fan(n=300):
    """n triangles round the z axis, each with two vertices at z = -1 and one at z = +1: the plane z = 0 cuts every one of them."""
    a = (np.arange(n, dtype=np.float32) * np.float32(2 * np.pi / n)).astype(np.float32)
    b = (a + np.float32(np.pi / n)).astype(np.float32)
    r = np.float32(1) + (np.arange(n) % 7).astype(np.float32) * np.float32(0.25)
    pos = np.zeros((n, 3, 3), np.float32)
    pos[:, 0] = np.stack([r * np.cos(a), r * np.sin(a), np.full(n, -1, np.float32)], axis=1)
    pos[:, 1] = np.stack([r * np.cos(b), r * np.sin(b), np.full(n, -1, np.float32)], axis=1)
    pos[:, 2] = np.stack([(r + 1) * np.cos(a), (r + 1) * np.sin(a), np.full(n, 1, np.float32)], axis=1)
    return pos


def scene_pair(name):
    """(product scene, Geometry with the same tree): one triangle, the quad, the closed tetrahedron, models/cube.gltf, the soup of 3000
    triangles at two per leaf (1500 leaves), the chain of 43 levels, cornell_box with the editor's tree, the fan at two per leaf, and
    a soup built with a leaf target of 100 (leaves longer than a wave)."""
    if name not in _cache:
        if name in ("single", "quad", "tetrahedron"):
            sc, osc = flat_scene({"single": SINGLE, "quad": QUAD, "tetrahedron": TETRAHEDRON}[name])
            g = nr.from_oracle(osc)
        elif name == "fan":
            sc, osc = flat_scene(fan(), leaf=2)
            g = nr.from_oracle(osc)
            assert g.is_leaf.sum() > 128
        elif name == "soup":
            sc, osc = rq.programmatic_scene(drt, *rq.soup(3000, 5), 2, 8)
            g = nr.from_oracle(osc)
            assert sc.bvh_depth > 8 and g.is_leaf.sum() >= 1500
        elif name == "long_leaves":
            sc, osc = rq.programmatic_scene(drt, *rq.soup(700, 9), 100, 8)
            g = nr.from_oracle(osc)
            assert g.count[g.is_leaf].max() > 64
        elif name == "chain":
            sc, osc = rq.programmatic_scene(drt, *rq.degenerate_chain(), 1, 2)
            g = nr.from_oracle(osc)
            assert sc.bvh_depth == 43
        else:
            sc = drt.Scene()
            sc.loadGLTFmodel(os.path.join(MODELS, "cube.gltf") if name == "cube" else scene_path(name))
            b = drt.BVHBuilder()
            b.m_TargetLeafPrimitivesCount, b.m_BinCount = (4, 8) if name == "cube" else (20, 8)
            b.buildIterative(sc)
            g = nr.from_product(sc) if name == "cube" else nr.from_oracle(oracle.Scene.load_glb(scene_path(name)).build_bvh(20, 8))
        _cache[name] = (sc, g)
    return _cache[name]


def sweep_planes(g, n, seed):
    """About n planes [N, 4]: axis planes through vertices (s == 0 exactly there); the planes of faces; random ones through the scene,
    a third of them scaled by 1e-3 and a third by 1e3; far away; n = 0; zero and negative-zero components; and, last, four invalid
    ones with a NaN or an infinity."""
    rng = np.random.default_rng(seed)
    lo, hi = nr.bounds(g)
    extent = np.float32((hi - lo).max())
    k = max(n // 5, 2)
    v = nr.tie_points(g, k, rng)
    axis = (np.eye(3, dtype=np.float32)[rng.integers(0, 3, k)] * np.float32(rng.choice([-1, 1], k))[:, None]).astype(np.float32)
    through = sr.pack(axis, nr.dot(axis, v))
    t = rng.integers(0, len(g.v0), k)
    fn = np.cross(g.e1[t], g.e2[t]).astype(np.float32)
    fn = (fn / np.maximum(np.abs(fn).max(axis=1, keepdims=True), np.float32(1e-30))).astype(np.float32)     # (no overflow in d on the chain)
    faces = sr.pack(fn, nr.dot(fn, g.v0[t]))
    nn = rng.normal(size=(2 * k, 3)).astype(np.float32)
    pts = nr.box_points(g, 2 * k, rng)
    rand = sr.pack(nn, nr.dot(nn, pts))
    rand[::3] *= np.float32(1e-3)
    rand[1::3] *= np.float32(1e3)
    far = sr.pack(nn[:4], nr.dot(nn[:4], pts[:4]) + np.float32(100) * extent * np.linalg.norm(nn[:4], axis=1).astype(np.float32))
    mid = ((lo + hi) / 2).astype(np.float32)
    zeros = sr.pack([(0, 0, 0), (0, 0, 0), (-0.0, -0.0, -0.0)], [0, 1, -1])
    signed_zero = sr.pack([(-0.0, 0.0, 1), (0.0, -0.0, -1), (1, -0.0, -0.0), (-0.0, -1, 0.0), (0.0, 0.0, 1)],
                          [mid[2], -mid[2], mid[0], -mid[1], mid[2]])
    bad = np.repeat(sr.pack([(0, 0, 1)], [mid[2]]), 4, axis=0)
    bad[0, 0], bad[1, 3], bad[2, 2], bad[3, 1] = np.nan, np.inf, -np.inf, np.nan
    return np.concatenate([through, faces, rand, far, zeros, signed_zero, bad]).astype(np.float32)


def across(g):
    """Two planes through the middle of the scene: the long lists."""
    lo, hi = nr.bounds(g)
    mid = ((lo + hi) / 2).astype(np.float32)
    return sr.pack([(0, 0, 1), (0.3, 1, -0.2)], [mid[2], nr.dot(np.float32([0.3, 1, -0.2]), mid)])


def raw(r, sc, planes, offsets, out, capacity, counts, n, mode, stream=None):
    """The entry point itself on device tensors (or None): the status code."""
    ptr = lambda x: None if x is None else x.data_ptr()
    return drt._lib.drt_renderer_plane_sections(r._h, sc._h, ptr(planes), ptr(offsets), ptr(out), capacity, ptr(counts), n, mode, stream)


def run_raw(r, sc, planes, offsets, size, capacity, mode=sr.LIST, with_out=True, with_counts=True):
    """One call on sentinel-filled buffers of `size` records: (records as SECTION, counts) as host arrays (None where not given)."""
    n = len(planes)
    p = torch.from_numpy(np.ascontiguousarray(planes, np.float32)).to(DEV)
    off = None if offsets is None else torch.from_numpy(np.asarray(offsets).astype(np.int32)).to(DEV)
    out = torch.full((size, 8), SENTINEL, dtype=torch.int32, device=DEV) if with_out else None
    counts = torch.full((n,), -1, dtype=torch.int32, device=DEV) if with_counts else None
    assert raw(r, sc, p, off, out, capacity, counts, n, mode) == drt.OK
    torch.cuda.synchronize()
    return (None if out is None else out.cpu().numpy().view(sr.SECTION).reshape(-1)), (None if counts is None else counts.cpu().numpy())


def untouched(rec):
    return (rec.view(np.int32) == SENTINEL).all()


def csr(totals):
    return np.concatenate([[0], np.cumsum(totals.astype(np.int64))])


def as_records(lst):
    """A SectionList of host arrays as SECTION records."""
    rec = np.zeros(len(lst.prim), sr.SECTION)
    rec["p"], rec["q"], rec["prim"], rec["code"] = lst.p, lst.q, lst.prim, lst.code
    return rec


def cut(full, totals, caps):
    """The flat records of segments of `caps` slots (a scalar or [N]) from the whole lists: a prefix, then miss records."""
    n = len(totals)
    caps = np.broadcast_to(np.asarray(caps, np.int64), n)
    start, base = csr(totals), csr(caps)
    out = np.repeat(sr.MISS, int(base[-1]))
    for i in range(n):
        m = min(int(caps[i]), int(totals[i]))
        out[base[i]:base[i] + m] = full[start[i]:start[i] + m]
    return out


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_both_modes_are_bit_equal_to_the_restatement(renderer, name):
    sc, g = scene_pair(name)
    planes = np.concatenate([across(g), sweep_planes(g, 200, 11)])
    n = len(planes)
    full, totals = sr.whole(g, planes)
    print("%s: %d planes, %d records, the longest list %d" % (name, n, len(full), totals.max()))
    assert (totals == 0).any() and (totals > 0).any() and not totals[-4:].any()                 # nothing; something; NaN and inf
    assert np.isfinite(full["p"]).all() and np.isfinite(full["q"]).all()        # (bit-equal is meant of numbers: no NaN payloads)
    if name == "fan":
        assert totals[0] == 300                                                 # every lane of several chunks emits
    if name == "soup":
        assert totals.max() > 128
    # every segment of every plane: a count with capacity 0, the scan, the fill.  numpy in, numpy out, normals and d apart.
    got = renderer.planeSections(sc, planes[:, 0:3].copy(), planes[:, 3].copy())
    assert isinstance(got, drt.SectionList) and got.splits.dtype == np.int32 and got.prim.dtype == np.int32 and got.code.dtype == np.int32
    assert got.p.dtype == np.float32 and got.p.shape == (len(full), 3) and got.q.shape == (len(full), 3)
    assert (got.splits == csr(totals)).all() and as_records(got).tobytes() == full.tobytes(), name
    # the packed [N, 4] form, from torch: device tensors come back
    dev = renderer.planeSections(sc, torch.from_numpy(planes).to(DEV))
    assert all(x.device == torch.device(DEV) for x in dev) and dev.splits.dtype == torch.int32 and dev.p.dtype == torch.float32
    assert as_records(drt.SectionList(*(x.cpu().numpy() for x in dev))).tobytes() == full.tobytes()
    # mode ANY is LIST's count > 0
    hit = renderer.cutsAny(sc, planes)
    assert hit.dtype == np.bool_ and hit.shape == (n,) and (hit == (totals > 0)).all()
    assert (sr.sections(g, planes, 0, sr.ANY)[1] == hit).all()
    assert torch.equal(renderer.cutsAny(sc, torch.from_numpy(planes).to(DEV)).cpu(), torch.from_numpy(hit))
    # the raw entry point with ragged capacities, zeros included, between sentinels
    rng = np.random.default_rng(5)
    caps = rng.integers(0, 7, n)
    caps[rng.integers(0, n, n // 8)] = 0
    assert (caps == 0).sum() >= n // 16 and (caps > totals).any() and (caps < totals).any()
    lead, trail = 3, 5
    off = lead + csr(caps)
    size = int(off[-1]) + trail
    rec, counts = run_raw(renderer, sc, planes, off, size, size)
    assert untouched(rec[:lead]) and untouched(rec[off[-1]:])
    assert rec[lead:off[-1]].tobytes() == cut(full, totals, caps).tobytes() and (counts.view(np.uint32) == totals).all()
    ref, ref_counts = sr.sections(g, planes, caps)                              # (the restatement itself at these capacities)
    assert rec[lead:off[-1]].tobytes() == ref.tobytes() and (ref_counts == totals).all()
    # counts NULL with out given: the same records
    rec2, _ = run_raw(renderer, sc, planes, off, size, size, with_counts=False)
    assert rec2.tobytes() == rec.tobytes()
    # a capacity stated smaller than the last offsets, ending inside a segment: the records at and beyond it are untouched
    i = int(np.nonzero((caps >= 2) & (np.arange(n) > n // 2))[0][0])
    stated = int(off[i]) + 1
    rec3, counts3 = run_raw(renderer, sc, planes, off, size, stated)
    clamped = sr.caps_of(off, stated)
    assert clamped[i] == 1 and not clamped[i + 1:].any() and untouched(rec3[stated:]) and untouched(rec3[:lead])
    assert rec3[lead:stated].tobytes() == cut(full, totals, clamped).tobytes() and (counts3.view(np.uint32) == totals).all()
    # a pure count: out NULL with capacity 0; and mode ANY without offsets
    _, counts = run_raw(renderer, sc, planes, np.zeros(n + 1), 0, 0, with_out=False)
    assert (counts.view(np.uint32) == totals).all()
    _, counts = run_raw(renderer, sc, planes, None, 0, 0, mode=sr.ANY, with_out=False)
    assert (counts == (totals > 0)).all()


@pytest.mark.parametrize("name", ["soup", "cornell_box", "long_leaves"])
def test_capacities_0_to_9_and_exact_on_planes_across_the_whole_scene(renderer, name):
    sc, g = scene_pair(name)
    planes = across(g)
    full, totals = sr.whole(g, planes)
    assert totals.min() > 9
    for cap in list(range(0, 10)) + ["exact", "one more", "one less"]:
        caps = np.full(len(planes), cap) if isinstance(cap, int) else totals.astype(np.int64) + {"exact": 0, "one more": 1, "one less": -1}[cap]
        lead = 3
        off = lead + csr(caps)
        size = int(off[-1]) + 5
        rec, counts = run_raw(renderer, sc, planes, off, size, size)
        assert untouched(rec[:lead]) and untouched(rec[off[-1]:]), cap
        assert rec[lead:off[-1]].tobytes() == cut(full, totals, caps).tobytes() and (counts.view(np.uint32) == totals).all(), cap


@pytest.fixture(scope="module")
def many():
    """500 planes on the soup and their whole lists."""
    sc, g = scene_pair("soup")
    rng = np.random.default_rng(31)
    nn = rng.normal(size=(500, 3)).astype(np.float32)
    planes = sr.pack(nn, nr.dot(nn, nr.box_points(g, 500, rng)))
    full, totals = sr.whole(g, planes)
    assert (totals > 0).mean() > 0.9 and (totals == 0).any() and totals.max() > 128
    return sc, g, planes, full, totals


def test_500_planes_a_permutation_and_a_second_run(renderer, many):
    sc, g, planes, full, totals = many
    got = renderer.planeSections(sc, planes)
    assert (got.splits == csr(totals)).all() and as_records(got).tobytes() == full.tobytes()
    again = renderer.planeSections(sc, planes)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))                            # two runs: identical bytes
    perm = np.random.default_rng(2).permutation(len(planes))
    shuffled = renderer.planeSections(sc, planes[perm])
    start = csr(totals)
    want = np.concatenate([full[start[i]:start[i + 1]] for i in perm])
    assert (shuffled.splits == csr(totals[perm])).all() and as_records(shuffled).tobytes() == want.tobytes()
    assert (renderer.cutsAny(sc, planes) == (totals > 0)).all()


CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import dustraytracer_amd as drt
from tests import ray_query_ref as rq
data = np.load(sys.argv[2])
sc, _ = rq.programmatic_scene(drt, *rq.soup(3000, 5), 2, 8)
r = drt.Renderer(0)
got = r.planeSections(sc, data["planes"])
rec = np.zeros(len(got.prim), data["full"].dtype)
rec["p"], rec["q"], rec["prim"], rec["code"] = got.p, got.q, got.prim, got.code
assert (got.splits == data["splits"]).all(), "splits differ"
assert rec.tobytes() == data["full"].tobytes(), "records differ"
assert (r.cutsAny(sc, data["planes"]) == (np.diff(data["splits"]) > 0)).all(), "mode any differs"
print("child ok", len(rec))
"""


@pytest.mark.parametrize("waves", [1, 3])
def test_many_planes_through_few_waves(many, tmp_path, waves):
    """DRT_SECTION_WAVES caps the grid: 500 planes go through one wave, and through three, in a fresh process."""
    sc, g, planes, full, totals = many
    np.savez(tmp_path / "want.npz", planes=planes, full=full, splits=csr(totals).astype(np.int32))
    (tmp_path / "child.py").write_text(CHILD)
    env = dict(os.environ, DRT_SECTION_WAVES=str(waves))
    res = subprocess.run([sys.executable, str(tmp_path / "child.py"), ROOT, str(tmp_path / "want.npz")], env=env, capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0 and "child ok %d" % len(full) in res.stdout, res.stdout + res.stderr


def _load(name):
    sc = drt.Scene()
    sc.loadGLTFmodel(scene_path(name))
    st = rf.streams(sc.m_PrimitivesBuffer)
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
    b.buildIterative(sc)
    return sc, st


def test_after_a_refit_the_moved_mesh_answers(renderer):
    sc, st = _load("cornell_box")
    moved = (st[0] + np.random.default_rng(1).normal(0, 0.05, st[0].shape)).astype(np.float32)
    host, _ = _load("cornell_box")
    host.refit(moved)                                          # the host scene refitted with the same positions: the same tree
    g_old, g_new = nr.from_product(sc), nr.from_product(host)
    planes = np.concatenate([across(g_old), sweep_planes(g_old, 100, 4), sweep_planes(g_new, 100, 5)])
    old, old_counts = sr.whole(g_old, planes)
    new, new_counts = sr.whole(g_new, planes)
    assert (old_counts != new_counts).any() and old.tobytes() != new.tobytes()
    r = drt.Renderer(0)
    got = r.planeSections(sc, planes)
    assert (got.splits == csr(old_counts)).all() and as_records(got).tobytes() == old.tobytes()
    r.refit(sc, torch.from_numpy(moved).to(DEV))
    got = r.planeSections(sc, planes)
    assert (got.splits == csr(new_counts)).all() and as_records(got).tobytes() == new.tobytes()
    assert (r.cutsAny(sc, planes) == (new_counts > 0)).all()
    got = renderer.planeSections(sc, planes)                   # a renderer that was not refitted
    assert as_records(got).tobytes() == old.tobytes()


TETRA_PLANES = sr.pack([(0, 0, 1), (0, 0, -1), (0, 0, 1), (0, 0, 1), (1, 1, 1), (1, 0, 0)], [2, -2, 0, 4, 4, 1])
TETRA_AREAS = [2, 2, 0, 0, 8 * np.sqrt(3), 4.5]


def check_areas(renderer, s, g, planes, name):
    """sectionAreas against the same formula on the restatement's segments (section_ref.areas, float64, plane by plane), asserted on
    EVERY plane.  Only the order of the float64 sum differs: the terms' products of fp32 values are exact in float64, and two sums of
    the same m products in different orders differ by at most about m * 2^-53 * sum |products|.  With mass = 0.5 * sum |products|:
      every plane              |got - want| <= 1e-12 * mass: each of the two sums is within 3 m * 2^-53 of the mass, m <= 64 segments
                               here, so 2 * 192 * 1.1e-16 = 4.3e-14 of the mass is owed
      where mass <= 20 |area|  |got - want| <= 1e-12 * |area|, the issue's relative bound: 4.3e-14 * 20 = 8.5e-13 is owed
      mass == 0                got == 0 exactly (nothing listed, or zero-length segments only)
    Returns (want, mass, owed) for the caller's own assertions."""
    full, totals = sr.whole(g, planes)
    want = sr.areas(planes, full, totals)
    got = renderer.sectionAreas(s, planes)
    start = csr(totals)
    with np.errstate(invalid="ignore"):                                         # (the invalid planes: they list nothing)
        length = np.linalg.norm(planes[:, 0:3].astype(np.float64), axis=1)
        unit = planes[:, 0:3].astype(np.float64) / np.where(length > 0, length, 1)[:, None]
    mass = np.array([0.5 * np.abs(np.cross(full["p"][start[i]:start[i + 1]].astype(np.float64), full["q"][start[i]:start[i + 1]].astype(np.float64))
                                  * unit[i]).sum() for i in range(len(planes))])
    owed = (mass > 0) & (mass <= 20 * np.abs(want))
    diff = np.abs(got - want)
    print("%s: %d planes, %d cut, %d well conditioned; largest |got - want| / |area| there %.3e, largest |got - want| / mass anywhere %.3e"
          % (name, len(planes), (totals > 0).sum(), owed.sum(), (diff[owed] / np.abs(want)[owed]).max(initial=0),
             (diff[mass > 0] / mass[mass > 0]).max(initial=0)))
    assert totals.max() <= 64
    assert (diff[mass > 0] <= 1e-12 * mass[mass > 0]).all(), name
    assert (diff[owed] <= 1e-12 * np.abs(want)[owed]).all(), name
    assert (got[~(mass > 0)] == 0).all(), name
    return want, mass, owed


def test_section_areas_equal_the_restatement_s_on_every_plane(renderer):
    for name in ("tetrahedron", "cube", "cornell_box"):
        s, g = scene_pair(name)
        want, mass, owed = check_areas(renderer, s, g, sweep_planes(g, 100, 17), name)
        assert owed.sum() >= 50 and (mass == 0).any()
    # Small areas behind large running sums.  The reduction is a cumulative sum over ALL segments and differences at the splits, and
    # a running sum rounds relative to what the planes before it have summed to: 1500 tilted planes through the tetrahedron bring it
    # to several thousand, so a plain difference would give the four small triangles just under the apex (areas 4e-8 to 2e-6, each
    # well conditioned: n = (0, 0, 1), the contour is round the z axis) to no better than 1e-6 relative.  sectionAreas carries the
    # rounding errors of the running sum along, and the small planes meet the same 1e-12.
    s, g = scene_pair("tetrahedron")
    rng = np.random.default_rng(3)
    nn = rng.normal(size=(1500, 3)).astype(np.float32)
    big = sr.pack(nn, nr.dot(nn, nr.box_points(g, 1500, rng)))
    small = sr.pack(np.tile(np.float32([0, 0, 1]), (4, 1)), np.float32(4) - np.float32([0.0013, 0.0007, 0.0021, 0.0003]))
    planes = np.concatenate([big[:500], small[:1], big[500:1000], small[1:3], big[1000:], small[3:]]).astype(np.float32)
    at = [500, 1001, 1002, 1503]
    want, mass, owed = check_areas(renderer, s, g, planes, "small areas behind large running sums")
    assert owed[at].all() and (want[at] > 0).all() and (want[at] < 3e-6).all() and np.abs(want[:500]).sum() > 1000


def test_slices_and_section_areas(renderer):
    # the hand cases of tests/test_section_ref.py: the endpoints are fp32 and exact, the reduction is float64
    sc, g = scene_pair("tetrahedron")
    areas = renderer.sectionAreas(sc, TETRA_PLANES)
    assert isinstance(areas, np.ndarray) and areas.dtype == np.float64 and areas.shape == (6,)
    print("tetrahedron areas", areas.tolist())
    for a, want in zip(areas.tolist(), TETRA_AREAS):
        assert abs(a - want) <= 1e-6 * want
    dev_areas = renderer.sectionAreas(sc, torch.from_numpy(TETRA_PLANES[:, 0:3].copy()).to(DEV), torch.from_numpy(TETRA_PLANES[:, 3].copy()).to(DEV))
    assert dev_areas.device == torch.device(DEV) and dev_areas.dtype == torch.float64 and (dev_areas.cpu().numpy() == areas).all()
    # the cube at z = 0.25: the area of a face
    cube, gc = scene_pair("cube")
    face = float((nr.bounds(gc)[1][0] - nr.bounds(gc)[0][0]) * (nr.bounds(gc)[1][1] - nr.bounds(gc)[0][1]))
    a = renderer.sectionAreas(cube, sr.pack([(0, 0, 1), (0, 0, -2)], [0.25, -0.5]))
    assert abs(a[0] - face) <= 1e-6 * face and abs(a[1] - face) <= 1e-6 * face
    # slices: the cell centres of the scene's bounds along the axis, and planeSections at those heights
    for name, count, axis in (("tetrahedron", 8, 2), ("cornell_box", 33, 1), ("soup", 70, 0)):
        s, gg = scene_pair(name)
        heights, lst = renderer.slices(s, count, axis=axis)
        assert heights.device == torch.device(DEV) and heights.dtype == torch.float32 and tuple(heights.shape) == (count,)
        nodes = s.m_BVHNodes
        lo, hi = float(nodes[-1]["bmin"][axis]), float(nodes[-1]["bmax"][axis])
        got_h = heights.cpu().numpy()
        assert np.allclose(got_h, lo + (np.arange(count) + 0.5) * (hi - lo) / count, rtol=1e-6, atol=1e-6 * (hi - lo))   # the cell centres
        planes = np.zeros((count, 4), np.float32)
        planes[:, axis], planes[:, 3] = 1, got_h
        same = renderer.planeSections(s, planes)                                # at its own heights
        assert all(a.cpu().numpy().tobytes() == b.tobytes() for a, b in zip(lst, same))
        full, totals = sr.whole(gg, planes)
        assert as_records(same).tobytes() == full.tobytes() and totals.min() > 0
    heights, lst = renderer.slices(scene_pair("cube")[0], 4, axis=2, lo=0.0, hi=1.0)
    assert heights.cpu().tolist() == [0.125, 0.375, 0.625, 0.875] and (lst.splits.cpu().numpy() == [0, 8, 16, 16, 16]).all()


def test_queries_leave_the_renderer_alone_and_work_on_a_sharded_one(renderer):
    sc, g = scene_pair("cornell_box")
    planes = sweep_planes(g, 100, 21)
    full, totals = sr.whole(g, planes)
    _, pos, fwd, depth = SCENES["cornell_box"]
    cam = drt.Camera(pos)
    cam.m_Forward_dir = np.array(fwd, np.float32)
    images = []
    for with_queries in (False, True):
        r = drt.Renderer(0)
        r.m_RendererSettings = drt.RendererSettings(ray_bounce_limit=depth)
        r.ResizeBuffer(96, 64)
        r.Render(cam, sc)
        if with_queries:
            info, frame, accum, n, span = r.kernelInfo(), r.GetRenderTargetImage(), r.GetAccumulationBuffer(), r.getSampleCount(), r.kernelSpanMs()
            counters = bytes(r.getCounters())
            assert as_records(r.planeSections(sc, planes)).tobytes() == full.tobytes() and (r.cutsAny(sc, planes) == (totals > 0)).all()
            r.sectionAreas(sc, planes), r.slices(sc, 5)
            assert r.kernelInfo() == info and r.getSampleCount() == n and r.kernelSpanMs() == span
            assert bytes(r.getCounters()) == counters
            assert r.GetRenderTargetImage().tobytes() == frame.tobytes() and r.GetAccumulationBuffer().tobytes() == accum.tobytes()
        r.Render(cam, sc)
        images.append((r.GetRenderTargetImage(), r.getSampleCount()))
    assert images[0][0].tobytes() == images[1][0].tobytes() and images[0][1] == images[1][1]
    r = drt.Renderer(0)
    r.setShard(8, 1, 2)
    r.ResizeBuffer(96, 64)
    assert as_records(r.planeSections(sc, planes)).tobytes() == full.tobytes()


def test_an_empty_scene_lists_nothing(renderer):
    sc = drt.Scene()
    sc.addMaterial(*ONE_MATERIAL[0])
    sc.setGeometry(np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 2), np.float32), np.zeros(0, np.int32))
    drt.BVHBuilder().buildIterative(sc)
    planes = sr.pack(np.eye(3, dtype=np.float32), [0, 1, 2])
    got = renderer.planeSections(sc, planes)
    assert got.splits.tolist() == [0, 0, 0, 0] and len(got.prim) == 0 and got.p.shape == (0, 3)
    assert not renderer.cutsAny(sc, planes).any() and (renderer.sectionAreas(sc, planes) == 0).all()
    rec, counts = run_raw(renderer, sc, planes, [0, 2, 4, 6], 6, 6)
    assert rec.tobytes() == np.repeat(sr.MISS, 6).tobytes() and not counts.any()


def test_error_paths(renderer):
    sc, g = scene_pair("cornell_box")
    dev = torch.device(DEV)
    n = 64
    planes = torch.zeros((n + 1, 4), dtype=torch.float32, device=dev)
    planes[:, 1], planes[:, 3] = 1, 1                                            # y = 1
    offsets = (torch.arange(n + 2, dtype=torch.int32, device=dev) * 2)
    out = torch.full((2 * n + 8, 8), SENTINEL, dtype=torch.int32, device=dev)
    counts = torch.full((n + 1,), -1, dtype=torch.int32, device=dev)
    host = np.zeros((2 * n + 8, 8), np.float32)
    L, h = drt._lib, renderer._h
    INV = drt.ERR_INVALID
    cap = 2 * n
    B, O, P, C, H = planes.data_ptr(), offsets.data_ptr(), out.data_ptr(), counts.data_ptr(), host.ctypes.data
    for what, args in (("null planes", (h, sc._h, None, O, P, cap, C, n, 0)), ("null offsets", (h, sc._h, B, None, P, cap, C, n, 0)),
                       ("null renderer", (None, sc._h, B, O, P, cap, C, n, 0)), ("null scene", (h, None, B, O, P, cap, C, n, 1)),
                       ("mode 2", (h, sc._h, B, O, P, cap, C, n, 2)), ("mode -1", (h, sc._h, B, O, P, cap, C, n, -1)),
                       ("mode 2, n = 0", (h, sc._h, B, O, P, cap, C, 0, 2)), ("mode 2, null planes", (h, sc._h, None, O, P, cap, C, n, 2)),
                       ("both outputs null", (h, sc._h, B, O, None, 0, None, n, 0)), ("null out with a capacity", (h, sc._h, B, O, None, cap, C, n, 0)),
                       ("out without a capacity", (h, sc._h, B, O, P, 0, C, n, 0)),
                       ("any with out", (h, sc._h, B, O, P, cap, C, n, 1)), ("any with a capacity", (h, sc._h, B, O, None, cap, C, n, 1)),
                       ("any without counts", (h, sc._h, B, O, None, 0, None, n, 1)),
                       ("misaligned planes", (h, sc._h, B + 4, O, P, cap, C, n, 0)), ("misaligned out", (h, sc._h, B, O, P + 8, cap, C, n, 0)),
                       ("misaligned offsets", (h, sc._h, B, O + 2, P, cap, C, n, 0)), ("misaligned counts", (h, sc._h, B, O, P, cap, C + 1, n, 0)),
                       ("host planes", (h, sc._h, H, O, P, cap, C, n, 0)), ("host offsets", (h, sc._h, B, H, P, cap, C, n, 0)),
                       ("host out", (h, sc._h, B, O, H, cap, C, n, 0)), ("host counts", (h, sc._h, B, O, P, cap, H, n, 0)),
                       ("host counts, any", (h, sc._h, B, None, None, 0, H, n, 1)), ("null handles, n = 0", (None, None, B, O, P, cap, C, 0, 0))):
        assert L.drt_renderer_plane_sections(*args, None) == INV, what
        if what.startswith("mode"):
            assert b"mode" in L.drt_last_error(), what                                                    # checked first after the handles
    for mode in (0, 1):
        assert L.drt_renderer_plane_sections(h, sc._h, None, None, None, 0, None, 0, mode, None) == drt.OK    # n == 0: nothing to do
        assert L.drt_renderer_plane_sections(h, sc._h, B, O, P, cap, C, 0, mode, None) == drt.OK
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (counts == -1).all()                                                # nothing was launched
    # planes and out need 16-byte alignment, the rest 4: one plane, one record and one word further on
    assert L.drt_renderer_plane_sections(h, sc._h, B + 16, O + 4, P + 32, cap + 2, C + 4, n, 0, None) == drt.OK
    torch.cuda.synchronize()
    assert (out[0:1 + 2] == SENTINEL).all() and (out[1 + 2 + 2 * n:] == SENTINEL).all()
    assert not (out[1 + 2:1 + 2 + 2 * n, 3] == SENTINEL).any() and counts[0] == -1 and (counts[1:] >= 0).all()
    empty = renderer.planeSections(sc, np.zeros((0, 4), np.float32))
    assert empty.splits.tolist() == [0] and len(empty.prim) == 0
    assert renderer.cutsAny(sc, np.zeros((0, 3), np.float32), np.zeros(0, np.float32)).shape == (0,)
    assert renderer.sectionAreas(sc, np.zeros((0, 4), np.float32)).shape == (0,)
    for bad in (lambda: renderer.planeSections(sc, planes.cpu()),                                        # wrong device
                lambda: renderer.planeSections(sc, planes.double()),                                     # wrong dtype
                lambda: renderer.planeSections(sc, planes[:, :2]),                                       # wrong shape
                lambda: renderer.planeSections(sc, planes[:, :3]),                                       # normals without d
                lambda: renderer.planeSections(sc, planes, planes[:, 3]),                                # packed planes carry their d
                lambda: renderer.planeSections(sc, planes[:, :3], planes[:5, 3]),                        # d of another length
                lambda: renderer.planeSections(sc, planes[:, :3], host[:n + 1, 0].copy()),               # a mix of torch and numpy
                lambda: renderer.planeSections(sc, planes.tolist()),                                     # neither numpy nor torch
                lambda: renderer.cutsAny(sc, planes.cpu()),
                lambda: renderer.sectionAreas(sc, host[:, :4].astype(np.float64)),
                lambda: renderer.slices(sc, 0), lambda: renderer.slices(sc, 4, axis=5)):
        with pytest.raises(drt.DrtError) as e:
            bad()
        assert e.value.code == INV
    # a pending asynchronous batch
    r = drt.Renderer(0)
    r.ResizeBuffer(64, 32)
    r.RenderBatchAsync(drt.Camera(SCENES["cornell_box"][1]), sc, 1)
    for call in (lambda: r.planeSections(sc, planes), lambda: r.cutsAny(sc, planes)):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == INV
    assert raw(r, sc, planes, offsets, out, cap, counts, n, 0) == INV
    r.Wait()
    r.planeSections(sc, planes), r.cutsAny(sc, planes)
    # a tree deeper than 64 levels: the chain's centroids double per triangle (scaled down so that no area overflows)
    chain = list(rq.degenerate_chain(110))
    chain[0] = (chain[0] * np.float32(2.0 ** -55)).astype(np.float32)
    deep, _ = rq.programmatic_scene(drt, *chain, 1, 2)
    assert deep.bvh_depth > 64
    for call in (lambda: renderer.planeSections(deep, planes), lambda: renderer.cutsAny(deep, planes)):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == drt.ERR_UNSUPPORTED
    full, totals = sr.whole(g, planes.cpu().numpy())
    assert as_records(drt.SectionList(*(x.cpu().numpy() for x in renderer.planeSections(sc, planes)))).tobytes() == full.tobytes()   # after the errors
