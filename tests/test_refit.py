"""The host half of the BVH refit: the triangle order (drt_scene_get_triangle_order) through every build, and drt_scene_refit
against the restatement in tests/refit_ref.py -- triangles and node boxes bit for bit, topology untouched, errors that leave the
scene as it was.  The C++ wrapper's new members compile, link and run.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import ray_query_ref as rq
from tests import refit_ref as rf
from tests.scenes import ROOT, scene_path

drt = pytest.importorskip("dustraytracer_amd")

FILE_SCENES = ["cornell_box", "suzanne_plane", "uv_texture_test", "multi_material", "mc_transparency", "bvh_split_test",
               "scene_hier_test", "cs16_dust", "cornell_box_gltf"]
TOPOLOGY = ("is_leaf", "child1", "child2", "prim_count", "prim_start")


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def build(sc, leaf, bins, recursive=False):
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = leaf, bins
    (b.build if recursive else b.buildIterative)(sc)
    return sc


def scene(name, recursive=False):
    """(scene with the editor's BVH, its load-order streams)."""
    if name == "soup":
        s = rq.soup(90000, 1, spread=10.0)
        sc, _ = rq.programmatic_scene(drt, *s, 2, 8)
        return sc, (s[0], s[1], s[2], s[3])
    if name == "chain":
        s = rq.degenerate_chain()
        sc, _ = rq.programmatic_scene(drt, *s, 1, 2)
        return sc, (s[0], s[1], s[2], s[3])
    sc = drt.Scene()
    sc.loadGLTFmodel(scene_path(name))
    st = rf.streams(sc.m_PrimitivesBuffer)
    return build(sc, 20, 8, recursive), st


def assert_triangles_equal(tris, ref, what):
    """Product triangles against oracle records, every field bit for bit (a NaN face normal equals a NaN)."""
    v = tris["vertex"]
    for got, want, field in ((v["position"], ref["p"], "position"), (v["normal"], ref["n"], "normal"), (v["uv"], ref["uv"], "uv"),
                             (tris["centroid"], ref["centroid"], "centroid")):
        bad = (u32(got) != u32(want)).reshape(len(tris), -1).any(axis=1)
        assert not bad.any(), "%s: %s differs on %d triangles, first %d" % (what, field, bad.sum(), np.argmax(bad))
    fn, rfn = tris["face_normal"], ref["face_n"]
    bad = ((u32(fn) != u32(rfn)) & ~(np.isnan(fn) & np.isnan(rfn))).any(axis=1)
    assert not bad.any(), "%s: face normal differs on %d triangles" % (what, bad.sum())
    assert (tris["material"] == ref["material"]).all(), what


def assert_nodes_equal(got, want, what):
    for f in TOPOLOGY:
        assert np.array_equal(got[f], want[f]), (what, f)
    for f in ("bmin", "bmax"):
        bad = (u32(got[f]) != u32(want[f])).any(axis=1)
        assert not bad.any(), "%s: %s differs on %d nodes, first %d: %r vs %r" % (what, f, bad.sum(), np.argmax(bad), got[f][np.argmax(bad)], want[f][np.argmax(bad)])


@pytest.mark.parametrize("recursive", [False, True])
@pytest.mark.parametrize("name", FILE_SCENES + ["chain"])
def test_triangle_order_names_the_load_order(name, recursive):
    sc = drt.Scene()
    if name == "chain":
        s = rq.degenerate_chain()
        for alb, tex in s[4]:
            sc.addMaterial(alb, tex)
        sc.setGeometry(*s[:4])
    else:
        sc.loadGLTFmodel(scene_path(name))
    loaded = sc.m_PrimitivesBuffer
    assert np.array_equal(sc.triangleOrder(), np.arange(len(loaded)))          # identity on load
    build(sc, *((1, 2) if name == "chain" else (20, 8)), recursive=recursive)
    order = sc.triangleOrder()
    assert order.dtype == np.int32 and np.array_equal(np.sort(order), np.arange(len(loaded)))
    tris = sc.m_PrimitivesBuffer
    rows = loaded.view(np.uint8).reshape(len(loaded), -1)                    # (a structured gather would not copy the padding)
    assert tris.tobytes() == rows[order].tobytes(), name
    assert_triangles_equal(tris, rf.triangles(*rf.streams(loaded), order=order), name)


def test_set_geometry_extends_the_order():
    pos, nrm, uv, mat, materials, _ = rq.soup(500, 3)
    sc = drt.Scene()
    for alb, _ in materials:
        sc.addMaterial(alb, -1)
    sc.setGeometry(pos, nrm, uv, np.zeros(500, np.int32))
    build(sc, 4, 8)
    first = sc.triangleOrder()
    assert not np.array_equal(first, np.arange(500))
    sc.setGeometry(pos[:100], nrm[:100], uv[:100], np.zeros(100, np.int32))    # replaces the geometry: identity again
    assert np.array_equal(sc.triangleOrder(), np.arange(100))


@pytest.mark.parametrize("name", FILE_SCENES + ["soup", "chain"])
def test_refit_to_the_same_positions_reproduces_the_build(name):
    sc, st = scene(name)
    tris0, nodes0 = sc.m_PrimitivesBuffer, sc.m_BVHNodes
    sc.refit(st[0])
    assert sc.m_PrimitivesBuffer.tobytes() == tris0.tobytes(), name
    nodes1 = sc.m_BVHNodes
    for f in TOPOLOGY:
        assert np.array_equal(nodes1[f], nodes0[f]), (name, f)
    for f in ("bmin", "bmax"):
        assert np.array_equal(nodes1[f], nodes0[f]), (name, f)                 # equal as floats ...
        bits = u32(nodes1[f]) != u32(nodes0[f])
        assert not (bits & (nodes0[f] != 0)).any(), (name, f)                  # ... and bit for bit but for the sign of a zero
    assert_nodes_equal(nodes1, rf.nodes(nodes0, tris0["vertex"]["position"]), name)


def moved(name, st, how, rng):
    """(positions, normals or None) of a move of the load-order streams st."""
    pos, nrm = st[0].copy(), st[1].copy()
    if how == "jitter":
        return (pos + rng.normal(0, 0.01, pos.shape)).astype(np.float32), None
    if how in ("rotate", "rotate_normals"):
        a = 0.3
        rot = np.float32([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        p = (pos @ rot.T + np.float32([0.5, -0.25, 1.0])).astype(np.float32)
        return p, ((nrm @ rot.T).astype(np.float32) if how == "rotate_normals" else None)
    if how == "one_mesh":                    # a mesh's range (drt_mesh) moves, the others stay (else the first third)
        m = st[4] if len(st) > 4 else (0, len(pos) // 3)
        pos[m[0]:m[0] + m[1]] += np.float32([0.0, 0.75, -0.5])
        return pos, None
    if how == "collapse":                    # triangle 3 shrinks to a point; triangle 5 to a line
        pos[3] = pos[3, 0]
        pos[5, 2] = pos[5, 0] + (pos[5, 1] - pos[5, 0]) * np.float32(0.5)
        return pos, None
    raise ValueError(how)


@pytest.mark.parametrize("how", ["jitter", "rotate", "rotate_normals", "one_mesh", "collapse"])
@pytest.mark.parametrize("name", ["cornell_box", "scene_hier_test", "cs16_dust", "soup", "chain"])
def test_refit_matches_the_restatement(name, how):
    sc, st = scene(name)
    meshes = sc.m_Meshes
    if len(meshes) > 1:                      # cornell_box, scene_hier_test: one mesh of several moves
        st = st + (tuple(int(v) for v in meshes[len(meshes) // 2]),)
    order, nodes0 = sc.triangleOrder(), sc.m_BVHNodes
    pos, nrm = moved(name, st, how, np.random.default_rng(11))
    sc.refit(pos, nrm)
    ref_tris = rf.triangles(pos, nrm if nrm is not None else st[1], st[2], st[3], order=order)
    tris = sc.m_PrimitivesBuffer
    assert_triangles_equal(tris, ref_tris, "%s %s" % (name, how))
    assert_nodes_equal(sc.m_BVHNodes, rf.nodes(nodes0, pos[order]), "%s %s" % (name, how))
    assert np.array_equal(sc.triangleOrder(), order)
    if how == "collapse":
        assert np.isnan(tris["face_normal"][np.nonzero(order == 3)[0][0]]).all()


def test_two_refits_equal_one_to_the_final_positions():
    rng = np.random.default_rng(5)
    a, st = scene("cs16_dust")
    b, _ = scene("cs16_dust")
    p1 = (st[0] + rng.normal(0, 0.05, st[0].shape)).astype(np.float32)
    p2 = (st[0] + rng.normal(0, 0.05, st[0].shape)).astype(np.float32)
    n1 = (st[1] * np.float32(-1)).astype(np.float32)                           # normals given once, then kept
    a.refit(p1, n1)
    a.refit(p2)
    b.refit(p2, n1)
    assert a.m_PrimitivesBuffer.tobytes() == b.m_PrimitivesBuffer.tobytes()
    assert a.m_BVHNodes.tobytes() == b.m_BVHNodes.tobytes()


def test_refit_errors_leave_the_scene_unchanged():
    sc = drt.Scene()
    sc.loadGLTFmodel(scene_path("cornell_box"))
    pos = rf.streams(sc.m_PrimitivesBuffer)[0]
    with pytest.raises(drt.DrtError) as e:                                      # no BVH
        sc.refit(pos)
    assert e.value.code == drt.ERR_INVALID
    build(sc, 20, 8)
    assert drt._lib.drt_scene_refit(sc._h, None, None) == drt.ERR_INVALID
    assert drt._lib.drt_scene_refit(None, pos.ctypes.data, None) == drt.ERR_INVALID
    tris0, nodes0 = sc.m_PrimitivesBuffer.tobytes(), sc.m_BVHNodes.tobytes()
    moved_pos = pos + np.float32(1)
    for bad, where in ((np.nan, "positions"), (np.inf, "positions"), (-np.inf, "normals")):
        p, n = moved_pos.copy(), rf.streams(sc.m_PrimitivesBuffer)[1].copy()
        (p if where == "positions" else n)[7, 1, 2] = bad
        with pytest.raises(drt.DrtError) as e:
            sc.refit(p, n)
        assert e.value.code == drt.ERR_INVALID and "non-finite" in str(e.value)
        assert sc.m_PrimitivesBuffer.tobytes() == tris0 and sc.m_BVHNodes.tobytes() == nodes0
    with pytest.raises(drt.DrtError):
        sc.refit(pos[:-1])                                                      # wrong size (caught by the binding)


def test_cpp_wrapper_refit_members(tmp_path):
    src = tmp_path / "refit.cpp"
    src.write_text(r'''
#include "DustRayTracer.hpp"
#include <cstdio>
int main() {
    Scene scene;
    float pos[2 * 9] = { 0, 0, 0, 1, 0, 0, 0, 1, 0,   5, 0, 0, 6, 0, 0, 5, 1, 0 };
    float nrm[2 * 9] = { 0, 0, 1, 0, 0, 1, 0, 0, 1,   0, 0, 1, 0, 0, 1, 0, 0, 1 };
    float uv[2 * 6] = { 0 };
    int32_t mat[2] = { 0, 0 };
    const float albedo[3] = { 1, 1, 1 };
    drt_scene_add_material(scene.handle, albedo, -1);
    drt::check(drt_scene_set_geometry(scene.handle, pos, nrm, uv, mat, 2));
    BVHBuilder b;
    b.m_TargetLeafPrimitivesCount = 1; b.m_BinCount = 4;
    b.buildIterative(scene);
    for (float &p : pos) p *= 2;
    scene.Refit(pos);
    std::vector<int32_t> order = scene.TriangleOrder();
    std::vector<drt_bvh_node> nodes = scene.bvhNodes();
    std::printf("%d %d %g %g\n", (int)order.size(), order[0] + order[1], nodes.back().bmin[0], nodes.back().bmax[0]);
    Renderer *unused = nullptr;
    if (unused) unused->Refit(scene, pos);
    return 0;
}
''')
    exe = tmp_path / "refit"
    cmd = ["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src),
           "-L" + os.path.join(ROOT, "dustraytracer_amd"), "-ldrt_hip", "-Wl,-rpath," + os.path.join(ROOT, "dustraytracer_amd"),
           "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["2", "1", "0", "12"]
