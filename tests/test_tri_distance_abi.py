"""The triangle-distance entry point of include/drt.h without a GPU: exported, bound, laid out as declared, the argument checks that come
before any device work, the header states the rule and its limits, and the C++ wrapper compiles and links against it."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.scenes import ROOT

drt = pytest.importorskip("dustraytracer_amd")


def test_the_symbol_is_exported_and_bound():
    lib = ctypes.CDLL(drt.LIB_PATH)
    assert hasattr(lib, "drt_renderer_triangle_distance")
    fn = drt._lib.drt_renderer_triangle_distance
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 8
    assert fn.argtypes[5] is ctypes.c_uint32 and fn.argtypes[6] is ctypes.c_int32                     # n, mode
    assert all(fn.argtypes[i] is ctypes.c_void_p for i in (0, 1, 2, 3, 4, 7))
    for method in ("triangleDistance", "withinDistance", "meshDistance"):
        assert callable(getattr(drt.Renderer, method)), method
    assert drt.TriNearest._fields == ("d2", "prim", "point_q", "point_t", "u", "v", "feature")
    assert drt.MeshDistance._fields == ("d2", "query", "prim", "point_q", "point_t", "feature")
    assert (drt.TRIDIST_NEAREST, drt.TRIDIST_ANY) == (0, 1)
    for method in ("triangleDistance", "meshDistance"):
        assert "penetration depth" in getattr(drt.Renderer, method).__doc__
    assert drt._lib.drt_abi_version() == 2


def test_record_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "drt.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu\n", sizeof(drt_tri_near), offsetof(drt_tri_near, point_q), offsetof(drt_tri_near, d2), offsetof(drt_tri_near, point_t),
           offsetof(drt_tri_near, prim));
    printf("%zu %zu %zu %zu\n", offsetof(drt_tri_near, u), offsetof(drt_tri_near, v), offsetof(drt_tri_near, feature), offsetof(drt_tri_near, pad));
    printf("%zu %d %d %d\n", sizeof(drt_tri), DRT_TRIDIST_NEAREST, DRT_TRIDIST_ANY, DRT_ABI_VERSION);
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["48", "0", "12", "16", "28", "32", "36", "40", "44", "48", "0", "1", "2"]


def test_the_argument_checks_come_in_the_overlap_query_s_order():
    L = drt._lib
    sc = drt.Scene()
    fn = L.drt_renderer_triangle_distance
    assert fn(None, sc._h, None, None, None, 4, 0, None) == drt.ERR_INVALID
    assert b"null" in L.drt_last_error()
    assert fn(None, None, None, None, None, 0, 1, None) == drt.ERR_INVALID            # the handles are checked before n == 0
    assert fn(None, sc._h, None, None, None, 4, 7, None) == drt.ERR_INVALID           # ... and before the mode
    assert b"null" in L.drt_last_error()
    # the mode is checked first after the handles, before n == 0 and before the renderer is looked at: a block of zeros stands in for it
    stand_in = ctypes.create_string_buffer(1 << 16)
    h = ctypes.addressof(stand_in)
    for mode in (2, -1, 7):
        for n in (0, 4):
            assert fn(h, sc._h, None, None, None, n, mode, None) == drt.ERR_INVALID
            assert b"mode" in L.drt_last_error()
    tris = ctypes.create_string_buffer(48 * 4 + 16)
    B = (ctypes.addressof(tris) + 15) & ~15
    out = ctypes.create_string_buffer(48 * 4 + 16)
    O = (ctypes.addressof(out) + 15) & ~15
    words = ctypes.create_string_buffer(64)
    W = (ctypes.addressof(words) + 15) & ~15
    for mode in (0, 1):
        assert fn(h, sc._h, None, None, None, 0, mode, None) == drt.OK                 # n == 0: nothing to do
        for what, args in (("null tris", (None, W, O)), ("null out", (B, W, None)), ("both null", (None, None, None))):
            assert fn(h, sc._h, *args, 4, mode, None) == drt.ERR_INVALID, what
            assert b"null triangle or result" in L.drt_last_error(), what
        for what, args in (("misaligned tris", (B + 4, W, O)), ("misaligned out", (B, W, O + 8)), ("misaligned max_dist", (B, W + 2, O)),
                           ("misaligned tris, no max_dist", (B + 8, None, O))):
            assert fn(h, sc._h, *args, 4, mode, None) == drt.ERR_INVALID, what
            assert b"aligned" in L.drt_last_error(), what
        assert fn(h, sc._h, B, None, O, 0x80000000, mode, None) == drt.ERR_INVALID
        assert b"2^31" in L.drt_last_error()


def test_bad_arguments_are_refused_before_any_device_work():
    r = drt.Renderer.__new__(drt.Renderer)                                     # (no device: only the argument check runs)
    r._device = 0
    sc = drt.Scene()
    for call in (lambda: r.triangleDistance(sc, np.zeros((3, 3, 3), np.float64)), lambda: r.withinDistance(sc, [[0] * 12], 1.0),
                 lambda: r.meshDistance(sc, np.zeros((3, 9), np.float32))):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == drt.ERR_INVALID and "tris" in str(e.value)


def test_the_header_states_the_rule_and_its_limits():
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    sec = text[text.index("triangle distance queries (new"):text.index("typedef struct drt_tri_near ")]
    flat = re.sub(r" +", " ", re.sub(r"\s*\n \*\s*", " ", sec))
    for phrase in ("48 bytes, 16-byte aligned", "the three pad words are ignored", "infinite when max_dist is NULL", "A mesh is a batch of queries",
                   "fp32 with one rounding per operation, in the order written", "dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z",
                   "the correctly rounded division", "there is no tolerance anywhere",
                   "Validity and bounds are drt_renderer_overlap_triangles', unchanged", "valid iff all nine coordinates satisfy fabsf(x) <= FLT_MAX",
                   "An invalid query pushes nothing and gets the miss record", "relative to q0 as the overlap test is",
                   "a1 = q1 - q0, a2 = q2 - q0, g = a2 - a1", "p0 = v0 - q0, p1 = p0 + e1, p2 = p0 + e2, h = e2 - e1", "Fifteen candidates, in this order",
                   "0..2 the query's vertices 0, a1, a2 against the scene triangle (p0, e1, e2)", "the seven cases of drt_renderer_nearest",
                   "3..5 the scene triangle's vertices p0, p1, p2 against the query triangle (0, a1, a2)",
                   "query edge i of ((0, a1), (a1, g), (a2, -a2)) against scene edge j of ((p0, e1), (p1, h), (p2, -e2))", "candidate 6 + 3 i + j",
                   "Ericson, Real-Time Collision Detection 5.1.9", "exact-zero degenerate cases and no epsilon",
                   "r = P1 - P2, a = dot(d1, d1), e = dot(d2, d2), f = dot(d2, r), c = dot(d1, r), b = dot(d1, d2), den = a e - b b",
                   "clamp(x) = fminf(fmaxf(x, 0), 1) + 0", "a <= 0 && e <= 0: s = t = 0", "a <= 0: s = 0, t = clamp(f / e)",
                   "e <= 0: t = 0, s = clamp(-c / a)", "s = den > 0 ? clamp((b f - c e) / den) : 0 and t = (b s + f) / e",
                   "if t < 0 then t = 0 and s = clamp(-c / a)", "t > 1 then t = 1 and s = clamp((b - c) / a)",
                   "c1 = P1 + d1 s", "c2 = P2 + d2 t", "dist2 = dot(diff, diff)", "replaces them iff its dist2 < d2",
                   "the first wins a tie and a NaN never wins", "never understates the true distance by more than rounding",
                   "d2 = 0 and feature = candidate | 16", "NOT a contact point", "cannot see an edge that pierces the interior of a large triangle",
                   "conservatism on zero-area triangles is inherited", "d = fmaxf(fmaxf(bmin - qmax, 0), qmin - bmax)", "box2 = (dx dx + dy dy) + dz dz",
                   "drt_renderer_nearest's, word for word", "best = max_dist * max_dist, prim = -1", "dropped unless box2 < best",
                   "a pair replaces the result iff d2 < best", "the farther one first (b1 > b2 -> child 1)", "touching meshes end early",
                   "DRT_TRIDIST_NEAREST is the search above", "DRT_TRIDIST_ANY ends a query at the first pair with d2 < best",
                   "not the nearest", "point_q = q0 + c_query and point_t = q0 + c_scene", "(0, 0), (1, 0), (0, 1) for 3, 4, 5",
                   "(t, 0) on scene edge 0, (1 - t, t) on edge 1, (0, 1 - t) on edge 2", "all zero with d2 = max_dist * max_dist and prim = -1",
                   "a refitted device copy is the one queried", "the 64-level bound", "counters, kernel info and kernel span are not touched"):
        assert phrase in flat, phrase
    limits = flat[flat.index("What this is not:"):]
    for phrase in ("no penetration depth", "the conservative overlap predicate does not separate the pair", "no self-clearance",
                   "no k-nearest or within-distance list", "alpha cut-outs are ignored"):
        assert phrase in limits, phrase
    before = re.sub(r"\s*\n \*\s*", " ", text[:text.index("#define DRT_ABI_VERSION 2")])
    assert "the triangle-distance entry point (drt_renderer_triangle_distance)" in before
    # the working range paragraph names the query and the measured range, which tests/test_tri_distance_ref.py asserts
    from tests.test_tri_distance_ref import SCALE_RANGE
    rng = re.sub(r"\s*\n \*\s*", " ", text[text.index("working range of the mesh queries"):text.index("intersection curves (new")])
    assert "drt_renderer_triangle_distance:" in rng and "unchanged for 2^%d to 2^%d" % SCALE_RANGE in rng[rng.index("drt_renderer_triangle_distance:"):]


def test_cpp_wrapper_compiles_and_links(tmp_path):
    src = tmp_path / "tri_distance_calls.cpp"
    src.write_text(r"""
#include <cstdio>
#include "DustRayTracer.hpp"
// the statements only -- main() runs none of them without arguments
int main(int argc, char **) {
    if (argc < 2) { std::printf("%zu %zu %d\n", sizeof(drt_tri_near), alignof(drt_tri_near), DRT_ABI_VERSION); return 0; }
    Scene scene;
    Renderer r(0);
    const drt_tri *tris = nullptr;
    const float *max_dist = nullptr;
    drt_tri_near *out = nullptr;
    r.TriangleDistance(scene, tris, max_dist, out, 0u);
    r.TriangleDistance(scene, tris, nullptr, out, 0u, DRT_TRIDIST_ANY, nullptr);
    return 0;
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    exe = tmp_path / "tri_distance_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib_dir, "-ldrt_hip",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["48", "4", "2"]
