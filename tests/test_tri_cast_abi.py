"""The triangle-cast entry point of include/drt.h without a GPU: exported, bound, laid out as declared, the argument checks that come
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
    assert hasattr(lib, "drt_renderer_triangle_cast")
    fn = drt._lib.drt_renderer_triangle_cast
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 8
    assert fn.argtypes[5] is ctypes.c_uint32 and fn.argtypes[6] is ctypes.c_int32                     # n, mode
    assert all(fn.argtypes[i] is ctypes.c_void_p for i in (0, 1, 2, 3, 4, 7))
    for method in ("triangleCast", "castsAny", "meshCast"):
        assert callable(getattr(drt.Renderer, method)), method
    assert drt.TriHits._fields == ("t", "prim", "point", "normal", "u", "v", "feature")
    assert drt.MeshHit._fields == ("t", "query", "prim", "point", "normal", "feature")
    assert (drt.TRICAST_FIRST, drt.TRICAST_ANY) == (0, 1)
    for method in ("triangleCast", "meshCast"):
        doc = getattr(drt.Renderer, method).__doc__
        assert "penetration depth" in doc and "rotation" in doc
    assert drt._lib.drt_abi_version() == 2


def test_record_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "drt.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu\n", sizeof(drt_tri_hit), offsetof(drt_tri_hit, point), offsetof(drt_tri_hit, t), offsetof(drt_tri_hit, normal),
           offsetof(drt_tri_hit, prim));
    printf("%zu %zu %zu %zu\n", offsetof(drt_tri_hit, u), offsetof(drt_tri_hit, v), offsetof(drt_tri_hit, feature), offsetof(drt_tri_hit, pad));
    printf("%zu %zu %zu\n", sizeof(drt_motion), offsetof(drt_motion, d), offsetof(drt_motion, tmax));
    printf("%zu %d %d %d\n", sizeof(drt_tri), DRT_TRICAST_FIRST, DRT_TRICAST_ANY, DRT_ABI_VERSION);
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["48", "0", "12", "16", "28", "32", "36", "40", "44", "16", "0", "12", "48", "0", "1", "2"]


def test_the_argument_checks_come_in_the_distance_query_s_order():
    L = drt._lib
    sc = drt.Scene()
    fn = L.drt_renderer_triangle_cast
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
    motions = ctypes.create_string_buffer(16 * 4 + 16)
    M = (ctypes.addressof(motions) + 15) & ~15
    for mode in (0, 1):
        assert fn(h, sc._h, None, None, None, 0, mode, None) == drt.OK                 # n == 0: nothing to do
        for what, args in (("null tris", (None, M, O)), ("null motions", (B, None, O)), ("null out", (B, M, None)), ("all null", (None, None, None))):
            assert fn(h, sc._h, *args, 4, mode, None) == drt.ERR_INVALID, what
            assert b"null triangle, motion or result" in L.drt_last_error(), what
        for what, args in (("misaligned tris", (B + 4, M, O)), ("misaligned out", (B, M, O + 8)), ("misaligned motions", (B, M + 4, O)),
                           ("motions 8-byte aligned only", (B, M + 8, O))):
            assert fn(h, sc._h, *args, 4, mode, None) == drt.ERR_INVALID, what
            assert b"16-byte aligned" in L.drt_last_error(), what
        assert fn(h, sc._h, B, M, O, 0x80000000, mode, None) == drt.ERR_INVALID
        assert b"2^31" in L.drt_last_error()


def test_bad_arguments_are_refused_before_any_device_work():
    r = drt.Renderer.__new__(drt.Renderer)                                     # (no device: only the argument check runs)
    r._device = 0
    sc = drt.Scene()
    d = np.float32([0, 0, -1])
    for call in (lambda: r.triangleCast(sc, np.zeros((3, 3, 3), np.float64), d), lambda: r.castsAny(sc, [[0] * 12], d, 1.0),
                 lambda: r.meshCast(sc, np.zeros((3, 9), np.float32), d)):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == drt.ERR_INVALID and "tris" in str(e.value)


def test_the_header_states_the_rule_and_its_limits():
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    sec = text[text.index("triangle casts (new"):text.index("typedef struct drt_motion ")]
    flat = re.sub(r" +", " ", re.sub(r"\s*\n \*\s*", " ", sec))
    for phrase in ("48 bytes, 16-byte aligned", "the three pad words are ignored", "a drt_motion {d[3], tmax} (16 bytes, 16-byte aligned)",
                   "The triangle is at q + d t", "the smallest t in [0, tmax)", "There is no tmin", "t is a quotient and not a sum",
                   "fp32 with one rounding per operation, in the order written", "dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z",
                   "the correctly rounded division", "no tolerance and no thickness anywhere",
                   "all nine coordinates satisfy fabsf(x) <= FLT_MAX", "no component of d and not tmax is a NaN",
                   "An invalid cast pushes nothing and gets the miss record", "relative to q0 as the distance query is",
                   "a1 = q1 - q0, a2 = q2 - q0, g = a2 - a1, nq = cross(a1, a2)", "p0 = v0 - q0, p1 = p0 + e1, p2 = p0 + e2, h = e2 - e1",
                   "sg = det < 0 ? -1 : 1 and ad = fabsf(det)", "every numerator is multiplied by sg (exact)",
                   "compares a numerator with 0 or with ad, all closed", "a parameter is fabsf(numerator) / ad, one division",
                   "no reciprocal is taken", "A NaN fails every test", "det = 0 has no candidate", "Fifteen candidates, in this order",
                   "0..2 the query's vertices 0, a1, a2 as rays (o, d) against the scene triangle (p0, e1, e2)",
                   "3..5 the scene triangle's vertices p0, p1, p2 as rays (o, -d) against the query triangle (0, a1, a2)",
                   "Moller-Trumbore without the renderer's 1e-6", "pv = cross(d, f2), det = dot(f1, pv), tv = o - w0, qv = cross(tv, f1)",
                   "nu = dot(tv, pv) sg, nv = dot(d, qv) sg, ntau = dot(f2, qv) sg",
                   "det != 0 && nu >= 0 && nv >= 0 && nu + nv <= ad && ntau >= 0", "tau = fabsf(ntau) / ad",
                   "query edge i of ((0, a1), (a1, g), (a2, -a2)) against scene edge j of ((p0, e1), (p1, h), (p2, -e2))", "candidate 6 + 3 i + j",
                   "a + ea s + d tau = b + eb w by Cramer's rule on the columns (ea, d, -eb)",
                   "nb = -eb, c = cross(d, nb), det = dot(ea, c), r = b - a",
                   "ns = dot(r, c) sg, ntau = dot(ea, cross(r, nb)) sg, nw = dot(ea, cross(d, r)) sg",
                   "det != 0 && ns >= 0 && ns <= ad && nw >= 0 && nw <= ad && ntau >= 0",
                   "t = +infinity, candidate = 15", "replaces them iff it passes and its tau < t", "the first wins a tie",
                   "Touching counts: every comparison is closed", "the pair's t = 0 and feature = candidate | 16 (31 if no candidate passed)",
                   "cannot see a pair that already interpenetrates", "conservatism on zero-area triangles is inherited",
                   "best = tmax, prim = -1", "t < best || (t == best && k < prim)", "the answer does not depend on the tree", "tmax <= 0 finds nothing",
                   "ext_lo = qmin - q0 and ext_hi = qmax - q0", "inv_d = 1 / d per component",
                   "t0 = ((bmin - ext_hi) - q0) inv_d, t1 = ((bmax - ext_lo) - q0) inv_d",
                   "visited iff enter <= exit && exit >= 0 && enter <= best", "dropped unless its enter <= best still holds",
                   "the farther one first (enter1 > enter2 -> child 1)", "the limit is 64 levels", "d = 0 degenerates to the static overlap test",
                   "DRT_TRICAST_FIRST is the search above", "DRT_TRICAST_ANY ends a cast at the first pair with t < best in traversal order",
                   "not the first contact", "drt_tri_hit {point, t, normal, prim, u, v, feature, pad}, 48 bytes",
                   "recomputed once, after the traversal, from the winning (prim, candidate)",
                   "u = fabsf(nu) / ad, v = fabsf(nv) / ad, c = (p0 + e1 u) + e2 v, normal = cross(e1, e2)",
                   "(u, v) = (0, 0), (1, 0), (0, 1), normal = nq", "w = fabsf(nw) / ad, c = b + eb w",
                   "(w, 0) on scene edge 0, (1 - w, w) on edge 1, (0, 1 - w) on edge 2", "normal = cross(ea, eb)",
                   "point = q0 + c is the contact point on the scene triangle", "if dot(normal, d) > 0 every component is negated",
                   "point, normal, u and v are zeros, t = 0", "all zero with t = tmax, the motion's own word, prim = -1 and feature = -1",
                   "a refitted device copy is the one queried", "DRT_ERR_UNSUPPORTED beyond 64 levels",
                   "DRT_ERR_INVALID while an asynchronous batch is pending", "legal on a sharded renderer",
                   "counters, kernel info and kernel span are not touched"):
        assert phrase in flat, phrase
    limits = flat[flat.index("What this is not:"):]
    for phrase in ("coplanar and slides in its common plane is seen only by the start overlap", "every det is 0 there",
                   "drt_renderer_intersect_triangles has no coplanar records either", "no tolerance and no thickness", "contact exactly on a seam",
                   "in rare cases by none", "no rotation", "no penetration depth", "alpha cut-outs are ignored", "one answer per cast"):
        assert phrase in limits, phrase
    before = re.sub(r"\s*\n \*\s*", " ", text[:text.index("#define DRT_ABI_VERSION 2")])
    assert "the triangle-cast entry point (drt_renderer_triangle_cast)" in before
    # the working range paragraph names the query and the measured range, which tests/test_tri_cast_ref.py asserts
    from tests.test_tri_cast_ref import SCALE_RANGE
    rng = re.sub(r"\s*\n \*\s*", " ", text[text.index("working range of the mesh queries"):text.index("intersection curves (new")])
    assert "drt_renderer_triangle_cast:" in rng and "unchanged for 2^%d to 2^%d" % SCALE_RANGE in rng[rng.index("drt_renderer_triangle_cast:"):rng.index("drt_renderer_sphere_cast:")]
    assert "THIRD power" in rng[rng.index("drt_renderer_triangle_cast:"):rng.index("drt_renderer_sphere_cast:")]


def test_cpp_wrapper_compiles_and_links(tmp_path):
    src = tmp_path / "tri_cast_calls.cpp"
    src.write_text(r"""
#include <cstdio>
#include "DustRayTracer.hpp"
// the statements only -- main() runs none of them without arguments
int main(int argc, char **) {
    if (argc < 2) { std::printf("%zu %zu %zu %d\n", sizeof(drt_tri_hit), alignof(drt_tri_hit), sizeof(drt_motion), DRT_ABI_VERSION); return 0; }
    Scene scene;
    Renderer r(0);
    const drt_tri *tris = nullptr;
    const drt_motion *motions = nullptr;
    drt_tri_hit *out = nullptr;
    r.TriangleCast(scene, tris, motions, out, 0u);
    r.TriangleCast(scene, tris, motions, out, 0u, DRT_TRICAST_ANY, nullptr);
    return 0;
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    exe = tmp_path / "tri_cast_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib_dir, "-ldrt_hip",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["48", "4", "16", "2"]
