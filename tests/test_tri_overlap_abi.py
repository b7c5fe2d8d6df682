"""The triangle-overlap entry point of include/drt.h without a GPU: exported, bound, laid out as declared, the argument checks that come
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
    assert hasattr(lib, "drt_renderer_overlap_triangles")
    fn = drt._lib.drt_renderer_overlap_triangles
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 10
    assert fn.argtypes[5] is ctypes.c_uint32 and fn.argtypes[7] is ctypes.c_uint32 and fn.argtypes[8] is ctypes.c_int32   # prims_capacity, n, mode
    assert all(fn.argtypes[i] is ctypes.c_void_p for i in (0, 1, 2, 3, 4, 6, 9))
    assert fn.argtypes == drt._lib.drt_renderer_overlap_boxes.argtypes
    for method in ("overlapTriangles", "intersectsAny", "selfIntersections"):
        assert callable(getattr(drt.Renderer, method)), method
    assert drt.TriList._fields == ("splits", "prim") and drt.TriTable._fields == ("prim", "count")
    assert "not reported" in drt.Renderer.selfIntersections.__doc__                  # neighbours that also cut each other
    assert drt._lib.drt_abi_version() == 2


def test_record_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "drt.h"
int main(void) {
    printf("%zu %zu %zu\n", sizeof(drt_tri), offsetof(drt_tri, v), offsetof(drt_tri, pad));
    printf("%zu %zu %zu\n", sizeof(((drt_tri *)0)->v), sizeof(((drt_tri *)0)->v[0]), sizeof(((drt_tri *)0)->pad));
    printf("%d %d %d\n", DRT_OVERLAP_LIST, DRT_OVERLAP_ANY, DRT_ABI_VERSION);
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["48", "0", "36", "36", "12", "12", "0", "1", "2"]


def test_the_argument_checks_are_the_box_query_s_in_its_order():
    L = drt._lib
    sc = drt.Scene()
    fn = L.drt_renderer_overlap_triangles
    assert fn(None, sc._h, None, None, None, 0, None, 4, 0, None) == drt.ERR_INVALID
    assert b"null" in L.drt_last_error()
    assert fn(None, None, None, None, None, 0, None, 0, 1, None) == drt.ERR_INVALID      # the handles are checked before n == 0
    assert fn(None, sc._h, None, None, None, 0, None, 4, 7, None) == drt.ERR_INVALID     # ... and before the mode
    assert b"null" in L.drt_last_error()
    # the mode is checked first after the handles, before n == 0 and before the renderer is looked at: a block of zeros stands in for it
    stand_in = ctypes.create_string_buffer(1 << 16)
    h = ctypes.addressof(stand_in)
    for mode in (2, -1, 7):
        for n in (0, 4):
            assert fn(h, sc._h, None, None, None, 0, None, n, mode, None) == drt.ERR_INVALID
            assert b"mode" in L.drt_last_error()
    for mode in (0, 1):
        assert fn(h, sc._h, None, None, None, 0, None, 0, mode, None) == drt.OK            # n == 0: nothing to do
        assert fn(h, sc._h, None, None, None, 0, None, 4, mode, None) == drt.ERR_INVALID
        assert b"null triangle" in L.drt_last_error()
    # the pointer combinations, checked before anything is dereferenced: stand-in addresses, 16-byte aligned
    tris = ctypes.create_string_buffer(48 * 4 + 16)
    B = (ctypes.addressof(tris) + 15) & ~15
    words = ctypes.create_string_buffer(64)
    W = (ctypes.addressof(words) + 15) & ~15
    for what, args in (("any with prims", (B, None, W, 4, W, 4, 1)), ("any with a capacity", (B, None, None, 4, W, 4, 1)),
                       ("any without counts", (B, None, None, 0, None, 4, 1)), ("any with prims, offsets given", (B, W, W, 4, W, 4, 1))):
        assert fn(h, sc._h, *args, None) == drt.ERR_INVALID, what
        assert b"mode any" in L.drt_last_error(), what
    for what, args, text in (("list without offsets", (B, None, W, 4, W, 4, 0), b"null triangle or offset"),
                             ("both outputs null", (B, W, None, 0, None, 4, 0), b"both null"),
                             ("null prims with a capacity", (B, W, None, 4, W, 4, 0), b"if and only if"),
                             ("prims without a capacity", (B, W, W, 0, W, 4, 0), b"if and only if"),
                             ("misaligned tris", (B + 4, W, W, 4, W, 4, 0), b"aligned"), ("misaligned prims", (B, W, W + 2, 4, W, 4, 0), b"aligned"),
                             ("misaligned offsets", (B, W + 1, W, 4, W, 4, 0), b"aligned"), ("misaligned counts", (B, W, W, 4, W + 3, 4, 0), b"aligned"),
                             ("misaligned counts, any", (B, None, None, 0, W + 2, 4, 1), b"aligned")):
        assert fn(h, sc._h, *args, None) == drt.ERR_INVALID, what
        assert text in L.drt_last_error(), what
    # the same calls give the box query the same codes: one order of checks
    for args in ((B, None, W, 4, W, 4, 1), (B, W, None, 0, None, 4, 0), (B + 4, W, W, 4, W, 4, 0), (None, None, None, 0, None, 4, 5)):
        assert fn(h, sc._h, *args, None) == L.drt_renderer_overlap_boxes(h, sc._h, *args, None) == drt.ERR_INVALID


def test_bad_arguments_are_refused_before_any_device_work():
    r = drt.Renderer.__new__(drt.Renderer)                                     # (no device: only the argument check runs)
    r._device = 0
    sc = drt.Scene()
    t = np.zeros((3, 3, 3), np.float32)
    for k in (0, -1, 2.5, True):
        with pytest.raises(drt.DrtError) as e:
            r.overlapTriangles(sc, t, k=k)
        assert e.value.code == drt.ERR_INVALID and "k" in str(e.value)


def test_the_header_states_the_rule_and_its_limits():
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    sec = text[text.index("triangle overlap queries (new"):text.index("typedef struct drt_tri ")]
    flat = re.sub(r"\s*\n \*\s*", " ", sec)
    for phrase in ("48 bytes, 16-byte aligned", "three pad words that are ignored", "A mesh is a batch of queries",
                   "drt_renderer_overlap_boxes', word for word", "DRT_OVERLAP_LIST and DRT_OVERLAP_ANY", "the -1 fill", "counts[i] as the total",
                   "the NULL rules and the argument checks in that order", "the error codes and the stream ordering",
                   "a refitted device copy is the one queried", "the 64-level bound", "counters, kernel info and kernel span are not touched",
                   "fp32 with one rounding per operation, in the order written", "min3(x, y, z) = fminf(fminf(x, y), z)",
                   "valid iff all nine coordinates satisfy fabsf(x) <= FLT_MAX", "pushes nothing and lists nothing",
                   "fminf would otherwise drop a NaN vertex from the bounds",
                   "qmin[j] = min3(q0[j], q1[j], q2[j])", "They are exact", "the box query's, unchanged", "child 2 first",
                   "v0 + e1 can round one ulp outside a node box", "a triangle whose leaf the cull rejects is not listed",
                   "relative to q0", "a1 = q1 - q0, a2 = q2 - q0, g = a2 - a1", "h = e2 - e1", "p0 = v0 - q0, p1 = p0 + e1, p2 = p0 + e2",
                   "nq = cross(a1, a2), nt = cross(e1, e2)", "Seventeen axes L, in this order", "1. nq", "2. nt",
                   "3. cross(A, E) for A in (a1, g, a2) (outer) and E in (e1, h, e2) (inner)", "4. cross(nq, A) for A in (a1, g, a2)",
                   "5. cross(nt, E) for E in (e1, h, e2)", "sq = (0, dot(L, a1), dot(L, a2))", "st = (dot(L, p0), dot(L, p1), dot(L, p2))",
                   "min3(st) <= max3(sq) && min3(sq) <= max3(st)", "listed iff all seventeen are ok", "Touching counts",
                   "a shared edge is a touch", "lists itself", "may evaluate the axes in any order and stop at the first failure",
                   "the exact intersection test of the two closed sets", "the standard 11 axes", "the six in-plane edge normals",
                   "the nine cross products vanish and pass with 0 <= 0", "it is conservative: it never misses",
                   "may list a near miss in the triangle's own plane", "the fourth power of the coordinate differences",
                   "a comparison on a NaN fails and the pair is not listed"):
        assert phrase in flat, phrase
    limits = flat[flat.index("What this is not:"):]
    for phrase in ("the intersection segment is not returned", "no clipping, no contour", "no pair exclusion at this level",
                   "are listed, because they touch", "not a large-list structure", "one-record-per-step insert of drt_renderer_list_hits",
                   "tris is 16-byte aligned"):
        assert phrase in limits, phrase
    assert "drt_renderer_overlap_triangles" in text[:text.index("#define DRT_ABI_VERSION 2")]
    # beside the box overlap block
    assert text.index("drt_renderer_overlap_boxes(drt_renderer") < text.index("triangle overlap queries (new") < text.index("sphere casts (new")


def test_cpp_wrapper_compiles_and_links(tmp_path):
    src = tmp_path / "tri_overlap_calls.cpp"
    src.write_text(r"""
#include <cstdio>
#include "DustRayTracer.hpp"
// the statements only -- main() runs none of them without arguments
int main(int argc, char **) {
    if (argc < 2) { std::printf("%zu %zu %d\n", sizeof(drt_tri), alignof(drt_tri), DRT_ABI_VERSION); return 0; }
    Scene scene;
    Renderer r(0);
    const drt_tri *tris = nullptr;
    const uint32_t *offsets = nullptr;
    int32_t *prims = nullptr;
    uint32_t *counts = nullptr;
    r.OverlapTriangles(scene, tris, offsets, prims, 0u, counts, 0u, DRT_OVERLAP_LIST);
    r.OverlapTriangles(scene, tris, nullptr, nullptr, 0u, counts, 0u, DRT_OVERLAP_ANY, nullptr);
    return 0;
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    exe = tmp_path / "tri_overlap_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib_dir, "-ldrt_hip",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["48", "4", "2"]
