"""The plane-section entry point of include/drt.h without a GPU: exported, bound, laid out as declared, the argument checks that come
before any device work, the header states the rule and its limits, and the C++ wrapper compiles and links against it."""
import ctypes
import os
import re
import subprocess

import pytest

from tests.scenes import ROOT

drt = pytest.importorskip("dustraytracer_amd")


def test_the_symbol_is_exported_and_bound():
    lib = ctypes.CDLL(drt.LIB_PATH)
    assert hasattr(lib, "drt_renderer_plane_sections")
    fn = drt._lib.drt_renderer_plane_sections
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 10
    assert fn.argtypes[5] is ctypes.c_uint32 and fn.argtypes[7] is ctypes.c_uint32 and fn.argtypes[8] is ctypes.c_int32   # out_capacity, n, mode
    assert all(fn.argtypes[i] is ctypes.c_void_p for i in (0, 1, 2, 3, 4, 6, 9))
    assert fn.argtypes == drt._lib.drt_renderer_overlap_boxes.argtypes
    for method in ("planeSections", "cutsAny", "slices", "sectionAreas"):
        assert callable(getattr(drt.Renderer, method)), method
    assert drt.SectionList._fields == ("splits", "p", "q", "prim", "code")
    assert (drt.SECTION_LIST, drt.SECTION_ANY) == (0, 1)
    assert "weld with a tolerance" in drt.Renderer.planeSections.__doc__
    assert drt._lib.drt_abi_version() == 2


def test_record_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "drt.h"
int main(void) {
    printf("%zu %zu %zu\n", sizeof(drt_plane), offsetof(drt_plane, n), offsetof(drt_plane, d));
    printf("%zu %zu %zu %zu %zu\n", sizeof(drt_section), offsetof(drt_section, p), offsetof(drt_section, prim), offsetof(drt_section, q),
           offsetof(drt_section, code));
    printf("%d %d %d\n", DRT_SECTION_LIST, DRT_SECTION_ANY, DRT_ABI_VERSION);
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["16", "0", "12", "32", "0", "12", "16", "28", "0", "1", "2"]


def test_the_argument_checks_are_the_box_query_s_in_its_order():
    L = drt._lib
    sc = drt.Scene()
    fn = L.drt_renderer_plane_sections
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
        assert b"null plane" in L.drt_last_error()
    # the pointer combinations, checked before anything is dereferenced: stand-in addresses, 16-byte aligned
    planes = ctypes.create_string_buffer(16 * 4 + 16)
    B = (ctypes.addressof(planes) + 15) & ~15
    words = ctypes.create_string_buffer(64)
    W = (ctypes.addressof(words) + 15) & ~15
    for what, args in (("any with out", (B, None, W, 4, W, 4, 1)), ("any with a capacity", (B, None, None, 4, W, 4, 1)),
                       ("any without counts", (B, None, None, 0, None, 4, 1)), ("any with out, offsets given", (B, W, W, 4, W, 4, 1))):
        assert fn(h, sc._h, *args, None) == drt.ERR_INVALID, what
        assert b"mode any" in L.drt_last_error(), what
    for what, args, text in (("list without offsets", (B, None, W, 4, W, 4, 0), b"null plane or offset"),
                             ("both outputs null", (B, W, None, 0, None, 4, 0), b"both null"),
                             ("null out with a capacity", (B, W, None, 4, W, 4, 0), b"if and only if"),
                             ("out without a capacity", (B, W, W, 0, W, 4, 0), b"if and only if"),
                             ("misaligned planes", (B + 4, W, W, 4, W, 4, 0), b"aligned"), ("misaligned out", (B, W, W + 4, 4, W, 4, 0), b"aligned"),
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
    for count in (0, -1, 2.5, True):
        with pytest.raises(drt.DrtError) as e:
            r.slices(sc, count)
        assert e.value.code == drt.ERR_INVALID and "count" in str(e.value)
    with pytest.raises(drt.DrtError) as e:
        r.slices(sc, 4, axis=3)
    assert e.value.code == drt.ERR_INVALID and "axis" in str(e.value)


def test_the_header_states_the_rule_and_its_limits():
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    sec = text[text.index("plane sections (new"):text.index("typedef struct drt_plane ")]
    flat = re.sub(r"\s*\n \*\s*", " ", sec)
    for phrase in ("16 bytes, 16-byte aligned", "It is the set dot(n, x) = d", "n is used as given and is not normalised",
                   "drt_renderer_overlap_boxes', word for word", "the NULL rules and the argument checks in that order",
                   "the error codes and the stream ordering", "a refitted device copy is the one queried", "the 64-level bound",
                   "counters, kernel info and kernel span are not touched", "fp32 with one rounding per operation, in the order written",
                   "dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z", "valid iff all four words satisfy fabsf(x) <= FLT_MAX",
                   "pushes nothing and lists nothing", "n = 0 is valid and cuts nothing", "s(x) = dot(n, x) - d",
                   "above iff s >= 0 (closed), otherwise below", "cmin[j] = n[j] >= 0 ? bmin[j] : bmax[j]", "cmax[j] is the other one",
                   "passes iff s(cmin) < 0 && s(cmax) >= 0", "The root is tested against the scene's root box", "child 1 before child 2",
                   "rounding is monotone", "s(cmin) <= s(v) <= s(cmax) holds in fp32",
                   "the cull never drops a cut triangle whose vertices lie in the box", "v0 + e1 can round one ulp outside a node box",
                   "a triangle whose leaf the cull rejects is not listed", "v1 = v0 + e1, v2 = v0 + e2",
                   "cut iff its three vertices are not all in the same class", "A triangle lying in the plane is all above and is not cut",
                   "exactly one vertex k is alone in its class: the apex", "lo be the below one of the two and hi the above one",
                   "t = s_lo / (s_lo - s_hi)", "lo + (hi - lo) * t per component", "depend on that edge's two vertices only",
                   "P = cut(k, k+1) and Q = cut(k, k+2), indices mod 3", "Apex above: the segment is P -> Q", "Apex below: it is Q -> P",
                   "dot(q - p, cross(n, fn)) >= 0 with fn = cross(e1, e2)", "counter-clockwise seen from the side n points to",
                   "0.5 * sum dot(n / |n|, cross(p, q)) is the positive section area", "code = k + 4 * (apex above)",
                   "A vertex exactly on the plane is above", "gives a zero-length segment, and it is listed",
                   "32 bytes: p[3], prim, q[3], code", "The miss record is all zeros with prim = -1", "ascending triangle index",
                   "does not depend on the traversal order", "with 32-byte records in place of int32", "The first cap_i records of the list are stored",
                   "the rest of the cap_i slots hold the miss record", "counts[i] is the total", "out is NULL iff out_capacity == 0: a pure count",
                   "the work ends at the first cut triangle found, and counts[i] is 0 or 1",
                   "may finish the group of leaves it is testing before it stops; counts[i] is the same", "returns DRT_ERR_UNSUPPORTED for a tree where it is false"):
        assert phrase in flat, phrase
    limits = flat[flat.index("What this is not:"):]
    for phrase in ("no chaining into loops", "agree only as far as their stored vertices do", "a caller welds with a tolerance",
                   "no caps or filled polygons", "alpha cut-outs are ignored", "not built for millions of planes with near-empty lists",
                   "it works there, one wave each", "planes and out are 16-byte aligned"):
        assert phrase in limits, phrase
    assert "drt_renderer_plane_sections" in text[:text.index("#define DRT_ABI_VERSION 2")]
    # beside the triangle overlap block
    assert text.index("drt_renderer_overlap_triangles(drt_renderer") < text.index("plane sections (new") < text.index("sphere casts (new")


def test_cpp_wrapper_compiles_and_links(tmp_path):
    src = tmp_path / "section_calls.cpp"
    src.write_text(r"""
#include <cstdio>
#include "DustRayTracer.hpp"
// the statements only -- main() runs none of them without arguments
int main(int argc, char **) {
    if (argc < 2) { std::printf("%zu %zu %zu %d\n", sizeof(drt_plane), sizeof(drt_section), alignof(drt_section), DRT_ABI_VERSION); return 0; }
    Scene scene;
    Renderer r(0);
    const drt_plane *planes = nullptr;
    const uint32_t *offsets = nullptr;
    drt_section *out = nullptr;
    uint32_t *counts = nullptr;
    r.PlaneSections(scene, planes, offsets, out, 0u, counts, 0u, DRT_SECTION_LIST);
    r.PlaneSections(scene, planes, nullptr, nullptr, 0u, counts, 0u, DRT_SECTION_ANY, nullptr);
    return 0;
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    exe = tmp_path / "section_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib_dir, "-ldrt_hip",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["16", "32", "4", "2"]

