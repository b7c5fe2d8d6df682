"""The box-overlap entry point of include/drt.h without a GPU: exported, bound, laid out as declared, the argument checks that come
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
    assert hasattr(lib, "drt_renderer_overlap_boxes")
    fn = drt._lib.drt_renderer_overlap_boxes
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 10
    assert fn.argtypes[5] is ctypes.c_uint32 and fn.argtypes[7] is ctypes.c_uint32 and fn.argtypes[8] is ctypes.c_int32   # prims_capacity, n, mode
    assert all(fn.argtypes[i] is ctypes.c_void_p for i in (0, 1, 2, 3, 4, 6, 9))
    for method in ("overlapBoxes", "overlapsAny", "voxelize"):
        assert callable(getattr(drt.Renderer, method)), method
    assert drt.BoxList._fields == ("splits", "prim") and drt.BoxTable._fields == ("prim", "count")
    assert (drt.OVERLAP_LIST, drt.OVERLAP_ANY) == (0, 1)
    assert drt._lib.drt_abi_version() == 2


def test_record_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "drt.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu\n", sizeof(drt_box), offsetof(drt_box, center), offsetof(drt_box, half), offsetof(drt_box, axis), offsetof(drt_box, pad));
    printf("%zu %zu\n", sizeof(((drt_box *)0)->axis), sizeof(((drt_box *)0)->axis[0]));
    printf("%d %d %d\n", DRT_OVERLAP_LIST, DRT_OVERLAP_ANY, DRT_ABI_VERSION);
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["64", "0", "12", "24", "60", "36", "12", "0", "1", "2"]


def test_null_handles_a_bad_mode_and_any_with_prims_are_invalid_without_a_gpu():
    L = drt._lib
    sc = drt.Scene()
    assert L.drt_renderer_overlap_boxes(None, sc._h, None, None, None, 0, None, 4, 0, None) == drt.ERR_INVALID
    assert b"null" in L.drt_last_error()
    assert L.drt_renderer_overlap_boxes(None, None, None, None, None, 0, None, 0, 1, None) == drt.ERR_INVALID   # the handles are checked before n == 0
    assert L.drt_renderer_overlap_boxes(None, sc._h, None, None, None, 0, None, 4, 7, None) == drt.ERR_INVALID  # ... and before the mode
    assert b"null" in L.drt_last_error()
    # the mode is checked first after the handles, before n == 0 and before the renderer is looked at: a block of zeros stands in for it
    stand_in = ctypes.create_string_buffer(1 << 16)
    h = ctypes.addressof(stand_in)
    for mode in (2, -1, 7):
        for n in (0, 4):
            assert L.drt_renderer_overlap_boxes(h, sc._h, None, None, None, 0, None, n, mode, None) == drt.ERR_INVALID
            assert b"mode" in L.drt_last_error()
    for mode in (0, 1):
        assert L.drt_renderer_overlap_boxes(h, sc._h, None, None, None, 0, None, 0, mode, None) == drt.OK        # n == 0: nothing to do
        assert L.drt_renderer_overlap_boxes(h, sc._h, None, None, None, 0, None, 4, mode, None) == drt.ERR_INVALID
        assert b"null box" in L.drt_last_error()
    # the pointer combinations, checked before anything is dereferenced: stand-in addresses, 16-byte aligned
    boxes = ctypes.create_string_buffer(64 * 4 + 16)
    B = (ctypes.addressof(boxes) + 15) & ~15
    words = ctypes.create_string_buffer(64)
    W = (ctypes.addressof(words) + 15) & ~15
    # mode ANY takes no prims and no capacity, and needs counts; offsets is not read, so null is fine (the next check, on the
    # stand-in renderer, is never reached: each of these fails before it)
    for what, args in (("any with prims", (B, None, W, 4, W, 4, 1)), ("any with a capacity", (B, None, None, 4, W, 4, 1)),
                       ("any without counts", (B, None, None, 0, None, 4, 1)), ("any with prims, offsets given", (B, W, W, 4, W, 4, 1))):
        assert L.drt_renderer_overlap_boxes(h, sc._h, *args, None) == drt.ERR_INVALID, what
        assert b"mode any" in L.drt_last_error(), what
    for what, args, text in (("list without offsets", (B, None, W, 4, W, 4, 0), b"null box or offset"),
                             ("both outputs null", (B, W, None, 0, None, 4, 0), b"both null"),
                             ("null prims with a capacity", (B, W, None, 4, W, 4, 0), b"if and only if"),
                             ("prims without a capacity", (B, W, W, 0, W, 4, 0), b"if and only if"),
                             ("misaligned boxes", (B + 4, W, W, 4, W, 4, 0), b"aligned"), ("misaligned prims", (B, W, W + 2, 4, W, 4, 0), b"aligned"),
                             ("misaligned offsets", (B, W + 1, W, 4, W, 4, 0), b"aligned"), ("misaligned counts", (B, W, W, 4, W + 3, 4, 0), b"aligned"),
                             ("misaligned counts, any", (B, None, None, 0, W + 2, 4, 1), b"aligned")):
        assert L.drt_renderer_overlap_boxes(h, sc._h, *args, None) == drt.ERR_INVALID, what
        assert text in L.drt_last_error(), what


def test_bad_arguments_are_refused_before_any_device_work():
    r = drt.Renderer.__new__(drt.Renderer)                                     # (no device: only the argument check runs)
    r._device = 0
    sc = drt.Scene()
    c = np.zeros((3, 3), np.float32)
    for k in (0, -1, 2.5, True):
        with pytest.raises(drt.DrtError) as e:
            r.overlapBoxes(sc, c, c, k=k)
        assert e.value.code == drt.ERR_INVALID and "k" in str(e.value)
    for res in (0, (4, 4), (2, 0, 2)):
        with pytest.raises(drt.DrtError) as e:
            r.voxelize(sc, res, lo=(0, 0, 0), hi=(1, 1, 1))
        assert e.value.code == drt.ERR_INVALID and "resolution" in str(e.value)


def test_the_header_states_the_rule_and_its_limits():
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    sec = text[text.index("box overlap queries (new"):text.index("typedef struct drt_box ")]
    flat = re.sub(r"\s*\n \*\s*", " ", sec)
    for phrase in ("64 bytes, 16-byte aligned", "center[3], half[3], axis[3][3] and one pad word that is ignored", "used as given: not normalised, not orthogonalised",
                   "with identity axes every product below is exact", "needs no code path of its own",
                   "fp32 with one rounding per operation, in the order written", "dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z",
                   "cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x)", "fminf / fmaxf drop a NaN operand", "Alpha cut-outs are ignored",
                   "computed once per query", "ext[j] = (|axis[0][j]| half[0] + |axis[1][j]| half[1]) + |axis[2][j]| half[2]",
                   "qmin = center - ext, qmax = center + ext", "qmin[j] <= bmax[j] && bmin[j] <= qmax[j]", "The comparisons are closed",
                   "no arithmetic is done on the node", "a NaN query lists nothing", "0 * inf",
                   "the root is tested against the scene's root box", "pushes each child that passes, child 2 first", "tests its triangles in order",
                   "The same 64-level stack bound applies", "does not depend on the traversal order", "a triangle whose leaf the cull rejects is not listed",
                   "v0 + e1 can round one ulp outside a node box built from the real v1", "Akenine-Moller (2001)", "on the stored (v0, e1, e2)",
                   "a = v0 - center", "p0[k] = dot(axis[k], a), f1[k] = dot(axis[k], e1), f2[k] = dot(axis[k], e2)", "p1 = p0 + f1, p2 = p0 + f2, g = f2 - f1",
                   "min3(x, y, z) = fminf(fminf(x, y), z)", "min3(p0[k], p1[k], p2[k]) <= half[k] && max3(p0[k], p1[k], p2[k]) >= -half[k]",
                   "n = cross(f1, f2), d = dot(n, p0), r = (|n.x| half[0] + |n.y| half[1]) + |n.z| half[2]; ok iff fabsf(d) <= r",
                   "L = cross(unit_k, E) for E in (f1, g, f2)", "all three projections, not the two-value shortcut", "left operand first",
                   "L = (0, -E.z, E.y): s_i = (-E.z) p_i.y + E.y p_i.z, r = half[1] |E.z| + half[2] |E.y|",
                   "L = (E.z, 0, -E.x): s_i = E.z p_i.x + (-E.x) p_i.z, r = half[0] |E.z| + half[2] |E.x|",
                   "L = (-E.y, E.x, 0): s_i = (-E.y) p_i.x + E.x p_i.y, r = half[0] |E.y| + half[1] |E.x|",
                   "ok iff min3(s0, s1, s2) <= r && max3(s0, s1, s2) >= -r", "listed iff all 13 are ok", "Touching counts",
                   "half = 0 is a point or a flat box, and it works", "passes its zero cross axes with 0 <= 0", "Only the predicate leaves the kernel",
                   "the 13 comparisons are made on the same rounded values",
                   "segments are exactly drt_renderer_list_hits'", "offsets holds n + 1 uint32 values", "prims[offsets[i] .. offsets[i+1])",
                   "cap_i = offsets[i+1] > offsets[i] ? offsets[i+1] - offsets[i] : 0", "offsets[i] + cap_i <= prims_capacity",
                   "offsets[i] >= prims_capacity gives 0", "and nothing else in prims", "int32 triangle indices in ascending order", "unused slots hold -1",
                   "counts[i] is the total number listed", "the first K of a longer list are the list at capacity K",
                   "prims may be NULL iff prims_capacity == 0", "a pure count", "both prims and counts NULL is DRT_ERR_INVALID",
                   "the traversal ends at the first listed triangle, and counts[i] is 0 or 1", "prims must be NULL and prims_capacity 0",
                   "offsets is not read", "counts NULL is DRT_ERR_INVALID", "An empty scene lists nothing"):
        assert phrase in flat, phrase
    limits = flat[flat.index("What this is not:"):]
    for phrase in ("box-versus-box", "clipped polygons", "a large-list structure", "one-record-per-step insert of drt_renderer_list_hits",
                   "drt_renderer_nearest_list's, checked in its order", "handles are checked before n == 0",
                   "a mode outside {0, 1} is DRT_ERR_INVALID (checked first after the handles)", "n == 0 is a no-op", "n < 2^31",
                   "boxes 16-byte aligned, offsets, prims and counts 4-byte aligned", "the call only enqueues", "refitted device copy",
                   "sharded renderer", "DRT_ERR_UNSUPPORTED beyond 64 levels", "DRT_ERR_INVALID while an asynchronous batch is pending",
                   "counters, kernel info and kernel span are not touched"):
        assert phrase in limits, phrase
    assert "drt_renderer_overlap_boxes" in text[:text.index("#define DRT_ABI_VERSION 2")]
    assert "#define DRT_OVERLAP_LIST 0" in text and "#define DRT_OVERLAP_ANY  1" in text


def test_cpp_wrapper_compiles_and_links(tmp_path):
    src = tmp_path / "overlap_calls.cpp"
    src.write_text(r"""
#include <cstdio>
#include "DustRayTracer.hpp"
// the statements only -- main() runs none of them without arguments
int main(int argc, char **) {
    if (argc < 2) { std::printf("%zu %d\n", sizeof(drt_box), DRT_ABI_VERSION); return 0; }
    Scene scene;
    Renderer r(0);
    const drt_box *boxes = nullptr;
    const uint32_t *offsets = nullptr;
    int32_t *prims = nullptr;
    uint32_t *counts = nullptr;
    r.OverlapBoxes(scene, boxes, offsets, prims, 0u, counts, 0u, DRT_OVERLAP_LIST);
    r.OverlapBoxes(scene, boxes, nullptr, nullptr, 0u, counts, 0u, DRT_OVERLAP_ANY, nullptr);
    return 0;
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    exe = tmp_path / "overlap_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib_dir, "-ldrt_hip",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["64", "2"]
