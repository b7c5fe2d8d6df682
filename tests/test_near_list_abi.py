"""The nearest-list entry point of include/drt.h without a GPU: exported, bound, laid out as declared, the argument checks that come
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
    assert hasattr(lib, "drt_renderer_nearest_list")
    fn = drt._lib.drt_renderer_nearest_list
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 11
    assert fn.argtypes[6] is ctypes.c_uint32 and fn.argtypes[8] is ctypes.c_uint32 and fn.argtypes[9] is ctypes.c_int32   # near_capacity, n, mode
    assert all(fn.argtypes[i] is ctypes.c_void_p for i in (0, 1, 2, 3, 4, 5, 7, 10))
    for method in ("kNearest", "withinRadius"):
        assert callable(getattr(drt.Renderer, method)), method
    assert drt.KNearest._fields == ("d2", "prim", "u", "v", "point", "side", "count")
    assert drt.NearList._fields == ("splits", "d2", "prim", "u", "v", "point", "side")
    assert (drt.NEAR_GATHER, drt.NEAR_K) == (0, 1)
    assert drt._lib.drt_abi_version() == 2


def test_record_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "drt.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu\n", sizeof(drt_near), offsetof(drt_near, d2), offsetof(drt_near, prim), offsetof(drt_near, u), offsetof(drt_near, v));
    printf("%zu %zu %zu\n", sizeof(drt_near_surf), offsetof(drt_near_surf, point), offsetof(drt_near_surf, side));
    printf("%d %d %d\n", DRT_NEAR_GATHER, DRT_NEAR_K, DRT_ABI_VERSION);
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["16", "0", "4", "8", "12", "16", "0", "12", "0", "1", "2"]


def test_null_handles_and_a_bad_mode_are_invalid_without_a_gpu():
    L = drt._lib
    sc = drt.Scene()
    assert L.drt_renderer_nearest_list(None, sc._h, None, None, None, None, 0, None, 4, 0, None) == drt.ERR_INVALID
    assert b"null" in L.drt_last_error()
    assert L.drt_renderer_nearest_list(None, None, None, None, None, None, 0, None, 0, 1, None) == drt.ERR_INVALID   # the handles are checked before n == 0
    assert L.drt_renderer_nearest_list(None, sc._h, None, None, None, None, 0, None, 4, 7, None) == drt.ERR_INVALID  # ... and before the mode
    assert b"null" in L.drt_last_error()
    # the mode is checked first after the handles, before n == 0 and before the renderer is looked at: a block of zeros stands in for it
    stand_in = ctypes.create_string_buffer(1 << 16)
    h = ctypes.addressof(stand_in)
    for mode in (2, -1, 7):
        for n in (0, 4):
            assert L.drt_renderer_nearest_list(h, sc._h, None, None, None, None, 0, None, n, mode, None) == drt.ERR_INVALID
            assert b"mode" in L.drt_last_error()
    for mode in (0, 1):
        assert L.drt_renderer_nearest_list(h, sc._h, None, None, None, None, 0, None, 0, mode, None) == drt.OK         # n == 0: nothing to do
        assert L.drt_renderer_nearest_list(h, sc._h, None, None, None, None, 0, None, 4, mode, None) == drt.ERR_INVALID
        assert b"null point" in L.drt_last_error()


def test_a_bad_k_is_refused_before_any_device_work():
    r = drt.Renderer.__new__(drt.Renderer)                                     # (no device: only the argument check runs)
    r._device = 0
    sc = drt.Scene()
    pts = np.zeros((3, 3), np.float32)
    for k in (0, -1, 2.5, None, True):
        with pytest.raises(drt.DrtError) as e:
            r.kNearest(sc, pts, k=k)
        assert e.value.code == drt.ERR_INVALID and "k" in str(e.value)
    # N * k >= 2^31 records: refused by the shape alone (a broadcast view: no memory behind it)
    many = np.broadcast_to(np.zeros((1, 3), np.float32), (2 ** 20, 3))
    with pytest.raises(drt.DrtError) as e:
        r.kNearest(sc, many, k=2 ** 11)
    assert e.value.code == drt.ERR_INVALID and "2^31" in str(e.value)


def test_the_header_states_the_rule_and_its_limits():
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    sec = text[text.index("nearest-triangle lists of points (new"):text.index("typedef struct drt_near ")]
    flat = re.sub(r"\s*\n \*\s*", " ", sec)
    for phrase in ("read as drt_renderer_nearest reads it", "drt_renderer_nearest's own on the stored (v0, e1, e2)", "Ericson case chain",
                   "carry the bits drt_renderer_nearest computes", "r2 = max_dist * max_dist", "listed iff dist2 < r2", "is never listed",
                   "r2 is some NaN and nothing is listed", "Alpha cut-outs are ignored",
                   "a.d2 < b.d2 || (a.d2 == b.d2 && a.prim < b.prim)", "total and independent of the traversal",
                   "offsets holds n + 1 uint32 values", "near[offsets[i] .. offsets[i+1])",
                   "cap_i = offsets[i+1] > offsets[i] ? offsets[i+1] - offsets[i] : 0", "offsets[i] + cap_i <= near_capacity",
                   "offsets[i] >= near_capacity gives 0", "and nothing else in near", "the miss record {r2, -1, 0, 0}", "the point's own product",
                   "surf may be NULL", "parallel array of near_capacity drt_near_surf records", "point = (v0 + e1 u) + e2 v",
                   "side = dot(p - point, fn) < 0 ? -1 : 1", "For a miss slot {0, 0, 0, 0}", "filled when the point finishes", "stay 16 bytes",
                   "evaluated at every pop and every push", "keep(box2) = (mode == DRT_NEAR_K && stored == cap_i) ? box2 <= tail.d2 : box2 < r2",
                   "The <= is deliberate", "equal d2 and smaller prim", "the root is pushed with its box2", "dropped unless keep(box2)",
                   "tests its triangles in order", "pushes each child that passes keep, the farther one first (b1 > b2 -> child 1)",
                   "the bound never shrinks", "counts[i] = total_i", "not just the stored ones", "the first cap_i of the full list",
                   "Each triangle lies in one leaf and the bound is constant", "near may be NULL iff near_capacity == 0", "a pure count",
                   "counts[i] = stored_i = min(cap_i, listed)", "A point with cap_i == 0 visits nothing and counts 0",
                   "fp32 box distances are not exactly conservative", "defined by this traversal, as drt_renderer_nearest's answer is",
                   "not by a brute force", "on every input tested they equal one", "counts may be NULL", "both near and counts NULL is DRT_ERR_INVALID"):
        assert phrase in flat, phrase
    limits = flat[flat.index("What this is not:"):]
    for phrase in ("point-to-point neighbours", "alpha-tested lists", "large-K", "moves one record per step", "has drt_renderer_nearest's d2",
                   "the smaller prim, not the first one found", "drt_renderer_list_hits', checked in its order", "handles are checked before n == 0",
                   "a mode outside {0, 1} is DRT_ERR_INVALID (checked first after the handles)", "n == 0 is a no-op", "n < 2^31",
                   "points, near and surf 16-byte aligned", "offsets and counts 4-byte aligned", "the call only enqueues", "refitted device copy",
                   "sharded renderer", "DRT_ERR_UNSUPPORTED beyond 64 levels", "DRT_ERR_INVALID while an asynchronous batch is pending",
                   "counters, kernel info and kernel span are not touched"):
        assert phrase in limits, phrase
    assert "drt_renderer_nearest_list" in text[:text.index("#define DRT_ABI_VERSION 2")]
    assert "#define DRT_NEAR_GATHER 0" in text and "#define DRT_NEAR_K      1" in text
    # the nearest section points here
    nearest = re.sub(r"\s*\n \*\s*", " ", text[text.index("nearest-surface queries (new"):text.index("typedef struct drt_point")])
    assert "k-nearest and radius-gather queries are drt_renderer_nearest_list, below" in nearest


def test_cpp_wrapper_compiles_and_links(tmp_path):
    src = tmp_path / "near_list_calls.cpp"
    src.write_text(r"""
#include <cstdio>
#include "DustRayTracer.hpp"
// the statements only -- main() runs none of them without arguments
int main(int argc, char **) {
    if (argc < 2) { std::printf("%zu %zu %zu %d\n", sizeof(drt_near), sizeof(drt_near_surf), sizeof(drt_point), DRT_ABI_VERSION); return 0; }
    Scene scene;
    Renderer r(0);
    const drt_point *points = nullptr;
    const uint32_t *offsets = nullptr;
    drt_near *near = nullptr;
    drt_near_surf *surf = nullptr;
    uint32_t *counts = nullptr;
    r.NearestList(scene, points, offsets, near, surf, 0u, counts, 0u, DRT_NEAR_K);
    r.NearestList(scene, points, offsets, near, surf, 0u, counts, 0u, DRT_NEAR_GATHER, nullptr);
    return 0;
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    exe = tmp_path / "near_list_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib_dir, "-ldrt_hip",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["16", "16", "16", "2"]
