"""The nearest-surface entry point of include/drt.h without a GPU: exported, bound, laid out as declared, the argument checks that come
before any device work, the header states the rule and the limits of `side`, and the C++ wrapper compiles and links against it."""
import ctypes
import os
import re
import subprocess

import pytest

from tests.scenes import ROOT

drt = pytest.importorskip("dustraytracer_amd")


def test_the_symbol_is_exported_and_bound():
    lib = ctypes.CDLL(drt.LIB_PATH)
    assert hasattr(lib, "drt_renderer_nearest")
    fn = drt._lib.drt_renderer_nearest
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 6 and fn.argtypes[4] is ctypes.c_uint32
    assert callable(drt.Renderer.nearest)
    assert drt.Nearest._fields == ("point", "d2", "prim", "u", "v", "side")
    assert drt._lib.drt_abi_version() == 2


def test_record_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "drt.h"
int main(void) {
    printf("%zu %zu %zu\n", sizeof(drt_point), offsetof(drt_point, p), offsetof(drt_point, max_dist));
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(drt_nearest), offsetof(drt_nearest, point), offsetof(drt_nearest, d2), offsetof(drt_nearest, prim),
           offsetof(drt_nearest, u), offsetof(drt_nearest, v), offsetof(drt_nearest, side));
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["16", "0", "12", "32", "0", "12", "16", "20", "24", "28"]


def test_null_handles_are_invalid_without_a_gpu():
    L = drt._lib
    sc = drt.Scene()
    assert L.drt_renderer_nearest(None, sc._h, None, None, 4, None) == drt.ERR_INVALID
    assert b"null" in L.drt_last_error()
    assert L.drt_renderer_nearest(None, None, None, None, 0, None) == drt.ERR_INVALID      # the handles are checked before n == 0


def test_the_header_states_the_rule_and_the_limits_of_side():
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    sec = text[text.index("nearest-surface queries (new"):text.index("typedef struct drt_point")]
    flat = re.sub(r"\s*\n \*\s*", " ", sec)
    for phrase in ("one rounding per operation", "dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z", "correctly rounded division", "Ericson",
                   "vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4", "d1 <= 0 && d2 <= 0", "d3 >= 0 && d4 <= d3",
                   "vc <= 0 && d1 >= 0 && d3 <= 0", "d6 >= 0 && d5 <= d6", "vb <= 0 && d2 >= 0 && d6 <= 0",
                   "va <= 0 && d4 - d3 >= 0 && d5 - d6 >= 0", "den = 1 / ((va + vb) + vc)", "c = (v0 + e1 u) + e2 v", "never wins",
                   "d = fmaxf(fmaxf(bmin - p, 0), p - bmax)", "box2 = (dx dx + dy dy) + dz dz", "best = max_dist * max_dist",
                   "dropped unless box2 < best", "the first one found wins a tie", "b1 > b2 -> child 1",
                   "side = dot(p - c, fn) < 0 ? -1 : 1", "{0, 0, 0, max_dist * max_dist, -1, 0, 0, 0}", "depends on its point and the scene only"):
        assert phrase in flat, phrase
    limits = flat[flat.index("What this is not:"):]
    for phrase in ("alpha cut-outs are ignored", "not an inside / outside classification", "non-convex", "parity test", "pseudonormals",
                   "k-nearest", "radius-gather", "refitted device copy", "sharded renderer", "DRT_ERR_UNSUPPORTED beyond 64 levels",
                   "DRT_ERR_INVALID while an asynchronous batch is pending"):
        assert phrase in limits, phrase


def test_cpp_wrapper_compiles_and_links(tmp_path):
    src = tmp_path / "nearest_calls.cpp"
    src.write_text(r"""
#include <cstdio>
#include "DustRayTracer.hpp"
// the statements only -- main() runs none of them without arguments
int main(int argc, char **) {
    if (argc < 2) { std::printf("%zu %zu\n", sizeof(drt_point), sizeof(drt_nearest)); return 0; }
    Scene scene;
    Renderer r(0);
    const drt_point *points = nullptr;
    drt_nearest *out = nullptr;
    r.Nearest(scene, points, out, 0);
    r.Nearest(scene, points, out, 0, nullptr);
    return 0;
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    exe = tmp_path / "nearest_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib_dir, "-ldrt_hip",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["16", "32"]
