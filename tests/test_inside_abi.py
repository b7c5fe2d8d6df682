"""The crossing-count entry points of include/drt.h without a GPU: exported, bound, laid out as declared, the argument checks that
come before any device work, the header states the rule and its limits, and the C++ wrapper compiles and links against them."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import inside_ref as ir
from tests.scenes import ROOT

drt = pytest.importorskip("dustraytracer_amd")

NAMES = ("drt_renderer_crossings", "drt_renderer_inside", "drt_renderer_signed_distance")


def test_the_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(drt.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
    fn = drt._lib.drt_renderer_crossings
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 6 and fn.argtypes[4] is ctypes.c_uint32
    for fn in (drt._lib.drt_renderer_inside, drt._lib.drt_renderer_signed_distance):
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 7 and fn.argtypes[4] is ctypes.c_uint32 and fn.argtypes[5] is ctypes.c_int32
    for method in ("crossings", "inside", "signedDistance", "sdfGrid"):
        assert callable(getattr(drt.Renderer, method)), method
    assert drt.Crossings._fields == ("count", "winding")
    assert drt.INSIDE_RULES == {"parity": 0, "winding": 1} == ir.RULES
    assert drt._lib.drt_abi_version() == 2


def test_record_layout_and_constants(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "drt.h"
int main(void) {
    drt_crossings c = {0u, -1};
    printf("%zu %zu %zu %d %d %d\n", sizeof(drt_crossings), offsetof(drt_crossings, count), offsetof(drt_crossings, winding), c.winding < 0 && c.count < 1u,
           DRT_INSIDE_PARITY, DRT_INSIDE_WINDING);
    printf("%zu %zu\n", sizeof(drt_nearest), offsetof(drt_nearest, side));
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["8", "0", "4", "1", "0", "1", "32", "28"]                  # the side word the vote replaces is at byte 28


def test_null_handles_are_invalid_without_a_gpu():
    L = drt._lib
    sc = drt.Scene()
    assert L.drt_renderer_crossings(None, sc._h, None, None, 4, None) == drt.ERR_INVALID
    assert b"null" in L.drt_last_error()
    assert L.drt_renderer_crossings(None, None, None, None, 0, None) == drt.ERR_INVALID       # the handles are checked before n == 0
    for fn in (L.drt_renderer_inside, L.drt_renderer_signed_distance):
        for rule in (0, 1):
            assert fn(None, sc._h, None, None, 4, rule, None) == drt.ERR_INVALID
            assert b"null" in L.drt_last_error()
            assert fn(None, None, None, None, 0, rule, None) == drt.ERR_INVALID


def test_a_bad_rule_is_refused_before_anything_else():
    L = drt._lib
    sc = drt.Scene()
    for fn in (L.drt_renderer_inside, L.drt_renderer_signed_distance):
        for rule in (2, -1, 7):
            assert fn(None, sc._h, None, None, 0, rule, None) == drt.ERR_INVALID
            msg = L.drt_last_error()
            assert b"rule" in msg and b"parity" in msg and b"null" not in msg, msg
    # the Python wrapper names the rules and refuses others before it touches a device
    r = drt.Renderer.__new__(drt.Renderer)                                     # (no device: only the argument check runs)
    r._device = 0
    for call in (lambda: r.inside(sc, np.zeros((1, 3), np.float32), rule="odd"), lambda: r.signedDistance(sc, np.zeros((1, 3), np.float32), rule=1),
                 lambda: r.sdfGrid(sc, 4, (0, 0, 0), (1, 1, 1), rule="even")):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == drt.ERR_INVALID and "parity" in str(e.value)


def test_the_header_states_the_rule_and_its_limits():
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    sec = text[text.index("crossing counts, inside / outside and signed distance (new"):text.index("typedef struct drt_crossings")]
    flat = re.sub(r"\s*\n \*\s*", " ", sec)
    for phrase in ("det = dot(e1, cross(dir, e2))", "counts iff the test hits, t > tmin and t < tmax", "Alpha cut-outs are ignored",
                   "(det < 0 ? +1 : -1)", "exits minus entries", "e1 x e2, not by the stored face normal", "without the early exit",
                   "the root is skipped if d < 0 || d > tmax", "a child is pushed iff d >= 0 && !(d > tmax)", "the farther child is pushed first",
                   "Each triangle lies in one leaf", "drt_crossings {count, winding}, 8 bytes", "an empty scene or a NaN ray gives {0, 0}",
                   "tmin = 0, tmax = +inf", "used as given, not normalised", "no component is zero", "count_j is odd (rule 0, parity)",
                   "winding_j != 0 (rule 1, winding)", "0..3; inside means 2 or more", "max_dist is ignored", "unchanged in its first seven words",
                   "-1 (inside) or +1 (outside)", "in miss records too"):
        assert phrase in flat, phrase
    # the directions, digit for digit, and the same values as the restatement's
    dirs = re.findall(r"D(\d) = \((-?[\d.]+)f, (-?[\d.]+)f, (-?[\d.]+)f\)", flat)
    assert [d[0] for d in dirs] == ["0", "1", "2"]
    assert (np.float32([[float(x) for x in d[1:]] for d in dirs]).view(np.uint32) == ir.DIRS.view(np.uint32)).all()
    assert (ir.DIRS != 0).all()
    limits = flat[flat.index("What this is not:"):]
    for phrase in ("a point on the surface has no defined answer", "parity assumes a closed mesh", "winding assumes consistent orientation as well",
                   "pseudonormals", "generalised winding numbers", "first K hits", "refitted device copy", "sharded renderer",
                   "DRT_ERR_UNSUPPORTED beyond 64 levels", "DRT_ERR_INVALID while an asynchronous batch is pending", "a rule other than 0 or 1",
                   "counters, kernel info and kernel span are not touched"):
        assert phrase in limits, phrase
    assert "drt_renderer_crossings / _inside / _signed_distance" in text[:text.index("#define DRT_ABI_VERSION 2")]


def test_cpp_wrapper_compiles_and_links(tmp_path):
    src = tmp_path / "inside_calls.cpp"
    src.write_text(r"""
#include <cstdio>
#include "DustRayTracer.hpp"
// the statements only -- main() runs none of them without arguments
int main(int argc, char **) {
    if (argc < 2) { std::printf("%zu %zu\n", sizeof(drt_crossings), sizeof(drt_nearest)); return 0; }
    Scene scene;
    Renderer r(0);
    const drt_ray *rays = nullptr;
    const drt_point *points = nullptr;
    drt_crossings *counts = nullptr;
    uint8_t *votes = nullptr;
    drt_nearest *out = nullptr;
    r.Crossings(scene, rays, counts, 0);
    r.Crossings(scene, rays, counts, 0, nullptr);
    r.Inside(scene, points, votes, 0);
    r.Inside(scene, points, votes, 0, DRT_INSIDE_WINDING, nullptr);
    r.SignedDistance(scene, points, out, 0);
    r.SignedDistance(scene, points, out, 0, DRT_INSIDE_PARITY, nullptr);
    return 0;
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    exe = tmp_path / "inside_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib_dir, "-ldrt_hip",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["8", "32"]
