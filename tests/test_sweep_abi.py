"""The sphere-cast entry point of include/drt.h without a GPU: exported, bound, laid out as declared, the argument checks that come
before any device work, the header states the rule and names the containment branches, and the C++ wrapper compiles and links
against it."""
import ctypes
import os
import re
import subprocess

import pytest

from tests.scenes import ROOT

drt = pytest.importorskip("dustraytracer_amd")


def test_the_symbol_is_exported_and_bound():
    lib = ctypes.CDLL(drt.LIB_PATH)
    assert hasattr(lib, "drt_renderer_sphere_cast")
    fn = drt._lib.drt_renderer_sphere_cast
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 7 and fn.argtypes[5] is ctypes.c_uint32
    assert callable(drt.Renderer.sphereCast)
    assert drt.SphereHits._fields == ("t", "prim", "u", "v", "point", "feature")
    assert drt._lib.drt_abi_version() == 2


def test_record_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "drt.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(drt_sweep_hit), offsetof(drt_sweep_hit, t), offsetof(drt_sweep_hit, prim), offsetof(drt_sweep_hit, u),
           offsetof(drt_sweep_hit, v), offsetof(drt_sweep_hit, point), offsetof(drt_sweep_hit, feature));
    printf("%zu %d\n", sizeof(drt_ray), DRT_ABI_VERSION);
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["32", "0", "4", "8", "12", "16", "28", "32", "2"]


def test_null_handles_are_invalid_without_a_gpu():
    L = drt._lib
    sc = drt.Scene()
    assert L.drt_renderer_sphere_cast(None, sc._h, None, None, None, 4, None) == drt.ERR_INVALID
    assert b"null" in L.drt_last_error()
    assert L.drt_renderer_sphere_cast(None, None, None, None, None, 0, None) == drt.ERR_INVALID      # the handles are checked before n == 0


def test_the_header_states_the_rule_and_names_the_containment_branches():
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    assert "the sphere-cast entry point (drt_renderer_sphere_cast)" in re.sub(r"\s*\n \*\s*", " ", text[:text.index("#define DRT_ABI_VERSION")])
    sec = text[text.index("sphere casts (new"):text.index("typedef struct drt_sweep_hit")]
    flat = re.sub(r"\s*\n \*\s*", " ", sec)
    for phrase in ("one rounding per operation", "dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z", "correctly rounded division", "correctly rounded square root",
                   "smallest t in [tmin, tmax)", "union of seven convex shapes", "overlap on purpose", "whole cylinder", "whole sphere", "Voronoi region",
                   "s = o + d tmin", "dd = dot(d, d)", "r2 = r r", "t = tmin + tau", "only on a strict <",
                   "n = cross(e1, e2), k = r sqrt(dot(n, n)), h = dot(n, m0), dn = dot(n, d)", "Containment branch: |h| <= k",
                   "(h > 0 && dn < 0) || (h < 0 && dn > 0)", "tau = (|h| - k) / |dn|", "den = d11 d22 - d12 d12",
                   "den > 0 && nu >= 0 && nv >= 0 && nu + nv <= den", "no face candidate", "Cq = ee c - me me", "Containment branch: Cq <= 0",
                   "A > 0 && B < 0", "disc = ee (A r2 - det det) >= 0", "tau = Cq / (sqrt(disc) - B)", "ee > 0 && ax >= 0 && ax <= ee",
                   "Containment branch: c <= 0", "dd > 0 && b < 0", "disc = dd r2 - dot(x, x) >= 0", "tau = c / (sqrt(disc) - b)",
                   "quotient of two positive numbers", "no separate start-overlap test", "adds 8 to the feature",
                   "t < best || (t == best && k < prim)", "does not depend on the tree", "t0 = ((bmin - r) - o) inv_dir", "t1 = ((bmax + r) - o) inv_dir",
                   "enter <= exit && exit >= tmin && enter <= best", "the farther one first", "A zero direction gives the static overlap test",
                   "point = (v0 + e1 u) + e2 v", "(o + d t) - point", "{tmax, -1, 0, 0, 0, 0, 0, -1}", "a negative or NaN radius", "a NaN ray",
                   "an empty scene", "depends on its cast and the scene only"):
        assert phrase in flat, phrase
    limits = flat[flat.index("What this is not:"):]
    for phrase in ("alpha cut-outs are ignored", "penetration depth", "radii a float[n] 4-byte aligned", "refitted device copy", "sharded renderer",
                   "DRT_ERR_UNSUPPORTED beyond 64 levels", "DRT_ERR_INVALID while an asynchronous batch is pending", "kernel info and kernel span are not touched"):
        assert phrase in limits, phrase


def test_cpp_wrapper_compiles_and_links(tmp_path):
    src = tmp_path / "sphere_cast_calls.cpp"
    src.write_text(r"""
#include <cstdio>
#include "DustRayTracer.hpp"
// the statements only -- main() runs none of them without arguments
int main(int argc, char **) {
    if (argc < 2) { std::printf("%zu %zu\n", sizeof(drt_ray), sizeof(drt_sweep_hit)); return 0; }
    Scene scene;
    Renderer r(0);
    const drt_ray *rays = nullptr;
    const float *radii = nullptr;
    drt_sweep_hit *out = nullptr;
    r.SphereCast(scene, rays, radii, out, 0);
    r.SphereCast(scene, rays, radii, out, 0, nullptr);
    return 0;
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    exe = tmp_path / "sphere_cast_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib_dir, "-ldrt_hip",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["32", "32"]
