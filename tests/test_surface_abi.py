"""The surface entry points of include/drt.h without a GPU: exported, bound, laid out as declared, the argument checks that come
before any device work, the header states the rules and their departures, and the C++ wrapper compiles and links against them."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.scenes import ROOT

drt = pytest.importorskip("dustraytracer_amd")


def test_the_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(drt.LIB_PATH)
    P, U = ctypes.c_void_p, ctypes.c_uint32
    for name, argtypes in (("drt_renderer_surface_lookup", [P, P, P, P, P, U, P]), ("drt_renderer_surface_weights", [P, P, P, P]),
                           ("drt_renderer_sample_surface", [P, P, U, U, P, U, P])):
        assert hasattr(lib, name), name
        fn = getattr(drt._lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == argtypes, name
    for method in ("surface", "sampleSurface", "surfaceWeights"):
        assert callable(getattr(drt.Renderer, method)), method
    assert drt.Surface._fields == ("position", "normal", "shading", "uv", "albedo", "emissive", "alpha", "roughness", "refractive_index",
                                   "material", "load_index", "texture", "metallic", "transmission")
    assert drt.SurfaceSamples._fields == ("prim", "u", "v")
    assert drt.SURFACE_SCAN_BLOCK == 256
    doc = drt.Renderer.surface.__doc__
    assert "not normalised" in " ".join(doc.split()) and "no normal maps" in doc and "nearest texel" in doc
    assert "not stratified" in drt.Renderer.sampleSurface.__doc__
    assert drt._lib.drt_abi_version() == 2


def test_record_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "drt.h"
int main(void) {
    printf("%zu %zu\n", sizeof(drt_surface), sizeof(drt_hit));
    printf("%zu %zu %zu %zu %zu %zu\n", offsetof(drt_surface, position), offsetof(drt_surface, material), offsetof(drt_surface, normal),
           offsetof(drt_surface, alpha), offsetof(drt_surface, shading), offsetof(drt_surface, load_index));
    printf("%zu %zu %zu %zu %zu %zu %zu\n", offsetof(drt_surface, albedo), offsetof(drt_surface, texture), offsetof(drt_surface, uv),
           offsetof(drt_surface, roughness), offsetof(drt_surface, flags), offsetof(drt_surface, emissive), offsetof(drt_surface, refractive_index));
    printf("%zu %zu %zu %zu\n", offsetof(drt_hit, t), offsetof(drt_hit, prim), offsetof(drt_hit, u), offsetof(drt_hit, v));
    printf("%d %d\n", DRT_SURFACE_SCAN_BLOCK, DRT_ABI_VERSION);
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["96", "16", "0", "12", "16", "28", "32", "44", "48", "60", "64", "72", "76", "80", "92", "0", "4", "8", "12", "256", "2"]


def test_the_argument_checks_come_in_the_ray_query_s_order():
    L = drt._lib
    sc = drt.Scene()
    look, weights, sample = L.drt_renderer_surface_lookup, L.drt_renderer_surface_weights, L.drt_renderer_sample_surface
    # the handles are checked first, before n == 0
    assert look(None, sc._h, None, None, None, 0, None) == drt.ERR_INVALID and b"null" in L.drt_last_error()
    assert sample(None, sc._h, 1, 0, None, 0, None) == drt.ERR_INVALID and b"null" in L.drt_last_error()
    assert weights(None, sc._h, None, None) == drt.ERR_INVALID and b"null" in L.drt_last_error()
    stand_in = ctypes.create_string_buffer(1 << 16)          # a block of zeros stands in for the renderer: it is not looked at yet
    h = ctypes.addressof(stand_in)
    assert look(h, None, None, None, None, 4, None) == drt.ERR_INVALID
    refs = ctypes.create_string_buffer(16 * 4 + 16)
    R = (ctypes.addressof(refs) + 15) & ~15
    out = ctypes.create_string_buffer(96 * 4 + 16)
    O = (ctypes.addressof(out) + 15) & ~15
    assert look(h, sc._h, None, None, None, 0, None) == drt.OK                    # n == 0: nothing to do
    assert sample(h, sc._h, 1, 0, None, 0, None) == drt.OK
    for what, args in (("null refs", (None, None, O)), ("null out", (R, None, None))):
        assert look(h, sc._h, *args, 4, None) == drt.ERR_INVALID, what
        assert b"null reference or result" in L.drt_last_error(), what
    for what, args in (("misaligned refs", (R + 4, None, O)), ("misaligned out", (R, None, O + 8)), ("misaligned normals", (R, O + 2, O))):
        assert look(h, sc._h, *args, 4, None) == drt.ERR_INVALID, what
        assert b"aligned" in L.drt_last_error(), what
    assert look(h, sc._h, R, None, O, 0x80000000, None) == drt.ERR_INVALID and b"2^31" in L.drt_last_error()
    assert sample(h, sc._h, 1, 0, None, 4, None) == drt.ERR_INVALID and b"null result" in L.drt_last_error()
    assert sample(h, sc._h, 1, 0, O + 8, 4, None) == drt.ERR_INVALID and b"16-byte aligned" in L.drt_last_error()
    assert sample(h, sc._h, 1, 0, O, 0x80000000, None) == drt.ERR_INVALID and b"2^31" in L.drt_last_error()
    assert sample(h, sc._h, 1, 0xFFFFFFFF, O, 2, None) == drt.ERR_INVALID and b"2^32" in L.drt_last_error()
    assert sample(h, sc._h, 1, 0xFFFFFFFD, O, 4, None) == drt.ERR_INVALID and b"2^32" in L.drt_last_error()
    assert weights(h, sc._h, None, None) == drt.ERR_INVALID and b"null table" in L.drt_last_error()
    assert weights(h, sc._h, O + 8, None) == drt.ERR_INVALID and b"16-byte aligned" in L.drt_last_error()


def test_bad_arguments_are_refused_before_any_device_work():
    r = drt.Renderer.__new__(drt.Renderer)                                     # (no device: only the argument check runs)
    r._device = 0
    sc = drt.Scene()
    prim, u = np.zeros(3, np.int32), np.zeros(3, np.float32)
    for call, word in ((lambda: r.surface(sc, prim), ".prim"), (lambda: r.surface(sc, prim, u), "prim, u and v"),
                       (lambda: r.surface(sc, prim.astype(np.int64), u, u), "dtype"), (lambda: r.surface(sc, prim, u.astype(np.float64), u), "dtype"),
                       (lambda: r.surface(sc, prim, u, u[:2]), "shape"), (lambda: r.surface(sc, [0, 1, 2], u, u), "numpy array or a torch tensor"),
                       (lambda: r.sampleSurface(sc, -1), "n >= 0"), (lambda: r.sampleSurface(sc, 2, first=2 ** 32 - 1), "2^32"),
                       (lambda: r.sampleSurface(sc, 2, seed=2 ** 32), "seed")):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == drt.ERR_INVALID and word in str(e.value), word


def test_the_header_states_the_rules_and_their_departures():
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    sec = text[text.index("surface lookups and area-weighted sampling (new"):text.index("typedef struct drt_surface ")]
    flat = re.sub(r" +", " ", re.sub(r"\s*\n \*\s*", " ", sec))
    for phrase in ("Neither traverses the BVH", "fp32 with one rounding per operation, in the order written",
                   "n drt_hit {t, prim, u, v} (16 bytes, 16-byte aligned)", "t is not read", "96 bytes, 16-byte aligned, written with six 16-byte stores",
                   "0 <= prim < n_tris", "all zero bits except material = load_index = texture = -1", "no clamp", "w = 1.0f - u - v",
                   "(v0 + u e1) + v e2 per component", "after drt_renderer_refit the moved triangle", "the stored face normal, as is", "not turned",
                   "which NaN is not specified", "(w uv0 + u uv1) + v uv2", "its flat albedo, alpha = 1", "f = c - floorf(c)",
                   "x = (int)(f.x width), y = (int)(f.y height)", "the texel y width + x", "followed by width + 1 zero texels",
                   "albedo = (c / 255)^2 per channel for 3 and 4 channels, (0, 0, 1) for any other count", "alpha = a / 255 with 4 channels, else 1",
                   "fails f >= 0 && f <= 1 is taken as 0 before the conversion", "A finite uv is unaffected", "nothing is read outside the pool",
                   "flags bit 0 = metallic, bit 1 = transmission", "(w N0 + u N1) + v N2", "NOT normalised and not turned",
                   "normals = NULL: the HOST scene's vertex normals", "also after a drt_renderer_refit that was given others",
                   "float[n_tris][3][3] in LOAD order", "used instead and not retained", "drt_scene_get_triangle_order's entry of prim",
                   "a = sqrtf((c.x c.x + c.y c.y) + c.z c.z)", "A non-finite a", "counts as 0", "amax == 0: every q is 0",
                   "frexp's exponent of amax", "(uint64_t)ldexp((double)a_k, 35 - e), truncated", "exact in double", "q_k < 2^36",
                   "smaller than amax 2^-36 has weight 0", "cdf[k] q_0 + ... + q_k", "total = cdf[n_tris - 1]", "no workgroup waits for another",
                   "A mesh scaled by a power of two has the same table", "i = first + k; first + n <= 2^32",
                   "s = pcg(i ^ pcg(seed)), h1 = pcg(s), h2 = pcg(h1), h3 = pcg(h2), h4 = pcg(h3)", "R = (uint64_t)h1 << 32 | h2",
                   "the high 64 bits of R total", "the smallest k with cdf[k] > target", "A triangle of weight 0 is never drawn",
                   "the miss record {0, -1, 0, 0}", "a = h3 >> 8, b = h4 >> 8", "if a + b > 2^24 then a = 2^24 - a and b = 2^24 - b",
                   "u = a 2^-24, v = b 2^-24", "w = 1 - u - v is exact and >= 0", "drt_hit {t = 0, prim, u, v}",
                   "a batch split in two with `first` gives the same records", "computed again by every call", "the moved mesh is sampled",
                   "a scene without a BVH is refused", "DRT_ERR_INVALID while an asynchronous batch is pending", "legal on a sharded renderer",
                   "counters, kernel info and kernel span are not touched"):
        assert phrase in flat, phrase
    limits = flat[flat.index("What this is not:"):]
    for phrase in ("the nearest texel only", "no normal maps and no tangents", "shading is not normalised", "no stratified or blue-noise sampling",
                   "no drt_group_* form and no command line"):
        assert phrase in limits, phrase
    before = re.sub(r"\s*\n \*\s*", " ", text[:text.index("#define DRT_ABI_VERSION 2")])
    assert "the surface entry points (drt_renderer_surface_lookup, drt_renderer_surface_weights, drt_renderer_sample_surface)" in before


def test_cpp_wrapper_compiles_and_links(tmp_path):
    src = tmp_path / "surface_calls.cpp"
    src.write_text(r"""
#include <cstdio>
#include "DustRayTracer.hpp"
// the statements only -- main() runs none of them without arguments
int main(int argc, char **) {
    if (argc < 2) { std::printf("%zu %zu %zu %d\n", sizeof(drt_surface), alignof(drt_surface), sizeof(drt_hit), DRT_ABI_VERSION); return 0; }
    Scene scene;
    Renderer r(0);
    const drt_hit *refs = nullptr;
    drt_hit *samples = nullptr;
    drt_surface *out = nullptr;
    const float *normals = nullptr;
    uint64_t *cdf = nullptr;
    r.SurfaceLookup(scene, refs, out, 0u);
    r.SurfaceLookup(scene, refs, out, 0u, normals, nullptr);
    r.SurfaceWeights(scene, cdf);
    r.SampleSurface(scene, 7u, samples, 0u);
    r.SampleSurface(scene, 7u, samples, 0u, 5u, nullptr);
    return 0;
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    exe = tmp_path / "surface_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib_dir, "-ldrt_hip",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["96", "4", "16", "2"]
