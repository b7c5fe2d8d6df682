"""The ambient-occlusion entry point of include/drt.h without a GPU: exported, bound, laid out as declared, every argument check that
comes before any device work, the header states the rule and what it is not, and the C++ wrapper compiles and links against it."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.scenes import ROOT, scene_path

drt = pytest.importorskip("dustraytracer_amd")


def test_the_symbol_is_exported_and_bound():
    lib = ctypes.CDLL(drt.LIB_PATH)
    P, U = ctypes.c_void_p, ctypes.c_uint32
    assert hasattr(lib, "drt_renderer_ambient_occlusion") and hasattr(lib, "drt_debug_ambient_stats")
    fn = drt._lib.drt_renderer_ambient_occlusion
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == [P, P, P, U, P, P, P]
    assert callable(drt.Renderer.ambientOcclusion)
    assert drt.AmbientOcclusion._fields == ("open", "visibility", "bent", "sums") and drt.AO_MAX_SAMPLES == 4096
    doc = " ".join(drt.Renderer.ambientOcclusion.__doc__.split())
    for phrase in ("No distance falloff", "not stratified", "no indirect light", "no filtering across points", "unit normals", "-1 = a skipped point"):
        assert phrase in doc, phrase
    assert drt._lib.drt_abi_version() == 2


def test_record_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "drt.h"
int main(void) {
    printf("%zu %zu %zu %zu\n", sizeof(drt_ao_point), sizeof(drt_ao_result), sizeof(drt_ao_params), sizeof(drt_ray));
    printf("%zu %zu %zu %zu\n", offsetof(drt_ao_point, p), offsetof(drt_ao_point, max_dist), offsetof(drt_ao_point, n), offsetof(drt_ao_point, bias));
    printf("%zu %zu %zu %zu\n", offsetof(drt_ray, org), offsetof(drt_ray, tmin), offsetof(drt_ray, dir), offsetof(drt_ray, tmax));
    printf("%zu %zu\n", offsetof(drt_ao_result, open), offsetof(drt_ao_result, bent));
    printf("%zu %zu %zu %zu\n", offsetof(drt_ao_params, samples), offsetof(drt_ao_params, seed), offsetof(drt_ao_params, first), offsetof(drt_ao_params, flags));
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["32", "16", "16", "32", "0", "12", "16", "28", "0", "12", "16", "28", "0", "4", "0", "4", "8", "12"]


def test_every_argument_is_checked_before_any_device_work():
    L = drt._lib
    ao = L.drt_renderer_ambient_occlusion
    built = drt.Scene()
    built.loadGLTFmodel(scene_path("cornell_box"))
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
    b.buildIterative(built)
    bare = drt.Scene()                                           # no BVH

    def params(samples=64, seed=0, first=0, flags=0):
        return (ctypes.c_uint32 * 4)(samples, seed, first, flags)

    stand_in = ctypes.create_string_buffer(1 << 16)              # a block of zeros stands in for the renderer: it is not looked at yet
    h = ctypes.addressof(stand_in)
    pts = ctypes.create_string_buffer(32 * 4 + 16)
    P = (ctypes.addressof(pts) + 15) & ~15
    out = ctypes.create_string_buffer(16 * 4 + 16)
    O = (ctypes.addressof(out) + 15) & ~15
    ok = params()
    # the handles and the parameters come first, before n == 0
    for args in ((None, built._h, P, 4, ok, O), (h, None, P, 4, ok, O), (h, built._h, P, 4, None, O), (None, built._h, None, 0, ok, None)):
        assert ao(*args, None) == drt.ERR_INVALID and b"null argument" in L.drt_last_error()
    for samples in (0, 4097, 2 ** 32 - 1):
        assert ao(h, built._h, P, 4, params(samples=samples), O, None) == drt.ERR_INVALID and b"1 .. 4096" in L.drt_last_error()
        assert ao(h, built._h, None, 0, params(samples=samples), None, None) == drt.ERR_INVALID                  # also with n == 0
    assert ao(h, built._h, P, 4, params(flags=1), O, None) == drt.ERR_INVALID and b"flags" in L.drt_last_error()
    for samples in (1, 4096):
        assert ao(h, built._h, None, 0, params(samples=samples), None, None) == drt.OK                           # n == 0: nothing to do
    assert ao(h, bare._h, None, 0, ok, None, None) == drt.OK
    for what, p, o in (("null pts", None, O), ("null out", P, None)):
        assert ao(h, built._h, p, 4, ok, o, None) == drt.ERR_INVALID and b"null point or result" in L.drt_last_error(), what
    for what, p, o in (("misaligned pts", P + 4, O), ("misaligned out", P, O + 8)):
        assert ao(h, built._h, p, 4, ok, o, None) == drt.ERR_INVALID and b"16-byte aligned" in L.drt_last_error(), what
    assert ao(h, built._h, P, 0x80000000, ok, O, None) == drt.ERR_INVALID and b"2^31" in L.drt_last_error()
    assert ao(h, built._h, P, 2, params(first=2 ** 32 - 1), O, None) == drt.ERR_INVALID and b"2^32" in L.drt_last_error()
    assert ao(h, bare._h, P, 4, ok, O, None) == drt.ERR_INVALID and b"no BVH" in L.drt_last_error()
    # all of them passed: only now the renderer is looked at (zeros: no batch pending) and the device asked for -- host memory or no
    # device, either way the call fails after the checks
    assert ao(h, built._h, P, 4, ok, O, None) in (drt.ERR_INVALID, drt.ERR_DEVICE)
    assert b"device" in L.drt_last_error().lower() or b"hip" in L.drt_last_error().lower()


def test_bad_arguments_are_refused_by_the_python_interface_before_any_device_work():
    r = drt.Renderer.__new__(drt.Renderer)                                     # (no device: only the argument check runs)
    r._device = 0
    sc = drt.Scene()
    p, n1 = np.zeros((3, 3), np.float32), np.tile(np.float32([0, 0, 1]), (3, 1))
    refs = drt.SurfaceSamples(np.zeros(3, np.int32), np.zeros(3, np.float32), np.zeros(3, np.float32))
    for call, word in ((lambda: r.ambientOcclusion(sc, points=p, normals=n1, samples=0), "1 .. 4096"),
                       (lambda: r.ambientOcclusion(sc, points=p, normals=n1, samples=4097), "1 .. 4096"),
                       (lambda: r.ambientOcclusion(sc, points=p, normals=n1, seed=2 ** 32), "seed"),
                       (lambda: r.ambientOcclusion(sc, points=p, normals=n1, first=-1), "first"),
                       (lambda: r.ambientOcclusion(sc, points=p, normals=n1, first=2 ** 32 - 2), "2^32"),
                       (lambda: r.ambientOcclusion(sc), "refs, or points= and normals="),
                       (lambda: r.ambientOcclusion(sc, refs, points=p, normals=n1), "refs, or points= and normals="),
                       (lambda: r.ambientOcclusion(sc, points=p), "come with normals="),
                       (lambda: r.ambientOcclusion(sc, refs, normals=n1), "come with points="),
                       (lambda: r.ambientOcclusion(sc, (1, 2, 3)), ".prim, .u and .v"),
                       (lambda: r.ambientOcclusion(sc, points=[[0, 0, 0]], normals=n1), "numpy array or a torch tensor"),
                       (lambda: r.ambientOcclusion(sc, points=p.astype(np.float64), normals=n1), "dtype"),
                       (lambda: r.ambientOcclusion(sc, points=p, normals=n1[:2]), "shape"),
                       (lambda: r.ambientOcclusion(sc, points=p, normals=n1, facing=n1[:, :2]), "facing"),
                       (lambda: r.ambientOcclusion(sc, points=p, normals=n1, max_dist=np.ones(2, np.float32)), "max_dist"),
                       (lambda: r.ambientOcclusion(sc, points=p, normals=n1, bias="x"), "bias"),
                       (lambda: r.ambientOcclusion(sc, points=p, normals=n1, side=np.ones((3, 1), np.float32)), "side")):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == drt.ERR_INVALID and word in str(e.value), word


def test_the_header_states_the_rule_and_what_it_is_not():
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    sec = text[text.index("ambient occlusion (new"):text.index("typedef struct drt_ao_point ")]
    flat = re.sub(r" +", " ", re.sub(r"\s*\n \*\s*", " ", sec))
    for phrase in ("fp32 with one rounding per operation, in the order written", "dot(a, b) = a.x b.x + a.y b.y + a.z b.z",
                   "normalize(v) = v * (1.0f / sqrtf(dot(v, v)))", "drt_ao_point {p[3], max_dist, n[3], bias}: 32 bytes, the layout of drt_ray",
                   "drt_ao_params {samples, seed, first, flags}", "1 <= S <= 4096", "first + n <= 2^32", "flags must be 0",
                   "h pcg((first + i) ^ pcg(seed))", "state pcg(j ^ h)", "fuzz randomUnitSphereVec3(state)", "until len * len < 1",
                   "the 1024th candidate is kept", "d normalize(n + fuzz)", "o p + n * bias",
                   "{o, tmin = 0, d, tmax = max_dist}", "e < 0 || e > tmax", "e >= 0 && !(e > tmax)", "t > tmin && t < tmax && AnyHit",
                   "Otherwise the sample is open", "n is used as given: pass a unit normal for a cosine-weighted answer", "No guard is added",
                   "a NaN anywhere in o or d hits nothing, as in drt_renderer_occluded, and the sample counts as open",
                   "drt_ao_result {open, bent[3]}: 16 bytes", "the number of open samples",
                   "the sum over the open samples of (int32_t)(d[k] * 65536.0f): the product is exact, the cast truncates",
                   "A product that is a NaN or not below 2^31 in magnitude adds 0", "|bent[k]| <= 4096 * 65536 = 2^28: it cannot overflow",
                   "a point with !(max_dist >= 0) (negative or a NaN) costs no rays; its record is {-1, 0, 0, 0}", "max_dist = +inf: sky visibility",
                   "max_dist = 0: every sample is open", "the same bytes whatever order, tiling or hardware computes it", "that is why bent is not a float",
                   "a batch split in two with `first` gives the same records", "After drt_renderer_refit the moved mesh occludes",
                   "a tile of 64 lanes", "samples [64 t, min(64 t + 64, S)) of one point", "S in {1, 2, 4, 8, 16, 32} 64 / S consecutive points",
                   "one point with idle lanes", "The tile count is a 64-bit number", "one 16-byte store (S <= 64)", "integer atomics (S > 64)",
                   "writes the skipped points' records", "There are no floating-point atomics",
                   "every argument checked before any device work", "samples 0 or > 4096, flags != 0, n == 0 is a no-op, NULL pts or out",
                   "a scene without a BVH, a pending asynchronous batch", "DRT_ERR_UNSUPPORTED for trees deeper than 64 levels",
                   "in order with the other queries (the same event)", "counters, kernel info and kernel span are not touched"):
        assert phrase in flat, phrase
    limits = flat[flat.index("What this is not:"):]
    for phrase in ("no distance falloff and no weighting beyond the cosine of the draw", "no stratified or low-discrepancy directions",
                   "no indirect light -- drt_renderer_radiance does that", "no filtering across points",
                   "the absolute bias and the ray family's 1e-6 apply as in drt_renderer_trace_rays", "working range",
                   "no drt_group_* form and no command line"):
        assert phrase in limits, phrase
    before = re.sub(r"\s*\n \*\s*", " ", text[:text.index("#define DRT_ABI_VERSION 2")])
    assert "the ambient-occlusion entry point (drt_renderer_ambient_occlusion)" in before


def test_cpp_wrapper_compiles_and_links(tmp_path):
    src = tmp_path / "ambient_calls.cpp"
    src.write_text(r"""
#include <cstdio>
#include "DustRayTracer.hpp"
// the statements only -- main() runs none of them without arguments
int main(int argc, char **) {
    if (argc < 2) { std::printf("%zu %zu %zu %d\n", sizeof(drt_ao_point), sizeof(drt_ao_result), alignof(drt_ao_result), DRT_ABI_VERSION); return 0; }
    Scene scene;
    Renderer r(0);
    const drt_ao_point *points = nullptr;
    drt_ao_result *out = nullptr;
    r.AmbientOcclusion(scene, points, out, 0u);
    r.AmbientOcclusion(scene, points, out, 0u, 256u, 7u, 100u, nullptr);
    return 0;
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    exe = tmp_path / "ambient_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib_dir, "-ldrt_hip",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["32", "16", "4", "2"]
