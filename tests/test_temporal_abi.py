"""The temporal entry points of include/drt.h without a GPU: exported, bound, laid out as declared, defaults, argument checks that
come before any device work, and the C++ wrapper and the CLI compile against them."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests.scenes import ROOT

drt = pytest.importorskip("dustraytracer_amd")

NEW = ["drt_default_temporal_params", "drt_renderer_temporal_denoise", "drt_renderer_temporal_reset", "drt_renderer_read_temporal",
       "drt_renderer_device_temporal"]


def test_the_new_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(drt.LIB_PATH)
    assert all(hasattr(lib, n) for n in NEW)
    src = open(os.path.join(ROOT, "dustraytracer_amd", "__init__.py")).read()
    assert all(n in src for n in NEW)
    for name in ("TemporalDenoise", "resetTemporalHistory", "GetTemporalHistory", "DeviceTemporalHistory"):
        assert callable(getattr(drt.Renderer, name))
    assert drt.TemporalHistory._fields == ("color", "length", "moments", "variance", "weight")
    assert drt._lib.drt_abi_version() == 2


def test_pod_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "drt.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(drt_temporal_params), offsetof(drt_temporal_params, iterations),
           offsetof(drt_temporal_params, max_history), offsetof(drt_temporal_params, alpha_min), offsetof(drt_temporal_params, normal_cos_min),
           offsetof(drt_temporal_params, sigma_luma), offsetof(drt_temporal_params, sigma_normal), offsetof(drt_temporal_params, sigma_albedo));
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["28", "0", "4", "8", "12", "16", "20", "24"]
    assert ctypes.sizeof(drt.TemporalParams) == 28
    assert [(n, getattr(drt.TemporalParams, n).offset) for n, _ in drt.TemporalParams._fields_] == \
        [("iterations", 0), ("max_history", 4), ("alpha_min", 8), ("normal_cos_min", 12), ("sigma_luma", 16), ("sigma_normal", 20), ("sigma_albedo", 24)]


def test_default_parameters():
    raw = drt.TemporalParams.from_buffer_copy(bytes(28))
    drt._lib.drt_default_temporal_params(ctypes.byref(raw))
    assert (raw.iterations, raw.max_history) == (5, 32)
    assert [np.float32(getattr(raw, k)) for k in ("alpha_min", "normal_cos_min", "sigma_luma", "sigma_normal", "sigma_albedo")] == \
        [np.float32(0), np.float32(0.9), np.float32(4), np.float32(0.1), np.float32(0.1)]
    drt._lib.drt_default_temporal_params(None)                 # a NULL destination is ignored
    p = drt.TemporalParams(iterations=2, alpha_min=0.25)
    assert (p.iterations, p.max_history, p.alpha_min) == (2, 32, 0.25)
    with pytest.raises(TypeError):
        drt.TemporalParams(sigma_color=1.0)


def test_null_handles_are_invalid_without_a_gpu():
    L = drt._lib
    cam = drt.Camera()._pod()
    p = drt.TemporalParams()
    ms = ctypes.c_float(7.0)
    buf = np.zeros(4, np.float32)
    assert L.drt_renderer_temporal_denoise(None, ctypes.byref(cam), None, ctypes.byref(p), ctypes.byref(ms)) == drt.ERR_INVALID
    assert ms.value == 0.0
    assert L.drt_renderer_temporal_denoise(None, None, None, None, None) == drt.ERR_INVALID
    assert L.drt_renderer_temporal_reset(None) == drt.ERR_INVALID
    assert L.drt_renderer_read_temporal(None, 0, buf.ctypes.data, 4) == drt.ERR_INVALID
    assert L.drt_renderer_device_temporal(None, 0) is None
    assert b"null" in L.drt_last_error()


def test_cpp_wrapper_and_cli_compile(tmp_path):
    src = tmp_path / "temporal_calls.cpp"
    src.write_text(r"""
#include <cstdio>
#include <vector>
#include "DustRayTracer.hpp"
// the editor's per-frame loop with the temporal filter on (INTEGRATION.md): the statements only -- main() runs none of them without arguments
int main(int argc, char **) {
    if (argc < 2) { std::printf("%zu\n", sizeof(drt_temporal_params)); return 0; }
    Scene scene;
    Camera cam;
    Renderer r(0);
    r.ResizeBuffer(8, 8);
    float ms = 0;
    r.Render(&cam, scene, &ms);
    r.TemporalDenoise(&cam, scene, &ms);
    drt_temporal_params p;
    drt_default_temporal_params(&p);
    p.max_history = 8;
    r.TemporalDenoise(&cam, scene, &ms, &p);
    std::vector<float> img(8 * 8 * 4);
    r.ReadDenoisedTarget(img.data());
    r.ReadTemporal(0, img.data());
    r.ReadTemporal(1, img.data());
    r.ResetTemporalHistory();
    return drt_renderer_device_temporal(r.handle, 0) != nullptr;
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    link = ["-L" + lib_dir, "-ldrt_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"]
    exe = tmp_path / "temporal_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)] + link + ["-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip() == "28"
    cli = tmp_path / "drt_render"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "drt_render.cpp")]
                       + link + ["-o", str(cli)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(cli), "--temporal", "4"], capture_output=True, text=True)    # the flag alone: usage, exit code 2
    assert r.returncode == 2 and "--temporal K" in r.stderr
