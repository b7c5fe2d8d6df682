"""The guide / denoise entry points of include/drt.h without a GPU: exported, bound, laid out as declared, defaults, argument
checks that come before any device work, and the C++ wrapper and the CLI compile against them."""
import ctypes
import os
import subprocess

import pytest

from tests.scenes import ROOT

drt = pytest.importorskip("dustraytracer_amd")

NEW = ["drt_renderer_render_guides", "drt_default_denoise_params", "drt_renderer_denoise", "drt_renderer_read_denoised_rgba32f",
       "drt_renderer_device_denoised"]


def test_the_new_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(drt.LIB_PATH)
    assert all(hasattr(lib, n) for n in NEW)
    src = open(os.path.join(ROOT, "dustraytracer_amd", "__init__.py")).read()
    assert all(n in src for n in NEW)
    for name in ("renderGuides", "Denoise", "GetDenoisedImage"):
        assert callable(getattr(drt.Renderer, name))
    assert drt.Guides._fields == ("albedo", "normal", "t", "prim")


def test_pod_layouts(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "drt.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu | %zu %zu %zu %zu %zu\n", sizeof(drt_guide), offsetof(drt_guide, albedo), offsetof(drt_guide, t),
           offsetof(drt_guide, normal), offsetof(drt_guide, prim), sizeof(drt_denoise_params), offsetof(drt_denoise_params, iterations),
           offsetof(drt_denoise_params, sigma_color), offsetof(drt_denoise_params, sigma_normal), offsetof(drt_denoise_params, sigma_albedo));
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["32", "0", "12", "16", "28", "|", "16", "0", "4", "8", "12"]
    assert ctypes.sizeof(drt.DenoiseParams) == 16


def test_default_parameters():
    p = drt.DenoiseParams()
    assert (p.iterations, p.sigma_color, p.sigma_normal, p.sigma_albedo) == (5, pytest.approx(0.5), pytest.approx(0.1), pytest.approx(0.1))
    raw = drt.DenoiseParams.from_buffer_copy(bytes(16))
    drt._lib.drt_default_denoise_params(ctypes.byref(raw))
    import numpy as np
    assert [raw.iterations] + [np.float32(getattr(raw, k)) for k in ("sigma_color", "sigma_normal", "sigma_albedo")] == \
        [5, np.float32(0.5), np.float32(0.1), np.float32(0.1)]
    drt._lib.drt_default_denoise_params(None)                  # a NULL destination is ignored
    assert drt.DenoiseParams(iterations=2, sigma_color=1.5).iterations == 2


def test_null_handles_are_invalid_without_a_gpu():
    L = drt._lib
    cam = drt.Camera()._pod()
    p = drt.DenoiseParams()
    ms = ctypes.c_float(7.0)
    assert L.drt_renderer_render_guides(None, ctypes.byref(cam), None, 1, None, None) == drt.ERR_INVALID
    assert L.drt_renderer_render_guides(None, None, None, 0, None, None) == drt.ERR_INVALID
    assert L.drt_renderer_denoise(None, ctypes.byref(cam), None, ctypes.byref(p), ctypes.byref(ms)) == drt.ERR_INVALID
    assert ms.value == 0.0
    assert L.drt_renderer_denoise(None, None, None, None, None) == drt.ERR_INVALID
    assert L.drt_renderer_read_denoised_rgba32f(None, None, 0) == drt.ERR_INVALID
    assert L.drt_renderer_device_denoised(None) is None
    assert b"null" in L.drt_last_error()


def test_cpp_wrapper_and_cli_compile(tmp_path):
    src = tmp_path / "denoise_calls.cpp"
    src.write_text(r"""
#include <cstdio>
#include <vector>
#include "DustRayTracer.hpp"
// the editor's "denoise" toggle (INTEGRATION.md): the statements only -- main() runs none of them without arguments
int main(int argc, char **) {
    if (argc < 2) { std::printf("%zu\n", sizeof(drt_guide)); return 0; }
    Scene scene;
    Camera cam;
    Renderer r(0);
    r.ResizeBuffer(8, 8);
    float ms = 0;
    r.Render(&cam, scene, &ms);
    r.Denoise(&cam, scene, &ms);
    r.Denoise(&cam, scene, &ms, 3, 0.25f, 0.2f, 0.05f);
    std::vector<float> img(8 * 8 * 4);
    r.ReadDenoisedTarget(img.data());
    void *dev = r.DeviceDenoisedTarget();
    r.RenderGuides(&cam, scene, 2, static_cast<drt_guide *>(dev), nullptr);
    return 0;
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    link = ["-L" + lib_dir, "-ldrt_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"]
    exe = tmp_path / "denoise_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)] + link + ["-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip() == "32"
    cli = tmp_path / "drt_render"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "drt_render.cpp")]
                       + link + ["-o", str(cli)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(cli), "--denoise"], capture_output=True, text=True)         # the flag alone: usage, exit code 2
    assert r.returncode == 2 and "--denoise" in r.stderr
