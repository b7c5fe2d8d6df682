"""The upscaling entry points of include/drt.h without a GPU: exported, bound, laid out as declared, defaults, argument checks that
come before any device work, the header states the rule and what is out of scope, and the C++ wrapper and the CLI compile against
them."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.scenes import ROOT

drt = pytest.importorskip("dustraytracer_amd")

NEW = ["drt_default_upscale_params", "drt_renderer_upscale", "drt_renderer_read_upscaled_rgba32f", "drt_renderer_device_upscaled",
       "drt_debug_upscale"]
FIELDS = [("source", 0), ("demodulate", 4), ("sigma_normal", 8), ("sigma_depth", 12), ("sigma_albedo", 16), ("albedo_floor", 20)]


def test_the_new_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(drt.LIB_PATH)
    assert all(hasattr(lib, n) for n in NEW)
    assert all(getattr(drt._lib, n).argtypes is not None for n in NEW)
    for name in ("Upscale", "GetUpscaledImage", "DeviceUpscaledTarget"):
        assert callable(getattr(drt.Renderer, name))
    assert callable(drt.debug_upscale)
    assert drt._lib.drt_abi_version() == 2


def test_pod_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "drt.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(drt_upscale_params), offsetof(drt_upscale_params, source), offsetof(drt_upscale_params, demodulate),
           offsetof(drt_upscale_params, sigma_normal), offsetof(drt_upscale_params, sigma_depth), offsetof(drt_upscale_params, sigma_albedo),
           offsetof(drt_upscale_params, albedo_floor));
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["24"] + [str(o) for _, o in FIELDS]
    assert ctypes.sizeof(drt.UpscaleParams) == 24
    assert [(n, getattr(drt.UpscaleParams, n).offset) for n, _ in drt.UpscaleParams._fields_] == FIELDS


def test_default_parameters():
    raw = drt.UpscaleParams.from_buffer_copy(bytes([0xFF]) * 24)
    drt._lib.drt_default_upscale_params(ctypes.byref(raw))
    assert (raw.source, raw.demodulate) == (0, 0)                # (demodulate 0: drt.h says why)
    assert [np.float32(getattr(raw, k)) for k in ("sigma_normal", "sigma_depth", "sigma_albedo", "albedo_floor")] == \
        [np.float32(0.1), np.float32(0.05), np.float32(0.1), np.float32(0.01)]
    d = drt.DenoiseParams()
    assert (np.float32(raw.sigma_normal), np.float32(raw.sigma_albedo)) == (np.float32(d.sigma_normal), np.float32(d.sigma_albedo))
    drt._lib.drt_default_upscale_params(None)                  # a NULL destination is ignored
    p = drt.UpscaleParams(source=1, sigma_depth=0.25)
    assert (p.source, p.demodulate, p.sigma_depth) == (1, 0, 0.25)
    with pytest.raises(TypeError):
        drt.UpscaleParams(sigma_color=1.0)


def test_null_handles_and_bad_arguments_are_invalid_without_a_gpu():
    L = drt._lib
    cam = drt.Camera()._pod()
    p = drt.UpscaleParams()
    ms = ctypes.c_float(7.0)
    buf = np.zeros(4, np.float32)
    assert L.drt_renderer_upscale(None, ctypes.byref(cam), None, 4, 4, ctypes.byref(p), ctypes.byref(ms)) == drt.ERR_INVALID
    assert ms.value == 0.0
    assert L.drt_renderer_upscale(None, None, None, 0, 0, None, None) == drt.ERR_INVALID
    assert b"null" in L.drt_last_error()
    assert L.drt_renderer_read_upscaled_rgba32f(None, buf.ctypes.data, 4) == drt.ERR_INVALID
    assert L.drt_renderer_device_upscaled(None) is None
    # the kernel-only entry checks its arguments before it touches a device
    c, g = np.zeros((1, 1, 4), np.float32), np.zeros((1, 1, 8), np.float32)
    ok = (0, c.ctypes.data, g.ctypes.data, g.ctypes.data, 1, 1, 1, 1, ctypes.byref(p), buf.ctypes.data)
    for i in (1, 2, 3, 8, 9):
        assert L.drt_debug_upscale(*(ok[:i] + (None,) + ok[i + 1:])) == drt.ERR_INVALID, i
    for sizes in ((0, 1, 1, 1), (1, 0, 1, 1), (2, 1, 1, 1), (1, 2, 1, 1), (1, 1, 1 << 16, (1 << 15) + 1)):
        assert L.drt_debug_upscale(*(ok[:4] + sizes + ok[8:])) == drt.ERR_INVALID, sizes
    for bad in (dict(source=2), dict(source=-1), dict(demodulate=2), dict(demodulate=-1), dict(sigma_normal=0.0), dict(sigma_depth=-1.0),
                dict(sigma_albedo=float("nan")), dict(albedo_floor=float("inf")), dict(albedo_floor=0.0)):
        q = drt.UpscaleParams(**bad)
        assert L.drt_debug_upscale(*(ok[:8] + (ctypes.byref(q),) + ok[9:])) == drt.ERR_INVALID, bad


def test_the_header_states_the_rule_and_what_is_out_of_scope():
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    sec = text[text.index("guide-driven upscaling"):text.index("drt_debug_upscale(int32_t device")]
    flat = re.sub(r"\s*\n \*\s*", " ", sec)
    for phrase in ("fx = ((float)X * (float)W) / (float)Wo", "(gl.prim(q) < 0) == (gh.prim(P) < 0)", "e <= 16", "w = b * expf(-e)",
                   "dz = (gl.t(q) - gh.t(P)) * (1 / (sigma_depth * gh.t(P)))", "fmaxf(gl.albedo(q), albedo_floor)", "dy = -1..2",
                   "the first tap wins a tie", "a NaN e never wins", "(wx1 > 0.5f)", "fmaxf(gh.albedo(P), albedo_floor)",
                   "drt_renderer_render_guides returns on a renderer resized to Wo x Ho", "one rounding per operation"):
        assert phrase in flat, phrase
    scope = flat[flat.index("Out of scope:"):]
    for phrase in ("temporal accumulation at output resolution", "jitter-aware sample reuse", "drt_group", "sharded renderers"):
        assert phrase in scope, phrase
    for code, what in (("DRT_ERR_INVALID", "source == 1 before any denoise call"), ("DRT_ERR_UNSUPPORTED", "a sharded renderer (world > 1)")):
        assert what in flat[flat.index(code + ":"):], what


def test_cpp_wrapper_and_cli_compile(tmp_path):
    src = tmp_path / "upscale_calls.cpp"
    src.write_text(r"""
#include <cstdio>
#include <vector>
#include "DustRayTracer.hpp"
// the editor's per-frame loop at a quarter of the pixels (INTEGRATION.md): the statements only -- main() runs none of them without arguments
int main(int argc, char **) {
    if (argc < 2) { std::printf("%zu\n", sizeof(drt_upscale_params)); return 0; }
    Scene scene;
    Camera cam;
    Renderer r(0);
    r.ResizeBuffer(8, 8);
    float ms = 0;
    r.Render(&cam, scene, &ms);
    r.TemporalDenoise(&cam, scene, &ms);
    r.Upscale(&cam, scene, 16, 16, &ms);
    drt_upscale_params p;
    drt_default_upscale_params(&p);
    p.source = 1;
    r.Upscale(&cam, scene, 16, 16, &ms, &p);
    std::vector<float> img(16 * 16 * 4);
    r.ReadUpscaledTarget(img.data());
    return r.DeviceUpscaledTarget() != nullptr && r.m_UpscaledWidth == 16;
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    link = ["-L" + lib_dir, "-ldrt_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"]
    exe = tmp_path / "upscale_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)] + link + ["-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip() == "24"
    cli = tmp_path / "drt_render"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "drt_render.cpp")]
                       + link + ["-o", str(cli)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for flags in (["--upscale", "96", "64"], ["a.glb", "b.pfm", "4", "4", "1", "1", "--upscale", "0", "64"]):      # the flag alone, a zero size: usage, exit code 2
        r = subprocess.run([str(cli)] + flags, capture_output=True, text=True)
        assert r.returncode == 2 and "[--upscale OW OH] [--temporal K] [--denoise]" in r.stderr
