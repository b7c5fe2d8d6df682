"""The adaptive-sampling entry points of include/drt.h without a GPU: exported, bound, laid out as declared, defaults, the argument
checks that come before any device work, the header states the rule and what is out of scope, and the C++ wrapper and the CLI
compile against them."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.scenes import ROOT

drt = pytest.importorskip("dustraytracer_amd")

NEW = ["drt_default_adaptive_params", "drt_renderer_render_adaptive", "drt_renderer_adaptive_reset", "drt_renderer_read_adaptive",
       "drt_renderer_device_adaptive", "drt_debug_adaptive_plan", "drt_debug_adaptive_weights"]
FIELDS = [("budget", 0), ("min_spp", 4), ("max_spp", 8), ("target_error", 12), ("luma_floor", 16)]
INFO = [("samples", 0), ("active_pixels", 4), ("max_count", 8), ("ms", 12)]


def test_the_new_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(drt.LIB_PATH)
    assert all(hasattr(lib, n) for n in NEW)
    assert all(getattr(drt._lib, n).argtypes is not None for n in NEW)
    for name in ("RenderAdaptive", "GetAdaptiveState", "DeviceAdaptiveState", "resetAdaptive"):
        assert callable(getattr(drt.Renderer, name))
    assert callable(drt.debug_adaptive_plan) and callable(drt.debug_adaptive_weights)
    assert drt.AdaptiveState._fields == ("sum", "count", "m1", "m2", "last_q", "last_count")
    assert drt._lib.drt_abi_version() == 2


def test_pod_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "drt.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(drt_adaptive_params), offsetof(drt_adaptive_params, budget), offsetof(drt_adaptive_params, min_spp),
           offsetof(drt_adaptive_params, max_spp), offsetof(drt_adaptive_params, target_error), offsetof(drt_adaptive_params, luma_floor));
    printf("%zu %zu %zu %zu %zu\n", sizeof(drt_adaptive_info), offsetof(drt_adaptive_info, samples), offsetof(drt_adaptive_info, active_pixels),
           offsetof(drt_adaptive_info, max_count), offsetof(drt_adaptive_info, ms));
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["20"] + [str(o) for _, o in FIELDS] + ["16"] + [str(o) for _, o in INFO]
    assert ctypes.sizeof(drt.AdaptiveParams) == 20 and ctypes.sizeof(drt.AdaptiveInfo) == 16
    assert [(n, getattr(drt.AdaptiveParams, n).offset) for n, _ in drt.AdaptiveParams._fields_] == FIELDS
    assert [(n, getattr(drt.AdaptiveInfo, n).offset) for n, _ in drt.AdaptiveInfo._fields_] == INFO


def test_default_parameters():
    raw = drt.AdaptiveParams.from_buffer_copy(bytes([0xFF]) * 20)
    drt._lib.drt_default_adaptive_params(ctypes.byref(raw))
    assert (raw.budget, raw.min_spp, raw.max_spp) == (0, 1, 64)
    assert (np.float32(raw.target_error), np.float32(raw.luma_floor)) == (np.float32(0), np.float32(0.01))
    drt._lib.drt_default_adaptive_params(None)                 # a NULL destination is ignored
    p = drt.AdaptiveParams(max_spp=8, target_error=0.5)
    assert (p.budget, p.min_spp, p.max_spp, p.target_error) == (0, 1, 8, 0.5)
    with pytest.raises(TypeError):
        drt.AdaptiveParams(spp=4)


def test_null_handles_and_bad_arguments_are_invalid_without_a_gpu():
    L = drt._lib
    cam = drt.Camera()._pod()
    p = drt.AdaptiveParams()
    info = drt.AdaptiveInfo(7, 7, 7, 7.0)
    buf = np.zeros(4, np.float32)
    assert L.drt_renderer_render_adaptive(None, ctypes.byref(cam), None, ctypes.byref(p), ctypes.byref(info)) == drt.ERR_INVALID
    assert (info.samples, info.active_pixels, info.max_count, info.ms) == (0, 0, 0, 0.0)
    assert L.drt_renderer_render_adaptive(None, None, None, None, None) == drt.ERR_INVALID
    assert b"null" in L.drt_last_error()
    assert L.drt_renderer_adaptive_reset(None) == drt.ERR_INVALID
    assert L.drt_renderer_read_adaptive(None, 0, buf.ctypes.data, 16) == drt.ERR_INVALID
    assert L.drt_renderer_device_adaptive(None, 0) is None
    # the plan-only entry checks its arguments before it touches a device
    q, c, o = np.zeros(4, np.uint32), np.zeros(4, np.uint32), np.zeros(4, np.uint32)
    ok = (0, q.ctypes.data, 4, ctypes.byref(p), 0, c.ctypes.data, o.ctypes.data, None)
    for i in (1, 3, 5, 6):
        assert L.drt_debug_adaptive_plan(*(ok[:i] + (None,) + ok[i + 1:])) == drt.ERR_INVALID, i
    assert L.drt_debug_adaptive_plan(*(ok[:2] + (0,) + ok[3:])) == drt.ERR_INVALID                   # no pixels
    for bad in (dict(min_spp=3, max_spp=2), dict(min_spp=0, max_spp=0), dict(budget=3), dict(budget=1 << 31), dict(budget=(1 << 32) - 1),
                dict(min_spp=5, budget=19), dict(target_error=-1.0), dict(target_error=float("nan")), dict(target_error=float("inf")),
                dict(luma_floor=0.0), dict(luma_floor=-0.01), dict(luma_floor=float("nan")), dict(luma_floor=float("inf"))):
        b = drt.AdaptiveParams(**bad)
        assert L.drt_debug_adaptive_plan(*(ok[:3] + (ctypes.byref(b),) + ok[4:])) == drt.ERR_INVALID, bad
    big = np.zeros(1, np.uint32)                                # budget 0 = 4 per pixel: 2^29 pixels would make it 2^31
    assert L.drt_debug_adaptive_plan(0, big.ctypes.data, 1 << 29, ctypes.byref(p), 0, big.ctypes.data, big.ctypes.data, None) == drt.ERR_INVALID
    # so does the weights-only entry (Q and active are optional)
    s0, s1 = np.zeros((4, 4), np.float32), np.zeros((4, 4), np.float32)
    ok = (0, s0.ctypes.data, s1.ctypes.data, 4, ctypes.byref(p), q.ctypes.data, None, None)
    for i in (1, 2, 4, 5):
        assert L.drt_debug_adaptive_weights(*(ok[:i] + (None,) + ok[i + 1:])) == drt.ERR_INVALID, i
    assert b"null" in L.drt_last_error()
    assert L.drt_debug_adaptive_weights(*(ok[:3] + (0,) + ok[4:])) == drt.ERR_INVALID                # no pixels
    for bad in (dict(min_spp=3, max_spp=2), dict(min_spp=0, max_spp=0), dict(budget=3), dict(budget=1 << 31), dict(min_spp=5, budget=19),
                dict(target_error=-1.0), dict(target_error=float("nan")), dict(target_error=float("inf")), dict(luma_floor=0.0),
                dict(luma_floor=-0.01), dict(luma_floor=float("nan")), dict(luma_floor=float("inf"))):
        b = drt.AdaptiveParams(**bad)
        assert L.drt_debug_adaptive_weights(*(ok[:4] + (ctypes.byref(b),) + ok[5:])) == drt.ERR_INVALID, bad
    assert L.drt_debug_adaptive_weights(0, s0.ctypes.data, s1.ctypes.data, 1 << 29, ctypes.byref(p), q.ctypes.data, None, None) == drt.ERR_INVALID


def test_the_header_states_the_rule_and_what_is_out_of_scope():
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    sec = text[text.index("adaptive sampling: spend each call's samples"):text.index("typedef struct drt_adaptive_params")]
    flat = re.sub(r"\s*\n \*\s*", " ", sec)
    for phrase in ("q = 16777215", "mean = m1 / n", "var = fmaxf(m2 / n - mean * mean, 0)", "w = sqrtf(var / n) / (mean + luma_floor)",
                   "s = w * 65536.0f", "q = s < 16777215.0f ? (uint32)s : 16777215", "extra = budget - min_spp * pixels",
                   "min(max_spp, min_spp + (uint32)((uint64)extra * q / Q))", "min(max_spp, min_spp + extra / pixels)", "is not redistributed",
                   "seed = (x + y * width) * (n + k)", "sum / (float)n", "(0, 0, 0, 1) where n == 0", "one rounding per operation",
                   "A later drt_renderer_render overwrites the framebuffer", "drt_renderer_reset"):
        assert phrase in flat, phrase
    scope = flat[flat.index("Out of scope:"):]
    for phrase in ("frame loop's own kernels", "drt_group", "sharded renderers", "temporal filter's variance", "redistributing", "linear"):
        assert phrase in scope, phrase
    for code, what in (("DRT_ERR_INVALID", "a read before the first call"), ("DRT_ERR_UNSUPPORTED", "a sharded renderer (world > 1)"),
                       ("DRT_ERR_UNSUPPORTED", "render_mode DEBUGMODE"), ("DRT_ERR_UNSUPPORTED", "a tree deeper than 64 levels")):
        assert what in flat[flat.index(code + ":"):], what
    assert "adaptive-sampling entry points" in text[:text.index("#define DRT_ABI_VERSION 2")]


def test_cpp_wrapper_and_cli_compile(tmp_path):
    src = tmp_path / "adaptive_calls.cpp"
    src.write_text(r"""
#include <cstdio>
#include <vector>
#include "DustRayTracer.hpp"
// the statements only -- main() runs none of them without arguments
int main(int argc, char **) {
    if (argc < 2) { std::printf("%zu %zu\n", sizeof(drt_adaptive_params), sizeof(drt_adaptive_info)); return 0; }
    Scene scene;
    Camera cam;
    Renderer r(0);
    r.ResizeBuffer(8, 8);
    drt_adaptive_info info = r.RenderAdaptive(&cam, scene);
    drt_adaptive_params p;
    drt_default_adaptive_params(&p);
    p.budget = 8 * 8 * 2; p.target_error = 0.01f;
    info = r.RenderAdaptive(&cam, scene, &p);
    std::vector<float> st(8 * 8 * 4);
    r.ReadAdaptiveState(0, st.data());
    r.ResetAdaptive();
    return info.active_pixels == 0;
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    link = ["-L" + lib_dir, "-ldrt_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"]
    exe = tmp_path / "adaptive_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)] + link + ["-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["20", "16"]
    cli = tmp_path / "drt_render"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "drt_render.cpp")]
                       + link + ["-o", str(cli)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    base = ["a.glb", "b.pfm", "4", "4", "1", "1"]
    for flags in (["--adaptive", "4"], base + ["--adaptive", "0"], base + ["--adaptive", "4", "--adaptive-calls", "0"],
                  base + ["--adaptive", "4", "--target-error", "-1"], base + ["--target-error", "0.1"], base + ["--adaptive-calls", "2"]):
        r = subprocess.run([str(cli)] + flags, capture_output=True, text=True)
        assert r.returncode == 2 and "[--adaptive SPP [--target-error E] [--adaptive-calls K]] [--upscale OW OH]" in r.stderr, flags
