"""The motion entry points of include/drt.h without a GPU: exported, bound, argument checks that come before any device work, the
ABI version, and the C++ wrapper compiles against them."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests.scenes import ROOT

drt = pytest.importorskip("dustraytracer_amd")

NEW = ["drt_renderer_track_motion", "drt_renderer_motion_advance", "drt_renderer_motion_vectors"]


def test_the_new_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(drt.LIB_PATH)
    assert all(hasattr(lib, n) for n in NEW)
    src = open(os.path.join(ROOT, "dustraytracer_amd", "__init__.py")).read()
    assert all(n in src for n in NEW)
    for name in ("trackMotion", "advanceMotion", "motionVectors"):
        assert callable(getattr(drt.Renderer, name))
    assert drt._lib.drt_abi_version() == 2


def test_null_handles_are_invalid_without_a_gpu():
    L = drt._lib
    cam = drt.Camera()._pod()
    buf = np.zeros(4, np.float32)
    assert L.drt_renderer_track_motion(None, 1) == drt.ERR_INVALID
    assert L.drt_renderer_track_motion(None, 0) == drt.ERR_INVALID
    assert L.drt_renderer_motion_advance(None) == drt.ERR_INVALID
    assert L.drt_renderer_motion_vectors(None, ctypes.byref(cam), ctypes.byref(cam), None, buf.ctypes.data, None) == drt.ERR_INVALID
    assert L.drt_renderer_motion_vectors(None, None, None, None, None, None) == drt.ERR_INVALID
    assert b"null" in L.drt_last_error()


def test_the_header_states_the_rule_and_what_stays_out_of_scope():
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    for phrase in ("den = d11 * d22 - d12 * d12", "P' = (v0' + e1' * b1) + e2' * b2", "n' = dot(fn, g.normal(p)) < 0 ? -fn' : fn'",
                   "motion through a host-side"):
        assert phrase in text, phrase
    assert "the caller resets the history or accepts that" not in text       # the sentence the motion rule made untrue


def test_cpp_wrapper_compiles(tmp_path):
    src = tmp_path / "motion_calls.cpp"
    src.write_text(r"""
#include <cstdio>
#include "DustRayTracer.hpp"
// an interactive loop with moving geometry: the statements only -- main() runs none of them without arguments
int main(int argc, char **) {
    if (argc < 2) { std::printf("ok\n"); return 0; }
    Scene scene;
    Camera cam, prev;
    Renderer r(0);
    r.ResizeBuffer(8, 8);
    r.TrackMotion();
    float ms = 0;
    const float *positions = nullptr;
    float *mv = nullptr;
    r.Refit(scene, positions);
    r.Render(&cam, scene, &ms);
    r.MotionVectors(&cam, scene, mv, &prev);
    r.MotionVectors(&cam, scene, mv);
    r.TemporalDenoise(&cam, scene, &ms);
    r.AdvanceMotion();
    r.TrackMotion(false);
    return 0;
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    link = ["-L" + lib_dir, "-ldrt_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"]
    exe = tmp_path / "motion_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)] + link + ["-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip() == "ok"
