"""The winding-number entry points of include/drt.h without a GPU: exported, bound, every argument check that comes before any device
work, the header states the rule with the restatement's constants digit for digit and says what it is not, drt_renderer_inside still
refuses other rules, and the C++ wrapper compiles and links."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import winding_ref as wr
from tests.scenes import ROOT, scene_path

drt = pytest.importorskip("dustraytracer_amd")

ENTRY_POINTS = ("drt_renderer_winding_numbers", "drt_renderer_winding_inside", "drt_renderer_winding_signed_distance")


def test_the_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(drt.LIB_PATH)
    P, U, Fl = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float
    for name in ENTRY_POINTS + ("drt_debug_winding_moments",):
        assert hasattr(lib, name), name
    assert list(drt._lib.drt_renderer_winding_numbers.argtypes) == [P, P, P, U, Fl, P, P]
    assert list(drt._lib.drt_renderer_winding_inside.argtypes) == [P, P, P, U, Fl, Fl, P, P]
    assert list(drt._lib.drt_renderer_winding_signed_distance.argtypes) == [P, P, P, U, Fl, Fl, P, P]
    for name in ("windingNumbers", "windingInside", "windingSignedDistance", "windingGrid"):
        assert callable(getattr(drt.Renderer, name)), name
    doc = " ".join(drt.Renderer.windingNumbers.__doc__.split())
    for phrase in ("first order only", "a point on the surface has no defined answer", "orientation is still assumed per connected patch",
                   "no RendererGroup and no command line", "beta=inf is the exact sum"):
        assert phrase in doc, phrase
    assert drt._lib.drt_abi_version() == 2


def test_null_handles_and_a_bad_beta_are_refused_before_any_device_work():
    L = drt._lib
    built = drt.Scene()
    built.loadGLTFmodel(scene_path("cornell_box"))
    b = drt.BVHBuilder()
    b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
    b.buildIterative(built)
    stand_in = ctypes.create_string_buffer(1 << 16)              # a block of zeros stands in for the renderer: it is not looked at yet
    h = ctypes.addressof(stand_in)
    pts = ctypes.create_string_buffer(16 * 4 + 16)
    P = (ctypes.addressof(pts) + 15) & ~15
    out = ctypes.create_string_buffer(32 * 4 + 16)
    O = (ctypes.addressof(out) + 15) & ~15
    calls = {"numbers": (lambda r, s, p, n, beta, o: L.drt_renderer_winding_numbers(r, s, p, n, beta, o, None), 4),
             "inside": (lambda r, s, p, n, beta, o: L.drt_renderer_winding_inside(r, s, p, n, beta, 0.5, o, None), 0),
             "signed_distance": (lambda r, s, p, n, beta, o: L.drt_renderer_winding_signed_distance(r, s, p, n, beta, 0.5, o, None), 16)}
    for what, (fn, align) in calls.items():
        for args in ((None, built._h, P, 4, 2.0, O), (h, None, P, 4, 2.0, O), (None, None, None, 0, 2.0, None)):
            assert fn(*args) == drt.ERR_INVALID and b"null argument" in L.drt_last_error(), what
        for beta in (-1.0, -1e-30, float("nan"), -float("inf")):
            assert fn(h, built._h, P, 4, beta, O) == drt.ERR_INVALID and b"beta" in L.drt_last_error(), (what, beta)
            assert fn(h, built._h, None, 0, beta, None) == drt.ERR_INVALID, (what, beta)                  # also with n == 0
        for beta in (0.0, 2.0, float("inf")):
            assert fn(h, built._h, None, 0, beta, None) == drt.OK, (what, beta)                           # n == 0: nothing to do
        for name, p, o in (("null points", None, O), ("null out", P, None)):
            assert fn(h, built._h, p, 4, 2.0, o) == drt.ERR_INVALID and b"null point or result" in L.drt_last_error(), (what, name)
        assert fn(h, built._h, P + 4, 4, 2.0, O) == drt.ERR_INVALID and b"aligned" in L.drt_last_error(), what
        if align:
            assert fn(h, built._h, P, 4, 2.0, O + align // 2) == drt.ERR_INVALID and b"aligned" in L.drt_last_error(), what
        assert fn(h, built._h, P, 0x80000000, 2.0, O) == drt.ERR_INVALID and b"2^31" in L.drt_last_error(), what
        # all of them passed: only now the renderer is looked at (zeros: no batch pending) and the device asked for -- host memory or
        # no device, either way the call fails after the checks
        assert fn(h, built._h, P, 4, 2.0, O) in (drt.ERR_INVALID, drt.ERR_DEVICE), what
        assert b"device" in L.drt_last_error().lower() or b"hip" in L.drt_last_error().lower()
    count = ctypes.c_uint32(0)
    assert L.drt_debug_winding_moments(None, built._h, None, 0, ctypes.byref(count)) == drt.ERR_INVALID
    assert L.drt_debug_winding_moments(h, built._h, None, 0, None) == drt.ERR_INVALID


def test_bad_arguments_are_refused_by_the_python_interface_before_any_device_work():
    r = drt.Renderer.__new__(drt.Renderer)                                     # (no device: only the argument check runs)
    r._device = 0
    sc = drt.Scene()
    p = np.zeros((3, 3), np.float32)
    for call in (lambda: r.windingNumbers(sc, p, beta=-1), lambda: r.windingNumbers(sc, p, beta=float("nan")),
                 lambda: r.windingInside(sc, p, beta=-0.5), lambda: r.windingSignedDistance(sc, p, beta="x"),
                 lambda: r.windingGrid(sc, 4, (0, 0, 0), (1, 1, 1), beta=-2), lambda: r.windingSignedDistance(sc, p, 1.0, -1.0)):
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == drt.ERR_INVALID and "beta" in str(e.value)


def test_inside_still_refuses_a_rule_other_than_parity_and_winding():
    stand_in = ctypes.create_string_buffer(1 << 16)
    h = ctypes.addressof(stand_in)
    sc = drt.Scene()
    for rule in (2, 3, -1):
        assert drt._lib.drt_renderer_inside(h, sc._h, None, None, 0, rule, None) == drt.ERR_INVALID and b"rule" in drt._lib.drt_last_error()
        assert drt._lib.drt_renderer_signed_distance(h, sc._h, None, None, 0, rule, None) == drt.ERR_INVALID
    assert sorted(drt.INSIDE_RULES) == ["parity", "winding"]


def _flat(text):
    return re.sub(r" +", " ", re.sub(r"\s*\n \*\s*", " ", text))


def test_the_header_states_the_rule_and_what_it_is_not():
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    sec = text[text.index("generalised winding numbers (new"):text.index("typedef struct drt_winding_moment")]
    flat = _flat(sec)
    for phrase in ("fp32 with one rounding per operation, in the order written", "a = v0 - q, b = a + e1, c = a + e2",
                   "det = dot(a, cross(e1, e2))", "not the stored face normal",
                   "den = |a| * |b| * |c| + dot(a, b) * |c| + dot(b, c) * |a| + dot(c, a) * |b|", "omega = 2.0f * atan2(det, den), in steradians",
                   "A triangle with det == 0 contributes exactly 0", "atan2(0, x) is never evaluated", "the library's atan2f is not used",
                   "one division and a fixed polynomial", "swap = ay > ax; mx = swap ? ay : ax; mn = swap ? ax : ay",
                   "t = big ? (mn - mx) / (mn + mx) : mn / mx; s = t * t", "drt_winding_moment {N[3], r2, p[3], pad}, pad = 0",
                   "n_t = 0.5f * cross(e1, e2), area_t = |n_t|, c_t = v0 + (e1 + e2) / 3.0f", "in ascending tree index",
                   "A parent is child 1 + child 2, in that order, for N, A and S", "p = 0.5f * (lo + hi)",
                   "the child box in the parent's record, or the root box", "the squared distance from p to the farthest corner",
                   "the same bytes whatever computes it", "by the first winding call after an upload or a drt_renderer_refit",
                   "child 1 before child 2", "never holds more entries than the tree has levels", "One fp32 accumulator, in steradians",
                   "iff dd > (beta * beta) * r2", "accumulator += dot(d, N) / (dd * sqrtf(dd))", "a leaf adds omega of its triangles in ascending index",
                   "the 1 / (4 pi) is applied once, at the end", "beta = +inf never approximates", "inf * 0 is a NaN and the comparison fails",
                   "beta = 0 answers with the root's dipole alone", "beta = 2 is the default", "answers NaN without walking",
                   "an empty scene answers 0", "Alpha cut-outs are ignored", "w >= threshold ? 1 : 0", "w >= threshold ? -1 : +1",
                   "the first seven words are unchanged", "no floating-point atomics and no sums across lanes",
                   "a negative or NaN beta", "DRT_ERR_UNSUPPORTED for trees deeper than 64 levels", "counters, kernel info and kernel span are not touched"):
        assert phrase in flat, phrase
    limits = flat[flat.index("What this is not:"):]
    for phrase in ("first order only", "a point on the surface has no defined answer", "orientation is still assumed per connected patch",
                   "no drt_group_* form and no command line", "drt_renderer_inside's rules stay 0 and 1"):
        assert phrase in limits, phrase
    before = _flat(text[:text.index("#define DRT_ABI_VERSION 2")])
    assert "the winding-number entry points (drt_renderer_winding_numbers / _winding_inside / _winding_signed_distance)" in before
    # the crossings block is left as it was
    crossings = _flat(text[text.index("crossing counts, inside / outside and signed distance (new"):text.index("typedef struct drt_crossings")])
    assert "Angle-weighted pseudonormals and generalised winding numbers for open meshes are out of scope" in crossings


def test_the_constants_are_the_restatements_digit_for_digit():
    header = _flat(open(os.path.join(ROOT, "include", "drt.h")).read())
    kernel = open(os.path.join(ROOT, "dustraytracer_amd", "csrc", "winding.hpp")).read()
    evaluate = open(os.path.join(ROOT, "dustraytracer_amd", "csrc", "kernel_winding.hip")).read()
    c = wr.ATAN_COEFFS
    poly = "(((%sf * s - %sf) * s + %sf) * s - %sf) * s * t + t" % c
    assert poly in header and poly in kernel
    for text in (header, kernel):
        for lit in (wr.TAN_PI_8, wr.PI_4, wr.PI_2, wr.PI):
            assert lit + "f" in text, lit
    assert "big = mn > %sf * mx" % wr.TAN_PI_8 in header and "r = %sf + r" % wr.PI_4 in header
    assert "r = %sf - r" % wr.PI_2 in header and "r = %sf - r" % wr.PI in header
    assert "w = accumulator * %sf" % wr.INV_4PI in header and "acc * %sf" % wr.INV_4PI in evaluate
    # and they are what they claim to be, to the last place of fp32
    assert np.float32(wr.TAN_PI_8) == np.float32(np.tan(np.pi / 8)) and np.float32(wr.PI_4) == np.float32(np.pi / 4)
    assert np.float32(wr.PI_2) == np.float32(np.pi / 2) and np.float32(wr.PI) == np.float32(np.pi)
    assert np.float32(wr.INV_4PI) == np.float32(1 / (4 * np.pi))


def test_cpp_wrapper_compiles_and_links(tmp_path):
    src = tmp_path / "winding_calls.cpp"
    src.write_text(r"""
#include <cstdio>
#include "DustRayTracer.hpp"
// the statements only -- main() runs none of them without arguments
int main(int argc, char **) {
    if (argc < 2) { std::printf("%zu %zu %d\n", sizeof(drt_winding_moment), sizeof(drt_point), DRT_ABI_VERSION); return 0; }
    Scene scene;
    Renderer r(0);
    const drt_point *points = nullptr;
    float *w = nullptr;
    uint8_t *flags = nullptr;
    drt_nearest *near = nullptr;
    r.WindingNumbers(scene, points, w, 0u);
    r.WindingNumbers(scene, points, w, 0u, 3.0f, nullptr);
    r.WindingInside(scene, points, flags, 0u);
    r.WindingInside(scene, points, flags, 0u, 2.0f, 0.25f, nullptr);
    r.WindingSignedDistance(scene, points, near, 0u);
    r.WindingSignedDistance(scene, points, near, 0u, 2.0f, 0.5f, nullptr);
    return 0;
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    exe = tmp_path / "winding_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib_dir, "-ldrt_hip",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["32", "16", "2"]
