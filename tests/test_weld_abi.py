"""The welding entry points of include/drt.h without a GPU: exported, bound, every argument check that comes before any device work,
the header states the three rules and says what they are not, the Python wrappers refuse bad arguments, the kernel's constants are the
header's, and the C++ wrappers compile and link."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.scenes import ROOT

drt = pytest.importorskip("dustraytracer_amd")

NAN = float("nan")


def test_the_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(drt.LIB_PATH)
    P, U, I = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32
    for name in ("drt_renderer_weld", "drt_renderer_vertex_normals", "drt_renderer_smooth_vertices"):
        assert hasattr(lib, name), name
    assert list(drt._lib.drt_renderer_weld.argtypes) == [P, P, U, U, P, P, P, U, P, P]
    assert list(drt._lib.drt_renderer_vertex_normals.argtypes) == [P, P, U, P, U, I, P, P]
    assert list(drt._lib.drt_renderer_smooth_vertices.argtypes) == [P, P, U, P, U, P, U, P, P, P]
    for name in ("weld", "vertexNormals", "smooth"):
        assert callable(getattr(drt.Renderer, name)), name
    for name in ("triangles", "toScene"):
        assert callable(getattr(drt.IndexedMesh, name)), name
    assert drt.IndexedMesh._fields == ("vertices", "faces", "first") and drt.NORMAL_WEIGHTS == {"angle": 0, "area": 1}
    doc = " ".join((drt.Renderer.weld.__doc__ + drt.Renderer.smooth.__doc__).split())
    for phrase in ("no tolerance", "no cotangent weights", "no feature preservation", "no boundary detection", "no simplification",
                   "no vertex-to-triangle lists", "no device edge adjacency from faces", "no RendererGroup and no command line"):
        assert phrase in doc, phrase
    assert drt._lib.drt_abi_version() == 2


def _stand_ins():
    stand_in = ctypes.create_string_buffer(1 << 16)              # a block of zeros stands in for the renderer: it is not looked at yet
    pending = ctypes.create_string_buffer(b"\x01" * (1 << 16), 1 << 16)      # every flag of the stand-in true: a batch is pending
    buf = ctypes.create_string_buffer(1 << 14)
    return stand_in, pending, buf, (ctypes.addressof(buf) + 15) & ~15


def _after_the_checks(L, rc):
    """all checks passed: only now the renderer is looked at and the device asked for -- host memory or no device, the call fails"""
    assert rc in (drt.ERR_INVALID, drt.ERR_DEVICE)
    assert b"device" in L.drt_last_error().lower() or b"hip" in L.drt_last_error().lower()


def test_weld_checks_return_their_error_code_with_no_launch():
    L = drt._lib
    stand_in, pending, buf, A = _stand_ins()
    h = ctypes.addressof(stand_in)
    T, FA, FI, VE, CNT = A, A + 1024, A + 2048, A + 3072, A + 4096

    def call(r=h, tris=T, n=4, stride=36, faces=FA, first=FI, vertices=VE, cap=12, count=CNT):
        return L.drt_renderer_weld(r, tris, n, stride, faces, first, vertices, cap, count, None)

    def refused(what, **kw):
        assert call(**kw) == drt.ERR_INVALID, kw
        assert what in L.drt_last_error(), (kw, L.drt_last_error())

    refused(b"null argument", r=None)
    refused(b"null argument", count=None)
    for stride in (0, 12, 35, 40, 44, 52, 96):
        refused(b"stride", stride=stride)
    refused(b"2^31", n=715827883)                                 # 3 n = 2^31 + 1
    refused(b"2^31", n=0xFFFFFFFF)
    assert call(n=715827882) != drt.ERR_INVALID or b"2^31" not in L.drt_last_error()      # 3 n = 2^31 - 2 passes this check
    refused(b"null tris or faces", tris=None)
    refused(b"null tris or faces", faces=None)
    refused(b"if and only if", first=None)
    refused(b"if and only if", cap=0)
    refused(b"vertices without first", first=None, cap=0)
    for name, base in (("tris", T), ("faces", FA), ("first", FI), ("vertices", VE), ("count", CNT)):
        refused(b"aligned", **{name: base + 2})
    # the order: an earlier check answers first
    refused(b"stride", stride=7, n=0xFFFFFFFF, tris=None)
    refused(b"2^31", n=0xFFFFFFFF, tris=None, first=None)
    refused(b"null tris", tris=None, first=None, count=CNT + 1)
    refused(b"if and only if", first=None, count=CNT + 1)
    for kw in ({}, dict(stride=48), dict(vertices=None), dict(first=None, vertices=None, cap=0), dict(n=0, tris=None, faces=None)):
        _after_the_checks(L, call(**kw))
    refused(b"pending", r=ctypes.addressof(pending))


def test_normals_and_smoothing_checks_return_their_error_code_with_no_launch():
    L = drt._lib
    stand_in, pending, buf, A = _stand_ins()
    h = ctypes.addressof(stand_in)
    VE, FA, OUT, FX = A, A + 1024, A + 2048, A + 3072
    fac = (ctypes.c_float * 4)(0.5, -0.53, 1.0, -1.0)

    def normals(r=h, vertices=VE, nv=8, faces=FA, nt=4, weight=0, out=OUT):
        return L.drt_renderer_vertex_normals(r, vertices, nv, faces, nt, weight, out, None)

    def smooth(r=h, vertices=VE, nv=8, faces=FA, nt=4, factors=fac, nf=4, fixed=FX, out=OUT):
        return L.drt_renderer_smooth_vertices(r, vertices, nv, faces, nt, factors, nf, fixed, out, None)

    def refused(call, what, **kw):
        assert call(**kw) == drt.ERR_INVALID, kw
        assert what in L.drt_last_error(), (kw, L.drt_last_error())

    refused(normals, b"null argument", r=None)
    for weight in (-1, 2, 7):
        refused(normals, b"weight", weight=weight)
    assert normals(nv=0, vertices=None, out=None) == 0            # no vertices: a no-op
    refused(smooth, b"null argument", r=None)
    refused(smooth, b"null factors", factors=None)
    for bad in (1.5, -1.0000001, NAN, float("inf")):
        refused(smooth, b"|f| <= 1", factors=(ctypes.c_float * 2)(0.5, bad), nf=2)
    assert smooth(nv=0, vertices=None, out=None) == 0
    for call in (normals, smooth):
        refused(call, b"null vertices or out", vertices=None)
        refused(call, b"null vertices or out", out=None)
        refused(call, b"null faces", faces=None)
        refused(call, b"aligned", vertices=VE + 2)
        refused(call, b"aligned", faces=FA + 1)
        refused(call, b"aligned", out=OUT + 3)
        refused(call, b"2^31", nt=715827883)
        refused(call, b"2^31", nv=0x80000000)
        _after_the_checks(L, call())
        _after_the_checks(L, call(nt=0, faces=None))
        refused(call, b"pending", r=ctypes.addressof(pending))
    # out may not alias the input of a smoothing call, whole or in part
    refused(smooth, b"alias", out=VE)
    refused(smooth, b"alias", out=VE + 92)                        # the last float of eight vertices
    refused(smooth, b"alias", vertices=OUT + 92)
    _after_the_checks(L, smooth(out=VE + 96))
    _after_the_checks(L, smooth(nf=0, factors=None))
    _after_the_checks(L, smooth(fixed=None))
    # the order
    refused(normals, b"weight", weight=3, vertices=None)
    refused(smooth, b"|f| <= 1", factors=(ctypes.c_float * 1)(2.0), nf=1, vertices=None)
    refused(smooth, b"null vertices", vertices=None, out=VE)
    refused(smooth, b"2^31", nt=715827883, out=VE)
    refused(smooth, b"alias", out=VE, r=ctypes.addressof(pending))


def test_bad_arguments_are_refused_by_the_python_interface_before_any_device_work():
    r = drt.Renderer.__new__(drt.Renderer)                                     # (no device: only the argument check runs)
    r._device = 0
    v, f = np.zeros((4, 3), np.float32), np.zeros((2, 3), np.int32)
    mesh = drt.IndexedMesh(v, f, None)
    cases = [(lambda: r.weld(np.zeros((2, 3, 3), np.float64)), "dtype"), (lambda: r.weld([[0.0] * 9]), "tris"),
             (lambda: r.weld(np.zeros((2, 9), np.float32)), "shape"), (lambda: r.weld(np.zeros((2, 3, 2), np.float32)), "shape"),
             (lambda: r.vertexNormals(mesh, weight="cotangent"), "weight"), (lambda: r.vertexNormals(mesh, weight=None), "weight"),
             (lambda: r.vertexNormals(5), "mesh"), (lambda: r.vertexNormals((v.astype(np.float64), f)), "vertices"),
             (lambda: r.vertexNormals((v, f.astype(np.int64))), "faces"), (lambda: r.vertexNormals((v, f.reshape(3, 2))), "faces"),
             (lambda: r.vertexNormals((v.reshape(3, 4), f)), "vertices"),
             (lambda: r.smooth(mesh, iterations=-1), "iterations"), (lambda: r.smooth(mesh, iterations=2.5), "iterations"),
             (lambda: r.smooth(mesh, iterations=True), "iterations"), (lambda: r.smooth(mesh, lam=1.5), "|f| <= 1"),
             (lambda: r.smooth(mesh, mu=NAN), "|f| <= 1"), (lambda: r.smooth(mesh, factors=[0.5, -2.0]), "|f| <= 1"),
             (lambda: r.smooth(mesh, factors=["x"]), "factors"), (lambda: r.smooth(mesh, factors=3), "factors")]
    for call, word in cases:
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == drt.ERR_INVALID and word in str(e.value), (word, str(e.value))


def test_an_indexed_mesh_gathers_triangles_and_makes_scenes():
    v = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]])
    f = np.int32([[0, 1, 2], [1, 3, 2]])
    mesh = drt.IndexedMesh(v, f, np.int32([0, 1, 2, 4]))
    t = mesh.triangles()
    assert t.shape == (2, 3, 3) and t.dtype == np.float32 and t[1].tolist() == [[1, 0, 0], [1, 1, 0], [0, 1, 0]]
    nrm = np.float32([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, -1]])
    for normals, want in ((None, np.tile(np.float32([0, 0, 1]), (2, 3, 1))), (nrm, nrm[f])):
        sc = mesh.toScene(normals=normals)
        prims = sc.m_PrimitivesBuffer                                         # (no BVH yet: load order)
        assert len(prims) == 2 and prims["vertex"]["position"].tolist() == t.tolist()
        assert prims["vertex"]["normal"].tolist() == want.tolist()
    with pytest.raises(drt.DrtError):
        mesh.toScene(normals=nrm[:3])


def _flat(text):
    return re.sub(r" +", " ", re.sub(r"\s*\n \*\s*", " ", text))


def test_the_header_states_the_rules_and_what_they_are_not():
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    flat = _flat(text[text.index("vertex welding, vertex normals and smoothing (new"):text.index("#define DRT_NORMALS_ANGLE")])
    for phrase in ("36 (float [N][3][3]) or 48", "3 n < 2^31", "Corner c = 3 t + k", "their three 32-bit words are equal as integers",
                   "-0.0 and +0.0 are different vertices", "NaNs are compared by their bits", "no tolerance and nothing is moved",
                   "rep[c] is the smallest corner index with c's position", "numbered in ascending rep, that is by first appearance",
                   "vertex_count, one device word that is always the total V", "3 n always suffices",
                   "faces and the count are still complete", "the same bytes on every run, in every launch shape",
                   "n = cross(v1 - v0, v2 - v0), l = sqrtf(dot(n, n))", "a bounds check, never a fault", "u = n / l, three divisions",
                   "a = v[(k+1) % 3] - v[k], b = v[(k+2) % 3] - v[k]", "angle = atan2(l, dot(a, b))", "x = +inf", "x = -inf gives 3.14159265f",
                   "a corner whose angle is not finite adds nothing", "(int64) trunc((double)(angle * u_j) * 2^28)",
                   "e = floor(log2 M)", "(int64) trunc((double)n_j * 2^(28 - e))", "M = 0 gives all zeros",
                   "x / sqrt(x x + y y + z z)", "|f| <= 1, else DRT_ERR_INVALID", "out may not alias vertices",
                   "k = 27 - e (M = 0: k = 0)", "q(x) = (int64) trunc((double)x * 2^k)", "adds q(p_b) + q(p_c) to acc[a]", "adds 2 to cnt of each",
                   "names a vertex twice is not special-cased", "m = (double)acc / ((double)cnt * 2^k)",
                   "p' = (float)((double)p + (double)f * (m - (double)p))", "if cnt = 0, if fixed is set for it, or if a coordinate of it is not finite",
                   "a smoothed watertight mesh is watertight by construction", "DRT_ERR_DEVICE"):
        assert phrase in flat, phrase
    limits = flat[flat.index("What this is not:"):]
    for phrase in ("no cotangent weights", "no feature preservation", "no boundary detection", "drt_renderer_boundary_loops",
                   "no simplification", "no vertex-to-triangle lists", "no device edge adjacency from faces", "no tolerance",
                   "no drt_group_* form and no command line"):
        assert phrase in limits, phrase
    assert "the welding entry points (drt_renderer_weld / _vertex_normals / _smooth_vertices)" in _flat(text[:text.index("#define DRT_ABI_VERSION 2")])
    assert re.search(r"#define DRT_NORMALS_ANGLE 0\s+#define DRT_NORMALS_AREA 1", text)


def test_the_kernel_follows_the_stated_design():
    src = open(os.path.join(ROOT, "dustraytracer_amd", "csrc", "kernel_weld.hip")).read()
    hpp = open(os.path.join(ROOT, "dustraytracer_amd", "csrc", "weld.hpp")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomicCAS(&a.table[slot], kWeldEmpty, c)" in code and "atomicMin(&a.table[slot], c)" in code and "pcg_hash" in code
    assert "wn_atan2(l, dot(ea, eb))" in code and "0x1p28" in code and "28 - weld_exponent" in code and "27 - weld_exponent" in code
    assert re.findall(r"atomicAdd\(([^,]*),", code) == ["reinterpret_cast<unsigned long long *>(p)", "&a.cnt[tri.i[k]]"]   # integer sums only
    assert "while (s < 2ull * corners) s <<= 1;" in hpp                       # a power of two, at least 2 * 3 N slots
    for word in ("while (true)", "while (1)", "for (;;)"):                    # no lane waits for another: every loop is bounded
        assert word not in code, word


def test_cpp_wrappers_compile_and_link(tmp_path):
    src = tmp_path / "weld_calls.cpp"
    src.write_text(r"""
#include <cstdio>
#include "DustRayTracer.hpp"
// the statements only -- main() runs none of them without arguments
int main(int argc, char **) {
    if (argc < 2) {
        std::printf("%d %d\n", DRT_NORMALS_ANGLE, DRT_NORMALS_AREA);
        return 0;
    }
    Renderer r(0);
    const drt_iso_tri *records = nullptr;
    const float *soup = nullptr, *vertices = nullptr;
    int32_t *faces = nullptr, *first = nullptr;
    float *positions = nullptr, *out = nullptr;
    uint32_t *count = nullptr;
    const uint8_t *fixed = nullptr;
    const float factors[] = {0.5f, -0.53f};
    r.Weld(records, 10u, (uint32_t)sizeof(drt_iso_tri), faces, first, positions, 30u, count);
    r.Weld(soup, 10u, 36u, faces, nullptr, nullptr, 0u, count, nullptr);
    r.VertexNormals(vertices, 8u, faces, 10u, out);
    r.VertexNormals(vertices, 8u, faces, 10u, out, DRT_NORMALS_AREA, nullptr);
    r.SmoothVertices(vertices, 8u, faces, 10u, factors, 2u, out);
    r.SmoothVertices(vertices, 8u, faces, 10u, factors, 2u, out, fixed, nullptr);
    return 0;
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    exe = tmp_path / "weld_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib_dir, "-ldrt_hip",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["0", "1"]
