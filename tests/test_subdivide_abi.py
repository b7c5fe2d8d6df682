"""The subdivision entry point of include/drt.h without a GPU: exported, bound, every argument check that comes before any device work
in the documented order, the header states the rule bit for bit and says what it is not, the Python wrapper refuses bad arguments, the
kernel follows the stated design, and the C++ wrapper compiles and links."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.scenes import ROOT

drt = pytest.importorskip("dustraytracer_amd")


def test_the_symbol_is_exported_and_bound():
    lib = ctypes.CDLL(drt.LIB_PATH)
    P, U, I32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32
    assert hasattr(lib, "drt_renderer_subdivide")
    assert list(drt._lib.drt_renderer_subdivide.argtypes) == [P, P, U, P, U, I32, P, P, U, P, P, P]
    assert drt._lib.drt_renderer_subdivide.restype == ctypes.c_int
    assert callable(drt.Renderer.subdivide) and drt.SUBDIVIDE_SCHEMES == {"midpoint": 0, "loop": 1}
    assert drt.SubdividedMesh._fields == ("vertices", "faces", "parents")
    assert drt.SubdividedMesh.toScene is drt.IndexedMesh.toScene and drt.SubdividedMesh.triangles is drt.IndexedMesh.triangles
    doc = " ".join(drt.Renderer.subdivide.__doc__.split())
    for phrase in ("one read-back of vertex_count", "no Catmull-Clark, Butterfly or sqrt(3)", "no user crease tags or sharpness",
                   "no limit-surface projection or limit normals", "no adaptive refinement",
                   "no attribute interpolation beyond parents and the child order", "no RendererGroup and no command line"):
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


def test_the_checks_return_their_error_code_with_no_launch_in_the_documented_order():
    L = drt._lib
    stand_in, pending, buf, A = _stand_ins()
    h = ctypes.addressof(stand_in)
    VE, FA, OV, PA, OF, CNT = A, A + 1024, A + 2048, A + 4096, A + 6144, A + 8192

    def call(r=h, vertices=VE, nv=8, faces=FA, nt=4, scheme=1, out_v=OV, parents=PA, cap=20, out_f=OF, count=CNT):
        return L.drt_renderer_subdivide(r, vertices, nv, faces, nt, scheme, out_v, parents, cap, out_f, count, None)

    def refused(what, **kw):
        assert call(**kw) == drt.ERR_INVALID, kw
        assert what in L.drt_last_error(), (kw, L.drt_last_error())

    refused(b"null argument", r=None)                                         # 1
    refused(b"null argument", count=None)
    for scheme in (-1, 2, 7):                                                 # 2
        refused(b"scheme", scheme=scheme)
    refused(b"null argument", count=None, scheme=5)                           # the order: an earlier check answers first
    refused(b"3 N < 2^31", nt=715827883)                                      # 3: 3 N = 2^31 + 1
    refused(b"3 N < 2^31", nt=0xFFFFFFFF)
    refused(b"scheme", scheme=2, nt=0xFFFFFFFF)
    refused(b"V + 3 N < 2^31", nt=715827882, nv=2)                            # 4: 3 N = 2^31 - 2
    refused(b"V + 3 N < 2^31", nv=0x80000000, nt=0)
    refused(b"V + 3 N < 2^31", nv=0xFFFFFFFF)
    refused(b"12 N < 2^31", nt=178956971, nv=0)                               # 5: 12 N = 2^31 + 4
    refused(b"12 N < 2^31", nt=715827882, nv=1)
    assert call(nt=178956970) != drt.ERR_INVALID or b"2^31" not in L.drt_last_error()      # 12 N = 2^31 - 8 passes these
    refused(b"3 N < 2^31", nt=0xFFFFFFFF, vertices=None, faces=None)
    refused(b"12 N < 2^31", nt=178956971, vertices=None)
    refused(b"null vertices", vertices=None)                                  # 7
    refused(b"null vertices", vertices=None, nt=0, faces=None, out_f=None)    # (no triangles: the vertices are still copied)
    refused(b"null faces or out_faces", faces=None)                           # 8
    refused(b"null faces or out_faces", out_f=None)
    refused(b"null vertices", vertices=None, faces=None)
    refused(b"if and only if", out_v=None, parents=None)                      # 9
    refused(b"if and only if", cap=0)
    refused(b"null faces or out_faces", faces=None, cap=0)
    refused(b"parents without out_vertices", out_v=None, cap=0)               # 10
    refused(b"if and only if", out_v=None)
    for name, base in (("vertices", VE), ("faces", FA), ("out_v", OV), ("parents", PA), ("out_f", OF), ("count", CNT)):      # 11
        refused(b"aligned", **{name: base + 2})
    refused(b"parents without", out_v=None, cap=0, count=CNT + 1)
    refused(b"alias", out_v=VE + 4 * 20)                                      # 12: 8 vertices are 96 bytes
    refused(b"alias", out_v=VE - 12 * 20 + 4)
    refused(b"alias", parents=FA + 44)                                        # 4 triangles are 48 bytes
    refused(b"alias", out_f=FA - 48 * 4 + 4)
    refused(b"alias", count=VE + 92)
    refused(b"alias", count=FA)
    refused(b"aligned", out_v=VE + 2)
    refused(b"pending", r=ctypes.addressof(pending))                          # 13
    refused(b"alias", r=ctypes.addressof(pending), out_f=FA)
    kws = [{}, dict(scheme=0), dict(parents=None), dict(out_v=None, parents=None, cap=0), dict(nt=0, faces=None, out_f=None),
           dict(nv=0, vertices=None), dict(out_v=VE + 96, cap=1, parents=None), dict(count=FA + 48)]
    for kw in kws:                                                            # 14: the device is asked only now
        _after_the_checks(L, call(**kw))


def test_bad_arguments_are_refused_by_the_python_interface_before_any_device_work():
    r = drt.Renderer.__new__(drt.Renderer)                                     # (no device: only the argument check runs)
    r._device = 0
    v, f = np.zeros((4, 3), np.float32), np.zeros((2, 3), np.int32)
    mesh = drt.IndexedMesh(v, f, None)
    cases = [(lambda: r.subdivide(mesh, levels=-1), "levels"), (lambda: r.subdivide(mesh, levels=1.5), "levels"),
             (lambda: r.subdivide(mesh, levels=True), "levels"), (lambda: r.subdivide(mesh, levels="2"), "levels"),
             (lambda: r.subdivide(mesh, levels=None), "levels"),
             (lambda: r.subdivide(mesh, scheme="Loop"), "scheme"), (lambda: r.subdivide(mesh, scheme=1), "scheme"),
             (lambda: r.subdivide(mesh, scheme="butterfly"), "scheme"), (lambda: r.subdivide(mesh, scheme=None), "scheme"),
             (lambda: r.subdivide(5), "mesh"), (lambda: r.subdivide((v, f.astype(np.int64))), "faces"),
             (lambda: r.subdivide((v, f.reshape(3, 2))), "faces"), (lambda: r.subdivide((v.astype(np.float64), f)), "vertices"),
             (lambda: r.subdivide((v.reshape(3, 4), f), levels=0), "vertices"),
             (lambda: r.subdivide(drt.SubdividedMesh(v, f.astype(np.uint32), None), scheme="midpoint"), "faces"),
             (lambda: r.subdivide(np.zeros((2, 3, 3), np.float32)), "faces")]                  # (a soup is no indexed mesh)
    for call, word in cases:
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == drt.ERR_INVALID and word in str(e.value), (word, str(e.value))


def _flat(text):
    return re.sub(r" +", " ", re.sub(r"\s*\n \*\s*", " ", text))


def test_the_header_states_the_rule_and_what_it_is_not():
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    assert text.index("---- device edge adjacency (new") < text.index("---- mesh subdivision (new") < text.index("---- first-hit guide buffers")
    flat = _flat(text[text.index("---- mesh subdivision (new"):text.index("#define DRT_SUBDIVIDE_MIDPOINT")])
    for phrase in ("The connectivity is drt_renderer_face_adjacency's of faces -- by index, with the edges numbered",
                   "Even vertices keep their ids 0 ... V - 1; the odd vertex of edge e is V + e; *vertex_count = V + E always",
                   "V + 3 N always suffices", "out_vertices and parents are NULL iff vertex_capacity == 0, and parents alone may be NULL",
                   "m(h) = V + edge[h] if edge[h] >= 0, otherwise faces[h]: an index edge of zero length has no new vertex",
                   "[4 N][3], always complete, with no compaction",
                   "child 4 t + 0 = (a, m0, m2), child 4 t + 1 = (b, m1, m0), child 4 t + 2 = (c, m2, m1), child 4 t + 3 = (m0, m1, m2)",
                   "child k < 3 starts at corner k; the source triangle of child j is j >> 2",
                   "Out-of-range indices are copied as they are", "nothing faults",
                   "(v, v) for an even vertex", "with h = half_edge[e], (faces[h], faces[next(h)])",
                   "a closed oriented manifold input gives a closed oriented manifold output, adj >= 0 everywhere",
                   "V' - E' + F' = V - E + F", "a same-way pair, a fan or a boundary stays one in the output",
                   "float64 with one rounding per operation, in the order written, then one rounding to fp32",
                   "USABLE iff both ends of its representative half-edge are inside [0, V)", "all six coordinates are finite",
                   "three words 0x7FC00000", "even vertices copy their 12 bytes", "(float)(((double)pa + (double)pb) * 0.5)",
                   "the same bits whichever half-edge represents the edge",
                   "INTERIOR iff its representative h has adj[h] >= 0", "(-1 or -2: boundary, fan, same-way pair) is a CREASE",
                   "(float)(((double)pa + (double)pb) * 0.375 + ((double)pc + (double)pd) * 0.125)",
                   "if c or d is out of range or not finite, the midpoint", "A crease odd vertex is the midpoint",
                   "exactly drt_renderer_smooth_vertices' quantisation", "e = floor(log2 M), k = 27 - e (M = 0: k = 0)",
                   "q(x) = (int64) trunc((double)x * 2^k)", "One pass over the EDGES, not the half-edges",
                   "adds q(pb) to acc[a] and q(pa) to acc[b]", "Unusable edges add nothing", "S = (double)acc * 2^-k",
                   "n_cr == 0 && n_int == 0: the vertex keeps its bits",
                   "beta = (n_int == 3) ? 0.1875 : 0.375 / (double)n_int (Warren's weights)",
                   "p' = (float)((double)p + beta * (S_int - (double)n_int * (double)p))",
                   "n_cr == 2: p' = (float)((double)p + 0.125 * (S_cr - 2.0 * (double)p)); interior edges are ignored",
                   "any other n_cr (a dart, a corner where three creases meet, a non-manifold vertex): the vertex keeps its bits",
                   "the same bytes on every run, in every launch shape",
                   "in this order: NULL r or vertex_count; a scheme other than 0 or 1; 3 N >= 2^31; V + 3 N >= 2^31; 12 N >= 2^31",
                   "N == 0 stores *vertex_count = V, copies the stored vertices",
                   "NULL vertices with V > 0; NULL faces or out_faces with N > 0; out_vertices NULL without vertex_capacity 0 or the reverse; "
                   "parents without out_vertices; every pointer 4-byte aligned; an output overlapping vertices or faces; a pending "
                   "asynchronous batch; then every pointer must be device memory on the renderer's device",
                   "DRT_ERR_DEVICE", "legal on a sharded renderer"):
        assert phrase in flat, phrase
    limits = flat[flat.index("What this is not:"):]
    for phrase in ("no Catmull-Clark, Butterfly or sqrt(3)", "no user crease tags or sharpness", "no limit-surface projection or limit normals",
                   "no adaptive refinement", "no attribute interpolation beyond parents and the child order",
                   "no drt_group_* form and no command line"):
        assert phrase in limits, phrase
    version = _flat(text[:text.index("#define DRT_ABI_VERSION 2")])
    assert "and so is the subdivision entry point (drt_renderer_subdivide)" in version
    assert "#define DRT_SUBDIVIDE_MIDPOINT 0" in text and "#define DRT_SUBDIVIDE_LOOP 1" in text


def test_the_kernel_follows_the_stated_design():
    csrc = os.path.join(ROOT, "dustraytracer_amd", "csrc")
    code = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "kernel_subdivide.hip")).read())
    capi = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "drt_capi_subdivide.cpp")).read())
    assert code.count("__launch_bounds__(kWeldThreads)") == 3 and "atomicAdd(reinterpret_cast<unsigned long long *>(p)" in code
    assert code.count("atomicAdd(") == 3 and code.count("atomicAdd(&cnt[") == 2     # integer atomics only: 64-bit sums, 32-bit counts
    assert code.count("t += stride") == 1 and code.count("e += stride") == 1 and code.count("v += stride") == 1      # grid-stride loops
    for word in ("while (", "for (;;)", "__syncthreads", "__shared__", "hipStreamSynchronize", "dim3(kWeldThreads), 0, 0,"):
        assert word not in code, word                                           # no lane waits for another; nothing on the null stream
    assert "launch_adjacency(AdjacencyKey::index, adj, s)" in capi and "launch_smooth_maximum(m, r->num_cus, s)" in capi
    # the interior sums reuse the words of `other` only behind the adjacency's launches, in stream order
    assert capi.index("launch_adjacency(AdjacencyKey::index") < capi.index("hipMemsetAsync(r->wd_acc.ptr") < capi.index("launch_subdivide(")
    assert capi.index("grow(r, r->wd_acc") < capi.index("launch_adjacency(AdjacencyKey::index")
    state = open(os.path.join(csrc, "renderer_state.hpp")).read()
    for name in ("sd_adj", "sd_edge", "sd_half_edge", "sd_cnt", "sd_acc"):
        assert name in state and name in capi, name
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "kernel_subdivide.hip" in make and "drt_capi_subdivide.cpp" in make
    for name in ("kernel_adjacency.hip", "kernel_weld.hip"):                    # used through their seams
        assert "subdivide" not in open(os.path.join(csrc, name)).read().lower(), name


def test_cpp_wrapper_compiles_and_links(tmp_path):
    src = tmp_path / "subdivide_calls.cpp"
    src.write_text(r"""
#include <cstdio>
#include "DustRayTracer.hpp"
// the statements only -- main() runs none of them without arguments
int main(int argc, char **) {
    if (argc < 2) {
        std::printf("%d %d\n", DRT_SUBDIVIDE_MIDPOINT, DRT_SUBDIVIDE_LOOP);
        return 0;
    }
    Renderer r(0);
    const float *vertices = nullptr;
    const int32_t *faces = nullptr;
    float *out_vertices = nullptr;
    int32_t *parents = nullptr, *out_faces = nullptr;
    uint32_t *count = nullptr;
    r.Subdivide(vertices, 8u, faces, 10u, out_vertices, parents, 38u, out_faces, count);
    r.Subdivide(vertices, 8u, faces, 10u, out_vertices, nullptr, 38u, out_faces, count, DRT_SUBDIVIDE_MIDPOINT, nullptr);
    r.Subdivide(vertices, 8u, faces, 10u, nullptr, nullptr, 0u, out_faces, count, DRT_SUBDIVIDE_LOOP);
    return 0;
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    exe = tmp_path / "subdivide_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib_dir, "-ldrt_hip",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["0", "1"]
