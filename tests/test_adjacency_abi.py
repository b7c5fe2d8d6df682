"""The device edge-adjacency entry points of include/drt.h without a GPU: exported, bound, every argument check that comes before any
device work, the header states the rule for both kinds of end and says what it is not, the Python wrappers refuse bad arguments, the
kernel follows the stated design, and the C++ wrappers compile and link."""
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
    P, U, I = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    for name in ("drt_renderer_tri_adjacency", "drt_renderer_face_adjacency", "drt_renderer_boundary_vertices", "drt_renderer_adjacency_route"):
        assert hasattr(lib, name), name
    assert list(drt._lib.drt_renderer_tri_adjacency.argtypes) == [P, P, U, U, P, P, P, U, P, P]
    assert list(drt._lib.drt_renderer_face_adjacency.argtypes) == [P, P, U, P, P, P, U, P, P]
    assert list(drt._lib.drt_renderer_boundary_vertices.argtypes) == [P, P, P, U, U, U, P, P]
    assert list(drt._lib.drt_renderer_adjacency_route.argtypes) == [P] and drt._lib.drt_renderer_adjacency_route.restype == I
    for name in ("edgeAdjacency", "boundaryVertices", "adjacencyRoute", "smooth"):
        assert callable(getattr(drt.Renderer, name)), name
    assert drt.MeshEdges._fields == ("adj", "edge", "half_edge", "count") and callable(drt.MeshEdges.euler)
    doc = " ".join(drt.Renderer.edgeAdjacency.__doc__.split())
    for phrase in ("no vertex-to-triangle lists", "no tolerance", "no orientation repair", "no RendererGroup"):
        assert phrase in doc, phrase
    assert "Renderer.edgeAdjacency" in " ".join(drt.triEdgeAdjacency.__doc__.split())
    assert drt._lib.drt_abi_version() == 2 and drt._lib.drt_renderer_adjacency_route(None) == 0


def _stand_ins():
    stand_in = ctypes.create_string_buffer(1 << 16)              # a block of zeros stands in for the renderer: it is not looked at yet
    pending = ctypes.create_string_buffer(b"\x01" * (1 << 16), 1 << 16)      # every flag of the stand-in true: a batch is pending
    buf = ctypes.create_string_buffer(1 << 14)
    return stand_in, pending, buf, (ctypes.addressof(buf) + 15) & ~15


def _after_the_checks(L, rc):
    """all checks passed: only now the renderer is looked at and the device asked for -- host memory or no device, the call fails"""
    assert rc in (drt.ERR_INVALID, drt.ERR_DEVICE)
    assert b"device" in L.drt_last_error().lower() or b"hip" in L.drt_last_error().lower()


@pytest.mark.parametrize("by_position", [True, False])
def test_adjacency_checks_return_their_error_code_with_no_launch(by_position):
    L = drt._lib
    stand_in, pending, buf, A = _stand_ins()
    h = ctypes.addressof(stand_in)
    T, ADJ, ED, HE, CNT = A, A + 1024, A + 2048, A + 3072, A + 4096
    first_name = b"tris" if by_position else b"faces"

    def call(r=h, first=T, n=4, stride=36, adj=ADJ, edge=ED, half_edge=HE, cap=12, count=CNT):
        if by_position:
            return L.drt_renderer_tri_adjacency(r, first, n, stride, adj, edge, half_edge, cap, count, None)
        return L.drt_renderer_face_adjacency(r, first, n, adj, edge, half_edge, cap, count, None)

    def refused(what, **kw):
        assert call(**kw) == drt.ERR_INVALID, kw
        assert what in L.drt_last_error(), (kw, L.drt_last_error())

    refused(b"null argument", r=None)
    if by_position:
        for stride in (0, 12, 35, 40, 44, 52, 96, 128):
            refused(b"stride", stride=stride)
        refused(b"stride", stride=7, n=0xFFFFFFFF, first=None)                # the order: an earlier check answers first
    refused(b"2^31", n=715827883)                                 # 3 n = 2^31 + 1
    refused(b"2^31", n=0xFFFFFFFF)
    assert call(n=715827882) != drt.ERR_INVALID or b"2^31" not in L.drt_last_error()      # 3 n = 2^31 - 2 passes this check
    assert call(n=0, first=None, adj=None, edge=ED + 1, half_edge=None, count=None) == 0  # no triangles: a no-op, nothing is looked at
    assert call(n=0, r=ctypes.addressof(pending)) == 0
    refused(b"null " + first_name + b" or adj", first=None)
    refused(b"null " + first_name + b" or adj", adj=None)
    refused(b"null together", edge=None)
    refused(b"null together", count=None)
    refused(b"without edge", edge=None, count=None)
    refused(b"without edge", edge=None, count=None, half_edge=None)
    refused(b"without edge", edge=None, count=None, cap=0)
    refused(b"if and only if", half_edge=None)
    refused(b"if and only if", cap=0)
    for name, base in (("first", T), ("adj", ADJ), ("edge", ED), ("half_edge", HE), ("count", CNT)):
        refused(b"aligned", **{name: base + 2})
    refused(b"2^31", n=0xFFFFFFFF, first=None, edge=None)
    refused(b"null " + first_name, first=None, edge=None, count=CNT + 1)
    refused(b"null together", edge=None, half_edge=None, adj=ADJ + 1)
    refused(b"if and only if", half_edge=None, count=CNT + 1)
    kws = [{}, dict(half_edge=None, cap=0), dict(edge=None, half_edge=None, cap=0, count=None)] + ([dict(stride=48)] if by_position else [])
    for kw in kws:
        _after_the_checks(L, call(**kw))
    refused(b"pending", r=ctypes.addressof(pending))


def test_boundary_checks_return_their_error_code_with_no_launch():
    L = drt._lib
    stand_in, pending, buf, A = _stand_ins()
    h = ctypes.addressof(stand_in)
    FA, ADJ, OUT = A, A + 1024, A + 2048

    def call(r=h, faces=FA, adj=ADJ, nt=4, nv=8, flags=0, out=OUT):
        return L.drt_renderer_boundary_vertices(r, faces, adj, nt, nv, flags, out, None)

    def refused(what, **kw):
        assert call(**kw) == drt.ERR_INVALID, kw
        assert what in L.drt_last_error(), (kw, L.drt_last_error())

    refused(b"null argument", r=None)
    for flags in (2, 3, 0x80000000):
        refused(b"flags", flags=flags)
    refused(b"2^31", nt=715827883)
    refused(b"2^31", nv=0x80000000)
    assert call(nv=0, out=None, faces=None, adj=None) == 0        # no vertices: a no-op
    refused(b"null out", out=None)
    refused(b"null faces or adj", faces=None)
    refused(b"null faces or adj", adj=None)
    refused(b"aligned", faces=FA + 2)
    refused(b"aligned", adj=ADJ + 1)
    refused(b"flags", flags=4, nt=0xFFFFFFFF, out=None)           # the order
    refused(b"2^31", nt=0xFFFFFFFF, out=None)
    refused(b"null out", out=None, faces=None)
    for kw in ({}, dict(flags=1), dict(out=OUT + 1), dict(nt=0, faces=None, adj=None)):
        _after_the_checks(L, call(**kw))
    refused(b"pending", r=ctypes.addressof(pending))


def test_bad_arguments_are_refused_by_the_python_interface_before_any_device_work():
    r = drt.Renderer.__new__(drt.Renderer)                                     # (no device: only the argument check runs)
    r._device = 0
    v, f = np.zeros((4, 3), np.float32), np.zeros((2, 3), np.int32)
    mesh = drt.IndexedMesh(v, f, None)
    cases = [(lambda: r.edgeAdjacency(np.zeros((2, 3, 3), np.float64)), "dtype"), (lambda: r.edgeAdjacency(np.zeros((2, 9), np.float32)), "shape"),
             (lambda: r.edgeAdjacency(5), "mesh"), (lambda: r.edgeAdjacency((v, f.astype(np.int64))), "faces"),
             (lambda: r.edgeAdjacency((v, f.reshape(3, 2)), edges=True), "faces"), (lambda: r.edgeAdjacency((v.astype(np.float64), f)), "vertices"),
             (lambda: r.boundaryVertices(5), "mesh"), (lambda: r.boundaryVertices((v, f.astype(np.int64))), "faces"),
             (lambda: r.smooth(mesh, fixed="edges"), "fixed"), (lambda: r.smooth(mesh, fixed="Boundary"), "fixed")]
    for call, word in cases:
        with pytest.raises(drt.DrtError) as e:
            call()
        assert e.value.code == drt.ERR_INVALID and word in str(e.value), (word, str(e.value))


def _flat(text):
    return re.sub(r" +", " ", re.sub(r"\s*\n \*\s*", " ", text))


def test_the_header_states_the_rule_and_what_it_is_not():
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    assert text.index("---- mesh simplification (new") < text.index("---- device edge adjacency (new") < text.index("---- first-hit guide buffers")
    flat = _flat(text[text.index("---- device edge adjacency (new"):text.index("#define DRT_BOUNDARY_BAD_EDGES")])
    for phrase in ("Half-edge h = 3 t + e runs from corner e to corner (e + 1) % 3 of triangle t",
                   "the three 32-bit words of the corner at tris + t * stride + 12 e, stride 36 (float [N][3][3]) or 48 (drt_tri), compared as integers",
                   "-0.0 and +0.0 differ, NaNs are compared by their bits, there is no tolerance",
                   "the int32 word faces[3 t + e], compared as an integer", "No vertex array is read, so no value is out of range",
                   "the same unordered pair of ends", "a half-edge whose two ends are equal (zero length) gets -2", "a group of one half-edge gets -1",
                   "a group of exactly two that run in opposite directions (the start of one is the end of the other) are each other's twins",
                   "every other group -- three or more, two that run the same way -- gets -2",
                   "the same bytes as drt_tri_edge_adjacency's table of the same triangles for every input",
                   "edge, half_edge and edge_count are NULL together", "its representative is its smallest half-edge",
                   "numbered in ascending representative, which is by first appearance", "-1 for a zero-length one",
                   "*edge_count = E, stored whether or not capacity held all edges", "V - E + F without a host pass",
                   "out[v] = 1 iff a half-edge with adj == -1 starts or ends at v", "With DRT_BOUNDARY_BAD_EDGES (flag bit 0) adj == -2 counts as well",
                   "A triangle with an index outside [0, n_vertices) is skipped (a bounds check, never a fault)",
                   "from the host scene's positions in tree order", "a device refit leaves it alone", "DRT_ADJACENCY=host",
                   "0 = no table since the last upload, 1 = it was made on the host, 2 = on the device",
                   "the same bytes on every run, in every launch shape", "the hash decides nothing that can be observed",
                   "N == 0 is a no-op that touches nothing, edge_count included", "DRT_ERR_DEVICE"):
        assert phrase in flat, phrase
    limits = flat[flat.index("What this is not:"):]
    for phrase in ("no vertex-to-triangle lists", "no tolerance", "no orientation repair", "no drt_group_* form and no command line"):
        assert phrase in limits, phrase
    version = _flat(text[:text.index("#define DRT_ABI_VERSION 2")])
    assert "the device edge-adjacency entry points (drt_renderer_tri_adjacency / _face_adjacency / _boundary_vertices / _adjacency_route)" in version
    assert "#define DRT_BOUNDARY_BAD_EDGES 1u" in text


def test_the_kernel_follows_the_stated_design():
    src = open(os.path.join(ROOT, "dustraytracer_amd", "csrc", "kernel_adjacency.hip")).read()
    hpp = open(os.path.join(ROOT, "dustraytracer_amd", "csrc", "adjacency.hpp")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomicCAS(&a.table[slot], kWeldEmpty, h)" in code and "atomicMin(&a.table[slot], h)" in code and "pcg_hash" in code
    assert "atomicMin(&a.other[rep], h)" in code and "atomicMin(&a.other[rep], kAdjMany)" in code
    assert "atomicAdd" not in code and "float" not in code                   # integers only: minima and compare-and-swap
    assert "template <int K>" in code and "launch_adjacency_of<3>" in code and "launch_adjacency_of<1>" in code      # one template, two keys
    for word in ("while (true)", "while (1)", "for (;;)", "while ("):        # no lane waits for another: every loop is bounded
        assert word not in code, word
    assert "bytes per triangle" in hpp and "wd_table" in hpp and "wd_rep" in hpp and "wd_blocks" in hpp
    for name, host_calls in (("drt_capi_topology.cpp", 0), ("drt_capi_contour.cpp", 1)):      # one helper makes the scene's table; the one
        text = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "dustraytracer_amd", "csrc", name)).read())      # host call left is drt_scene_edge_adjacency's
        assert text.count("scene_adjacency(r, scene, s)") == 1 and text.count("host.edge_adjacency()") == host_calls, name


def test_cpp_wrappers_compile_and_link(tmp_path):
    src = tmp_path / "adjacency_calls.cpp"
    src.write_text(r"""
#include <cstdio>
#include "DustRayTracer.hpp"
// the statements only -- main() runs none of them without arguments
int main(int argc, char **) {
    if (argc < 2) {
        std::printf("%u\n", DRT_BOUNDARY_BAD_EDGES);
        return 0;
    }
    Renderer r(0);
    const drt_iso_tri *records = nullptr;
    const float *soup = nullptr;
    const int32_t *faces = nullptr;
    int32_t *adj = nullptr, *edge = nullptr, *half_edge = nullptr;
    uint32_t *count = nullptr;
    uint8_t *out = nullptr;
    r.TriAdjacency(records, 10u, (uint32_t)sizeof(drt_iso_tri), adj);
    r.TriAdjacency(soup, 10u, 36u, adj, edge, half_edge, 30u, count, nullptr);
    r.FaceAdjacency(faces, 10u, adj);
    r.FaceAdjacency(faces, 10u, adj, edge, nullptr, 0u, count, nullptr);
    r.BoundaryVertices(faces, adj, 10u, 8u, out);
    r.BoundaryVertices(faces, adj, 10u, 8u, out, DRT_BOUNDARY_BAD_EDGES, nullptr);
    return drt_renderer_adjacency_route(nullptr);
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    exe = tmp_path / "adjacency_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib_dir, "-ldrt_hip",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["1"]
