"""The section-contour entry points of include/drt.h without a GPU: exported, bound, laid out as declared, the argument checks that come
before any device work in the plane-section query's order, the header states the rule, the C++ wrappers compile and link, and
drt_scene_edge_adjacency is bit-equal to the dictionary of tests/contour_ref.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import contour_ref as cr
from tests import contour_scenes as cs
from tests import hostile_meshes as hm
from tests import ray_query_ref as rq
from tests.scenes import ROOT, scene_path

drt = pytest.importorskip("dustraytracer_amd")


def test_the_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(drt.LIB_PATH)
    assert hasattr(lib, "drt_renderer_chain_sections") and hasattr(lib, "drt_scene_edge_adjacency")
    fn = drt._lib.drt_renderer_chain_sections
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 9
    assert fn.argtypes[6] is ctypes.c_uint32 and fn.argtypes[7] is ctypes.c_uint32                     # n, total
    assert all(fn.argtypes[i] is ctypes.c_void_p for i in (0, 1, 2, 3, 4, 5, 8))
    fn = drt._lib.drt_scene_edge_adjacency
    assert fn.restype is ctypes.c_int and fn.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    for method in ("chainSections", "contours"):
        assert callable(getattr(drt.Renderer, method)), method
    assert callable(drt.Scene.edgeAdjacency) and callable(drt.ContourList.areas)
    assert drt.ContourList._fields == ("splits", "chain_splits", "closed", "p", "q", "prim", "code", "end")
    assert (drt.CHAIN_LINKED, drt.CHAIN_BOUNDARY, drt.CHAIN_NON_MANIFOLD, drt.CHAIN_NOT_LISTED, drt.CHAIN_OTHER_EDGES, drt.CHAIN_MISS) == (0, 1, 2, 3, 4, 5)
    assert drt._lib.drt_abi_version() == 2


def test_slot_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "drt.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu\n", sizeof(drt_chain_slot), offsetof(drt_chain_slot, seg), offsetof(drt_chain_slot, first),
           offsetof(drt_chain_slot, length), offsetof(drt_chain_slot, flags));
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["16", "0", "4", "8", "12"]
    assert cr.SLOT.itemsize == 16 and [cr.SLOT.fields[f][1] for f in ("seg", "first", "length", "flags")] == [0, 4, 8, 12]


def test_the_argument_checks_are_the_plane_query_s_in_its_order():
    """drt_renderer_plane_sections fed the same bad calls gives the same codes: the handles, n == 0, the NULL pointers, the alignment."""
    L = drt._lib
    sc = drt.Scene()
    chain, section = L.drt_renderer_chain_sections, L.drt_renderer_plane_sections
    assert chain(None, sc._h, None, None, None, None, 4, 4, None) == drt.ERR_INVALID
    assert b"null" in L.drt_last_error()
    assert chain(None, None, None, None, None, None, 0, 0, None) == drt.ERR_INVALID                   # the handles are checked before n == 0
    stand_in = ctypes.create_string_buffer(1 << 16)                              # a block of zeros stands in for the renderer
    h = ctypes.addressof(stand_in)
    assert chain(h, None, None, None, None, None, 0, 0, None) == drt.ERR_INVALID
    # n == 0 or total == 0: nothing to do, whatever the pointers are
    for n, total in ((0, 0), (0, 4), (4, 0)):
        assert chain(h, sc._h, None, None, None, None, n, total, None) == drt.OK
    assert section(h, sc._h, None, None, None, 0, None, 0, 0, None) == drt.OK
    buf = ctypes.create_string_buffer(256)
    B = (ctypes.addressof(buf) + 15) & ~15
    # the NULL pointers, before anything is dereferenced
    for what, args in (("null segs", (None, B, B, B)), ("null splits", (B, None, B, B)), ("null slots", (B, B, None, B)), ("all null", (None, None, None, None))):
        assert chain(h, sc._h, *args, 4, 4, None) == drt.ERR_INVALID, what
        assert b"null segment, split or slot" in L.drt_last_error(), what
    assert section(h, sc._h, None, B, B, 4, B, 4, 0, None) == section(h, sc._h, B, None, B, 4, B, 4, 0, None) == drt.ERR_INVALID
    # the alignment: segs and slots 16 bytes, splits and chains 4
    for what, args in (("misaligned segs", (B + 4, B, B, B)), ("misaligned slots", (B, B, B + 8, B)), ("misaligned splits", (B, B + 1, B, B)),
                       ("misaligned chains", (B, B, B, B + 2)), ("misaligned chains, the rest fine", (B + 16, B + 4, B + 32, B + 3))):
        assert chain(h, sc._h, *args, 4, 4, None) == drt.ERR_INVALID, what
        assert b"aligned" in L.drt_last_error(), what
    assert section(h, sc._h, B + 4, B, B, 4, B, 4, 0, None) == section(h, sc._h, B, B + 1, B, 4, B, 4, 0, None) == drt.ERR_INVALID
    assert b"aligned" in L.drt_last_error()
    # fewer than 2^31 planes and records
    assert chain(h, sc._h, B, B, B, None, 0x80000000, 4, None) == drt.ERR_INVALID and b"planes" in L.drt_last_error()
    assert chain(h, sc._h, B, B, B, None, 4, 0x80000000, None) == drt.ERR_INVALID and b"records" in L.drt_last_error()
    assert chain(h, sc._h, B, B, B, None, 4, 0xffffffff, None) == drt.ERR_INVALID
    assert section(h, sc._h, B, B, B, 4, B, 0x80000000, 0, None) == drt.ERR_INVALID and b"planes" in L.drt_last_error()
    # NULL comes before the alignment, the alignment before the counts
    assert chain(h, sc._h, None, B + 1, B, None, 0x80000000, 4, None) == drt.ERR_INVALID and b"null" in L.drt_last_error()
    assert chain(h, sc._h, B, B + 1, B, None, 0x80000000, 4, None) == drt.ERR_INVALID and b"aligned" in L.drt_last_error()


def test_the_adjacency_reader_s_errors():
    L = drt._lib
    out = np.zeros(64, np.int32)
    assert L.drt_scene_edge_adjacency(None, out.ctypes.data, 64) == drt.ERR_INVALID
    sc, _ = cs.scene(drt, "tetrahedron")
    assert L.drt_scene_edge_adjacency(sc._h, out.ctypes.data, 11) == drt.ERR_INVALID and b"too small" in L.drt_last_error()
    assert L.drt_scene_edge_adjacency(sc._h, None, 12) == drt.ERR_INVALID
    assert (out == 0).all()
    assert L.drt_scene_edge_adjacency(sc._h, out.ctypes.data, 64) == drt.OK and (out[12:] == 0).all() and (out[:12] >= 0).all()
    flat = drt.Scene()                                                         # geometry without a tree: the table is in tree order
    flat.addMaterial(*cs.ONE_MATERIAL[0])
    n = len(cs.QUAD)
    flat.setGeometry(cs.QUAD, np.zeros((n, 3, 3), np.float32), np.zeros((n, 3, 2), np.float32), np.zeros(n, np.int32))
    assert L.drt_scene_edge_adjacency(flat._h, out.ctypes.data, 64) == drt.ERR_INVALID and b"BVH" in L.drt_last_error()
    with pytest.raises(drt.DrtError) as e:
        flat.edgeAdjacency()
    assert e.value.code == drt.ERR_INVALID
    empty = drt.Scene()
    empty.addMaterial(*cs.ONE_MATERIAL[0])
    empty.setGeometry(np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 2), np.float32), np.zeros(0, np.int32))
    drt.BVHBuilder().buildIterative(empty)
    assert empty.edgeAdjacency().shape == (0, 3)


def _scene(name):
    if name == "soup":
        return rq.programmatic_scene(drt, *rq.soup(3000, 5), 2, 8)[0]
    if name == "degenerate":
        return hm.scene_pair(drt, hm.degenerate())[0]
    if name == "cornell_box":
        sc = drt.Scene()
        sc.loadGLTFmodel(scene_path(name))
        b = drt.BVHBuilder()
        b.m_TargetLeafPrimitivesCount, b.m_BinCount = 20, 8
        b.buildIterative(sc)
        return sc
    return cs.scene(drt, name)[0]


@pytest.mark.parametrize("name", ["cube", "cornell_box", "soup", "degenerate", "tetrahedron", "quad", "book", "flipped_quad", "hollow_box", "ring"])
def test_the_adjacency_is_bit_equal_to_the_restatement(name):
    sc = _scene(name)
    got = sc.edgeAdjacency()
    want = cr.adjacency(cs.tree_positions(sc))
    assert got.dtype == np.int32 and got.shape == (len(want) // 3, 3) and got.tobytes() == want.tobytes(), name
    counts = {v: int((want == v).sum()) for v in (-1, -2)}
    print("%s: %d half-edges, %d twinned, %d boundary, %d non-manifold / flipped / zero-length" % (name, len(want), (want >= 0).sum(), counts[-1], counts[-2]))
    if name == "degenerate":
        assert counts[-2] > 0 and counts[-1] > 0 and (want >= 0).any()          # duplicates and zero-length edges; shared edges
    if name in ("cube", "tetrahedron", "hollow_box"):
        assert (want >= 0).all()                                                # closed and manifold


def test_the_header_states_the_rule():
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    sec = text[text.index("section contours (new"):text.index("typedef struct drt_chain_slot ")]
    assert "plane sections (new" not in sec
    flat = re.sub(r"\s*\n \*\s*", " ", sec)
    for phrase in ("no coordinate is compared, no tolerance is chosen", "3 * n_triangles host values", "h = 3 * t + e", "t in tree order",
                   "runs from vertex e to vertex (e + 1) % 3", "not the packed v0 + e1", "the same iff their three words are bit-equal",
                   "grouped by their unordered pair of endpoint positions", "run in opposite directions is a pair of twins",
                   "A group of one is a boundary edge: adj[h] = -1", "Everything else is -2", "two that run the same way",
                   "an edge whose two ends are the same position", "dropped with that upload", "the table is still the host scene's",
                   "a refit keeps the triangle order, and a deformation keeps shared positions shared", "splits holds n + 1 values",
                   "plane i owns segs[splits[i] .. splits[i+1])", "a decreasing pair is an empty range",
                   "nothing beyond total is read or written", "records in ascending prim, followed by any miss records (prim < 0)",
                   "Unsorted input gives unspecified links, but the call completes and every index it writes is inside the plane's own range",
                   "k = code & 3 and up = code >> 2", "in_j = up ? k : (k + 2) % 3", "out_j = up ? (k + 2) % 3 : k",
                   "the segment runs P -> Q iff the apex is above", "a = adj[3 * prim_j + out_j]", "prim_m == a / 3",
                   "binary search in the ascending prefix", "3 * prim_m + in_m == a", "1 = boundary edge (a == -1)",
                   "2 = non-manifold or flipped (a == -2)", "3 = the neighbour is not in the list", "4 = the neighbour is cut through other edges",
                   "5 = j is a miss record", "succ is injective", "simple paths and simple cycles",
                   "a path starts at its record without a predecessor", "a cycle starts at its record of smallest index, and is closed",
                   "ordered by the ascending index of their first record", "Miss records stay where they are, after all chains",
                   "seg = the index into segs of the record that stands there", "first = the position of its chain's first record",
                   "bit 0 = the chain is closed, bits 1..3 = that record's exit status", "{own index, own position, 1, 5 << 1}",
                   "chains[2 * i] is the number of chains of plane i, misses not counted", "chains[2 * i + 1] is how many of them are closed",
                   "chains may be NULL", "depends on segs, splits and the adjacency only", "no welding and no new points",
                   "plus the last q of an open chain", "agree on which of their shared vertices are above the plane",
                   "statuses 3 and 4 mark the places where they do not", "no caps or filled polygons", "no RendererGroup",
                   "nothing on the command line", "n == 0 or total == 0 is DRT_OK with no launch", "n < 2^31 and total < 2^31",
                   "counters, kernel info and kernel span are not touched"):
        assert phrase in flat, phrase
    # directly after the plane-section declaration, before the sphere casts
    assert text.index("drt_renderer_plane_sections(drt_renderer") < text.index("section contours (new") < text.index("sphere casts (new")
    between = text[text.index("drt_renderer_plane_sections(drt_renderer"):text.index("section contours (new")]
    assert "/* ----" in between and between.count("/*") == 1


def test_cpp_wrappers_compile_and_link(tmp_path):
    src = tmp_path / "contour_calls.cpp"
    src.write_text(r"""
#include <cstdio>
#include "DustRayTracer.hpp"
// the statements only -- main() runs none of them without arguments
int main(int argc, char **) {
    if (argc < 2) { std::printf("%zu %zu %d\n", sizeof(drt_chain_slot), alignof(drt_chain_slot), DRT_ABI_VERSION); return 0; }
    Scene scene;
    Renderer r(0);
    const drt_section *segs = nullptr;
    const uint32_t *splits = nullptr;
    drt_chain_slot *slots = nullptr;
    uint32_t *chains = nullptr;
    r.ChainSections(scene, segs, splits, slots, chains, 0u, 0u);
    r.ChainSections(scene, segs, splits, slots, nullptr, 0u, 0u, nullptr);
    std::vector<int32_t> adj = scene.EdgeAdjacency();
    return (int)adj.size();
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    exe = tmp_path / "contour_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib_dir, "-ldrt_hip",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["16", "4", "2"]


def test_bad_lists_are_refused_before_any_device_work():
    r = drt.Renderer.__new__(drt.Renderer)                                     # (no device: only the argument check runs)
    r._device = 0
    sc = drt.Scene()
    for bad in (None, (1, 2, 3), [np.zeros(1, np.int32)] * 5):
        with pytest.raises(drt.DrtError) as e:
            r.chainSections(sc, bad)
        assert e.value.code == drt.ERR_INVALID
    lst = drt.ContourList(*([np.zeros(0, np.int32)] * 8))
    assert lst.normals is None
    with pytest.raises(drt.DrtError) as e:
        lst.areas()
    assert e.value.code == drt.ERR_INVALID and "normals" in str(e.value)
