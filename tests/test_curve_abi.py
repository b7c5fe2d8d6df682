"""The intersection-curve entry points of include/drt.h without a GPU: exported, bound, the argument checks that come before any device
work in drt_renderer_chain_sections' order, the header states the rule, its limits and its place, the C++ wrappers compile and link,
drt_tri_edge_adjacency is drt_scene_edge_adjacency's rule and the restatement's, and the stand-alone run of the routine behind both."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import contour_scenes as cs
from tests import curve_ref as cu
from tests import curve_scenes as cv
from tests.scenes import ROOT

drt = pytest.importorskip("dustraytracer_amd")


def test_the_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(drt.LIB_PATH)
    assert hasattr(lib, "drt_renderer_chain_intersections") and hasattr(lib, "drt_tri_edge_adjacency")
    fn = drt._lib.drt_renderer_chain_intersections
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 10
    assert fn.argtypes[7] is ctypes.c_uint32 and fn.argtypes[8] is ctypes.c_uint32                     # n, total
    assert all(fn.argtypes[i] is ctypes.c_void_p for i in (0, 1, 2, 3, 4, 5, 6, 9))
    sections = drt._lib.drt_renderer_chain_sections.argtypes
    assert fn.argtypes == sections[:4] + [ctypes.c_void_p] + sections[4:]                             # chain_sections' with query_adj after splits
    fn = drt._lib.drt_tri_edge_adjacency
    assert fn.restype is ctypes.c_int and fn.argtypes == [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32]
    for method in ("chainIntersections", "intersectionCurves"):
        assert callable(getattr(drt.Renderer, method)), method
    assert callable(drt.triEdgeAdjacency) and callable(drt.CurveList.lengths)
    assert drt.CurveList._fields == ("chain_splits", "closed", "p", "q", "query", "prim", "code", "end")
    # what the feature leaves as it was
    assert drt.CutList._fields == ("splits", "p", "q", "prim", "code") and drt.SelfCuts._fields == ("pairs", "p", "q", "code")
    assert drt.ContourList._fields == ("splits", "chain_splits", "closed", "p", "q", "prim", "code", "end")
    assert "Not chained into curves" in drt.Renderer.intersectTriangles.__doc__
    assert "Self-intersection curves are not chained" in drt.Renderer.chainIntersections.__doc__
    assert drt._lib.drt_abi_version() == 2
    # every drt_* name of the header is bound
    header = open(os.path.join(ROOT, "include", "drt.h")).read()
    source = open(os.path.join(ROOT, "dustraytracer_amd", "__init__.py")).read()
    for name in ("drt_tri_edge_adjacency", "drt_renderer_chain_intersections"):
        assert name in header and name in source


def test_the_argument_checks_are_chain_sections_in_its_order():
    """drt_renderer_chain_sections fed the same bad calls gives the same codes; query_adj is checked where splits is."""
    L = drt._lib
    sc = drt.Scene()
    curve, chain = L.drt_renderer_chain_intersections, L.drt_renderer_chain_sections
    assert curve(None, sc._h, None, None, None, None, None, 4, 4, None) == drt.ERR_INVALID
    assert b"null" in L.drt_last_error()
    assert curve(None, None, None, None, None, None, None, 0, 0, None) == drt.ERR_INVALID             # the handles are checked before n == 0
    stand_in = ctypes.create_string_buffer(1 << 16)                              # a block of zeros stands in for the renderer
    h = ctypes.addressof(stand_in)
    assert curve(h, None, None, None, None, None, None, 0, 0, None) == chain(h, None, None, None, None, None, 0, 0, None) == drt.ERR_INVALID
    # n == 0 or total == 0: nothing to do, whatever the pointers are
    for n, total in ((0, 0), (0, 4), (4, 0)):
        assert curve(h, sc._h, None, None, None, None, None, n, total, None) == chain(h, sc._h, None, None, None, None, n, total, None) == drt.OK
    buf = ctypes.create_string_buffer(256)
    B = (ctypes.addressof(buf) + 15) & ~15
    # the NULL pointers, before anything is dereferenced: (segs, splits, query_adj, slots, counts)
    for what, args in (("null segs", (None, B, B, B, B)), ("null splits", (B, None, B, B, B)), ("null query_adj", (B, B, None, B, B)),
                       ("null slots", (B, B, B, None, B)), ("all null", (None, None, None, None, None))):
        assert curve(h, sc._h, *args, 4, 4, None) == drt.ERR_INVALID, what
        assert b"null segment, split, query adjacency or slot" in L.drt_last_error(), what
        if what != "null query_adj":
            assert chain(h, sc._h, args[0], args[1], args[3], args[4], 4, 4, None) == drt.ERR_INVALID, what
    # the alignment: segs and slots 16 bytes, splits, query_adj and counts 4
    for what, args in (("misaligned segs", (B + 4, B, B, B, B)), ("misaligned slots", (B, B, B, B + 8, B)), ("misaligned splits", (B, B + 1, B, B, B)),
                       ("misaligned query_adj", (B, B, B + 2, B, B)), ("misaligned counts", (B, B, B, B, B + 2)),
                       ("misaligned counts, the rest fine", (B + 16, B + 4, B + 8, B + 32, B + 3))):
        assert curve(h, sc._h, *args, 4, 4, None) == drt.ERR_INVALID, what
        assert b"aligned" in L.drt_last_error(), what
        if what != "misaligned query_adj":
            assert chain(h, sc._h, args[0], args[1], args[3], args[4], 4, 4, None) == drt.ERR_INVALID and b"aligned" in L.drt_last_error(), what
    # fewer than 2^31 queries and records
    assert curve(h, sc._h, B, B, B, B, None, 0x80000000, 4, None) == drt.ERR_INVALID and b"queries" in L.drt_last_error()
    assert curve(h, sc._h, B, B, B, B, None, 4, 0x80000000, None) == drt.ERR_INVALID and b"records" in L.drt_last_error()
    assert curve(h, sc._h, B, B, B, B, None, 4, 0xffffffff, None) == drt.ERR_INVALID
    assert chain(h, sc._h, B, B, B, None, 4, 0x80000000, None) == drt.ERR_INVALID and b"records" in L.drt_last_error()
    # NULL comes before the alignment, the alignment before the counts
    assert curve(h, sc._h, None, B + 1, B, B, None, 0x80000000, 4, None) == drt.ERR_INVALID and b"null" in L.drt_last_error()
    assert curve(h, sc._h, B, B, None, B + 8, None, 0x80000000, 4, None) == drt.ERR_INVALID and b"null" in L.drt_last_error()
    assert curve(h, sc._h, B, B, B + 1, B, None, 0x80000000, 4, None) == drt.ERR_INVALID and b"aligned" in L.drt_last_error()


def test_the_table_reader_s_errors():
    L = drt._lib
    out = np.zeros(16, np.int32)
    tris = np.zeros((2, 12), np.float32)
    assert L.drt_tri_edge_adjacency(tris.ctypes.data, 2, out.ctypes.data, 5) == drt.ERR_INVALID and b"too small" in L.drt_last_error()
    assert L.drt_tri_edge_adjacency(None, 2, out.ctypes.data, 6) == drt.ERR_INVALID and b"null" in L.drt_last_error()
    assert L.drt_tri_edge_adjacency(tris.ctypes.data, 2, None, 6) == drt.ERR_INVALID
    assert (out == 0).all()
    assert L.drt_tri_edge_adjacency(None, 0, None, 0) == drt.OK                 # nothing to do
    assert L.drt_tri_edge_adjacency(tris.ctypes.data, 2, out.ctypes.data, 16) == drt.OK
    assert (out[:6] == -2).all() and (out[6:] == 0).all()                       # every edge of a triangle of zeros has both ends the same
    assert drt.triEdgeAdjacency(np.zeros((0, 3, 3), np.float32)).shape == (0, 3)
    for bad in (np.zeros((2, 3, 3), np.float64), np.zeros((2, 9), np.float32), [[0.0] * 12]):
        with pytest.raises(drt.DrtError) as e:
            drt.triEdgeAdjacency(bad)
        assert e.value.code == drt.ERR_INVALID


@pytest.mark.parametrize("name", ["spheres1", "aligned_x", "tube_quad", "tube_flipped", "strip", "book", "poke"])
def test_the_query_table_is_the_scene_s_rule_and_the_restatement_s(name):
    pos, tris = cv.case(name)
    sc, _ = cs.flat_scene(drt, pos)
    own = cs.tree_positions(sc)                                                # the scene's own triangles in tree order
    got = drt.triEdgeAdjacency(own)
    assert got.dtype == np.int32 and got.shape == (len(own), 3) and got.tobytes() == sc.edgeAdjacency().tobytes(), name
    got = drt.triEdgeAdjacency(tris)
    assert got.tobytes() == cu.tri_adjacency(tris).tobytes(), name
    packed = np.full((len(tris), 12), np.nan, np.float32)                       # the pad is not read
    packed[:, 0:9] = tris.reshape(-1, 9)
    assert drt.triEdgeAdjacency(packed).tobytes() == got.tobytes(), name
    if name == "tube_flipped":
        assert (got == -2).sum() == 2 and (got == -1).sum() == 4
    if name == "spheres1":
        assert (got >= 0).all() and (got.reshape(-1)[got.reshape(-1)] == np.arange(got.size)).all()      # closed: an involution


def test_the_header_states_the_rule_its_limits_and_its_place():
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    sec = text[text.index("intersection curves (new"):text.index("int           drt_tri_edge_adjacency")]
    for title in ("sphere casts (new", "mesh topology (new", "plane sections (new", "triangle overlap queries (new", "section contours (new",
                  "box overlap queries (new", "triangle intersection segments (new", "typedef struct"):
        assert title not in sec, title
    flat = re.sub(r"\s*\n \*\s*", " ", sec)
    for phrase in ("code = cp + 16 * cq names the edge each endpoint lies on", "edges 0..2 of the scene triangle, 4..6 of the query",
                   "the segment runs from p to q along cross(nq, nt)", "continues in the twin scene triangle with the same query",
                   "continues in the same scene triangle with the twin query", "No coordinate is compared, no tolerance is chosen",
                   "tris and out are HOST pointers", "out receives 3 * n values", "drt_scene_edge_adjacency's, word for word",
                   "the pad is not read", "half-edge 3 * i + e runs from vertex e to vertex (e + 1) % 3 of query i",
                   "the same iff their three words are bit-equal", "twins, -1 and -2 as there", "no order other than the caller's",
                   "splits (n + 1 values), query_adj (3 * n values), slots (total entries) and counts (3 words, may be NULL)",
                   "the one drt_renderer_chain_sections makes and drops", "clamped exactly as drt_renderer_chain_sections clamps it",
                   "a decreasing pair is an empty range", "nothing beyond total is read or written",
                   "records in ascending prim, followed by any miss records", "lo = mid + 1 if splits[mid] <= j, else hi = mid",
                   "j is owned by query lo - 1 iff lo > 0 and j lies in that query's range",
                   "a record is live iff it has an owner, 0 <= prim < n_triangles", "are in {0, 1, 2, 4, 5, 6}",
                   "has no successor, takes no predecessor, and gets exit status 5", "If cq < 4: a = adj[3 * T + cq]",
                   "the target prim is a / 3 and the required entry code is a % 3", "If cq >= 4: a = query_adj[3 * i + cq - 4]",
                   "the target range is query a / 3, the target prim is T and the required entry code is 4 + a % 3",
                   "a value with a / 3 >= n is treated as -2", "a == -1: exit status 1", "a == -2: exit status 2",
                   "lo = mid + 1 if prim_mid < target, else hi = mid", "or m is not live, or m's owner is not the target query: exit status 3",
                   "(code_m & 15) is not the required entry code: exit status 4", "succ(j) = m, exit status 0", "succ is injective",
                   "the one of smallest index keeps it and the others get exit status 3", "simple paths and simple cycles on any input",
                   "every index written is below total", "one order over the whole list, because a curve crosses queries",
                   "A path starts at its record without a predecessor", "a cycle starts at its record of smallest index, and is closed",
                   "A record that is not live is a chain of one", "ordered by the ascending index of their first record",
                   "bit 0 = the chain is closed, bits 1..3 = that record's exit status", "Every slot below total is written",
                   "counts = {chains of live records, closed ones among them, records that are not live}",
                   "depends on segs, splits and the two tables only", "n == 0 or total == 0 is DRT_OK with no launch",
                   "with query_adj checked where splits is", "counters, kernel info and kernel span are not touched"):
        assert phrase in flat, phrase
    limits = flat[flat.index("What this is not:"):]
    for phrase in ("no welding and no new points", "plus the last q of an open chain", "statuses 3 and 4 mark the places where they do not",
                   "falls into open chains", "self-intersection curves are not chained", "no clipped polygons and no boolean", "no RendererGroup",
                   "nothing on the command line"):
        assert phrase in limits, phrase
    before = text[:text.index("#define DRT_ABI_VERSION 2")]
    assert "drt_tri_edge_adjacency" in before and "drt_renderer_chain_intersections" in before
    # after the records it chains and after the sphere casts: the block in front keeps its one comment
    assert text.index("typedef struct drt_isect ") < text.index("typedef struct drt_sweep_hit") < text.index("intersection curves (new")
    assert text.index("drt_renderer_chain_intersections(drt_renderer") < text.index("first-hit guide buffers")
    between = text[text.index("drt_renderer_intersect_triangles(drt_renderer"):text.index("sphere casts (new")]
    assert between.count("/*") == 1
    # the call that fills the list still says that it does not chain
    isect = re.sub(r"\s*\n \*\s*", " ", text[text.index("triangle intersection segments (new"):text.index("typedef struct drt_isect ")])
    assert "the segments are not chained into curves" in isect


def test_cpp_wrappers_compile_and_link(tmp_path):
    src = tmp_path / "curve_calls.cpp"
    src.write_text(r"""
#include <cstdio>
#include "DustRayTracer.hpp"
// the statements that need a device only -- main() runs none of them without arguments
int main(int argc, char **) {
    drt_tri tris[2] = { { { { 0, 0, 0 }, { 1, 0, 0 }, { 1, 1, 0 } }, { 0, 0, 0 } }, { { { 0, 0, 0 }, { 1, 1, 0 }, { 0, 1, 0 } }, { 0, 0, 0 } } };
    std::vector<int32_t> adj = TriEdgeAdjacency(tris, 2u);
    if (argc < 2) {
        std::printf("%zu %zu %d", sizeof(drt_chain_slot), adj.size(), DRT_ABI_VERSION);
        for (int32_t v : adj) std::printf(" %d", v);
        std::printf("\n");
        return 0;
    }
    Scene scene;
    Renderer r(0);
    const drt_isect *segs = nullptr;
    const uint32_t *splits = nullptr;
    const int32_t *query_adj = nullptr;
    drt_chain_slot *slots = nullptr;
    uint32_t *counts = nullptr;
    r.ChainIntersections(scene, segs, splits, query_adj, slots, counts, 0u, 0u);
    r.ChainIntersections(scene, segs, splits, query_adj, slots, nullptr, 0u, 0u, nullptr);
    return 0;
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    exe = tmp_path / "curve_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib_dir, "-ldrt_hip",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["16", "6", "2", "-1", "-1", "3", "2", "-1", "-1"]


def test_the_routine_behind_both_tables_stands_alone(tmp_path):
    """tests/cpp/edge_adjacency_check.cpp: the factored routine over tight heap buffers in the three layouts, with nothing of the
    library linked (the program is what a sanitizer build runs; here it is built plainly)."""
    exe = tmp_path / "edge_adjacency_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "edge_adjacency_check.cpp"), "-o", str(exe)], check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.split() == ["ok", "8"], done.stdout


def test_bad_lists_are_refused_before_any_device_work():
    r = drt.Renderer.__new__(drt.Renderer)                                     # (no device: only the argument check runs)
    r._device = 0
    sc = drt.Scene()
    for bad in (None, (1, 2, 3), [np.zeros(1, np.int32)] * 5):
        with pytest.raises(drt.DrtError) as e:
            r.chainIntersections(sc, bad, query_adj=np.zeros((0, 3), np.int32))
        assert e.value.code == drt.ERR_INVALID
    lst = drt.CurveList(np.int32([0, 2, 3]), np.array([True, False]), np.float32([[0, 0, 0], [3, 0, 0], [1, 1, 1]]),
                        np.float32([[3, 0, 0], [3, 4, 0], [1, 1, 3]]), *([np.zeros(3, np.int32)] * 4))
    assert lst.lengths().dtype == np.float64 and lst.lengths().tolist() == [7.0, 2.0]
    empty = drt.CurveList(np.int32([0]), np.zeros(0, bool), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), *([np.zeros(0, np.int32)] * 4))
    assert empty.lengths().shape == (0,)
