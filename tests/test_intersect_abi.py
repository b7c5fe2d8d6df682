"""The intersection-segment entry point of include/drt.h without a GPU: exported, bound, laid out as declared, the argument checks that
come before any device work, the header states the rule, its limits and its place, and the C++ wrapper compiles and links against it."""
import ctypes
import os
import re
import subprocess

import pytest

from tests.scenes import ROOT

drt = pytest.importorskip("dustraytracer_amd")


def test_the_symbol_is_exported_and_bound():
    lib = ctypes.CDLL(drt.LIB_PATH)
    assert hasattr(lib, "drt_renderer_intersect_triangles")
    fn = drt._lib.drt_renderer_intersect_triangles
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 9
    assert fn.argtypes[5] is ctypes.c_uint32 and fn.argtypes[7] is ctypes.c_uint32                       # out_capacity, n
    assert all(fn.argtypes[i] is ctypes.c_void_p for i in (0, 1, 2, 3, 4, 6, 8))
    sections = drt._lib.drt_renderer_plane_sections.argtypes
    assert fn.argtypes == sections[:8] + sections[9:]                                                   # plane sections' without the mode
    for method in ("intersectTriangles", "selfIntersectionSegments"):
        assert callable(getattr(drt.Renderer, method)), method
    assert drt.CutList._fields == ("splits", "p", "q", "prim", "code") and drt.SelfCuts._fields == ("pairs", "p", "q", "code")
    doc = " ".join(drt.Renderer.selfIntersectionSegments.__doc__.split())
    assert "A pair that only touches in a common plane is in selfIntersections but not here" in doc
    assert "Not chained into curves" in drt.Renderer.intersectTriangles.__doc__
    assert drt._lib.drt_abi_version() == 2


def test_record_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "drt.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu\n", sizeof(drt_isect), offsetof(drt_isect, p), offsetof(drt_isect, prim), offsetof(drt_isect, q),
           offsetof(drt_isect, code));
    printf("%zu %d\n", sizeof(drt_tri), DRT_ABI_VERSION);
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["32", "0", "12", "16", "28", "48", "2"]


def test_the_argument_checks_are_plane_sections_in_its_order():
    L = drt._lib
    sc = drt.Scene()
    fn, sections = L.drt_renderer_intersect_triangles, L.drt_renderer_plane_sections
    assert fn(None, sc._h, None, None, None, 0, None, 4, None) == drt.ERR_INVALID
    assert b"null" in L.drt_last_error()
    assert fn(None, None, None, None, None, 0, None, 0, None) == drt.ERR_INVALID         # the handles are checked before n == 0
    # before the renderer is looked at: a block of zeros stands in for it
    stand_in = ctypes.create_string_buffer(1 << 16)
    h = ctypes.addressof(stand_in)
    assert fn(h, sc._h, None, None, None, 0, None, 0, None) == drt.OK                    # n == 0: nothing to do
    assert fn(h, sc._h, None, None, None, 0, None, 4, None) == drt.ERR_INVALID
    assert b"null triangle" in L.drt_last_error()
    # the pointer combinations, checked before anything is dereferenced: stand-in addresses, 16-byte aligned
    tris = ctypes.create_string_buffer(48 * 4 + 16)
    B = (ctypes.addressof(tris) + 15) & ~15
    words = ctypes.create_string_buffer(64)
    W = (ctypes.addressof(words) + 15) & ~15
    calls = (("without offsets", (B, None, W, 4, W, 4), b"null triangle or offset"), ("without tris", (None, W, W, 4, W, 4), b"null triangle or offset"),
             ("both outputs null", (B, W, None, 0, None, 4), b"both null"),
             ("null out with a capacity", (B, W, None, 4, W, 4), b"if and only if"), ("out without a capacity", (B, W, W, 0, W, 4), b"if and only if"),
             ("misaligned tris", (B + 4, W, W, 4, W, 4), b"aligned"), ("misaligned out", (B, W, W + 4, 4, W, 4), b"aligned"),
             ("misaligned offsets", (B, W + 1, W, 4, W, 4), b"aligned"), ("misaligned counts", (B, W, W, 4, W + 3, 4), b"aligned"),
             ("too many", (B, W, W, 4, W, 0x80000000), b"2^31 - 1"))
    for what, args, text in calls:
        assert fn(h, sc._h, *args, None) == drt.ERR_INVALID, what
        assert text in L.drt_last_error(), what
        # the same call gives plane sections in mode LIST the same code: one order of checks
        assert sections(h, sc._h, *args, 0, None) == drt.ERR_INVALID, what
    # two faults in one call: the earlier check answers, as it does there
    for args, text in (((None, W + 1, None, 0, None, 4), b"null"), ((B + 4, W, None, 0, None, 4), b"both null"), ((B + 4, W, None, 4, W, 4), b"if and only if")):
        assert fn(h, sc._h, *args, None) == drt.ERR_INVALID and text in L.drt_last_error()
        assert sections(h, sc._h, *args, 0, None) == drt.ERR_INVALID and text in L.drt_last_error()


def test_the_header_states_the_rule_its_limits_and_its_place():
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    sec = text[text.index("triangle intersection segments (new"):text.index("typedef struct drt_isect ")]
    for title in ("sphere casts (new", "mesh topology (new", "plane sections (new", "triangle overlap queries (new", "section contours (new",
                  "box overlap queries (new", "typedef struct drt_tri "):
        assert title not in sec, title
    flat = re.sub(r"\s*\n \*\s*", " ", sec)
    for phrase in ("a drt_tri with vertices q0, q1, q2, as for drt_renderer_overlap_triangles", "w0 = v0, w1 = v0 + e1, w2 = v0 + e2",
                   "fp32 with one rounding per operation, in the order written", "as the box-overlap block defines them",
                   "are drt_renderer_overlap_triangles', word for word", "all nine coordinates satisfy fabsf(x) <= FLT_MAX",
                   "pushes nothing and lists nothing", "qmin[j] = min3(q0[j], q1[j], q2[j])", "qmin[j] <= bmax[j] && bmin[j] <= qmax[j]",
                   "the root is tested against the scene's root box", "child 2 first", "a leaf's triangles are tested in order",
                   "a1 = q1 - q0, a2 = q2 - q0, nq = cross(a1, a2)", "p_k = w_k - q0, s_k = dot(nq, p_k)", "vertex k is above iff s_k >= 0",
                   "all three in one class: no record", "nt = cross(e1, e2); r_k = q_k - v0, u_k = dot(nt, r_k)", "above iff u_k >= 0",
                   "taken from the world vertex itself, not built as p_0 + e1", "depends on that vertex and the query alone",
                   "A coplanar pair, and a zero-area triangle on either side, are therefore all above and give no record",
                   "this is stricter than drt_renderer_overlap_triangles' predicate", "D = cross(nq, nt)",
                   "j = 0; if (fabsf(D[1]) > fabsf(D[0])) j = 1; if (fabsf(D[2]) > fabsf(D[j])) j = 2", "If !(fabsf(D[j]) > 0): no record",
                   "drt_renderer_plane_sections' cut(a, b)", "lo is the below vertex of the two and hi the above one", "t = s_lo / (s_lo - s_hi)",
                   "lo + (hi - lo) * t per component, on the world vertices", "apex k (the vertex alone in its class)",
                   "T1 = cut(k, k+1) lies on edge k and T2 = cut(k, k+2) lies on edge (k+2) % 3",
                   "edge e runs from vertex e to vertex (e+1) % 3, as drt_scene_edge_adjacency has it",
                   "Q1 and Q2 are built the same way from q_k and u_k", "(tl, th) = (T1, T2) if T1[j] <= T2[j], else (T2, T1)",
                   "lo = ql if ql[j] > tl[j] else tl; hi = qh if qh[j] < th[j] else th", "on a tie the scene's point is kept",
                   "A record exists iff lo[j] <= hi[j]", "touching counts, and a zero-length segment is listed",
                   "a NaN fails, and the pair is not listed", "if D[j] > 0 then p = lo and q = hi, otherwise p = hi and q = lo",
                   "the segment runs along cross(nq, nt)", "a drt_isect, 32 bytes, 16-byte aligned: p[3], prim, q[3], code",
                   "code = cp + 16 * cq", "the scene triangle's edge (0..2) for a point of T, or 4 + the query's edge for a point of Q",
                   "The miss record is all zeros with prim = -1", "Endpoints are never interpolated along the line",
                   "each one is one of the four cut points", "the same bits from both neighbours wherever their stored vertices agree",
                   "ascending triangle index, at most one record per pair", "are drt_renderer_plane_sections' in mode LIST",
                   "there is no mode argument", "counts[i] is the total, stored or not", "out is NULL iff out_capacity == 0: a pure count",
                   "a count with capacity 0, an exclusive scan of the counts into offsets, a fill", "DRT_ERR_UNSUPPORTED for a tree whose leaves",
                   "appended to and never inserted into", "counters, kernel info and kernel span",
                   "for non-coplanar triangles of non-zero area, a record exists iff the two closed triangles meet",
                   "only for pairs within rounding of touching", "D is a fourth power of coordinate differences",
                   "for 2^-24 to 2^32", "tests/test_intersect_ref.py asserts the figure"):
        assert phrase in flat, phrase
    limits = flat[flat.index("What this is not:"):]
    for phrase in ("the segments are not chained into curves", "separate segments in triangle order", "no clipped polygons and no boolean",
                   "coplanar overlaps give nothing", "no pair exclusion at this level", "it works there, one lane per query",
                   "tris and out are 16-byte aligned; offsets and counts 4-byte aligned"):
        assert phrase in limits, phrase
    assert "drt_renderer_intersect_triangles" in text[:text.index("#define DRT_ABI_VERSION 2")]
    # after the last mesh-topology declaration, directly before the sphere casts
    assert text.index("drt_renderer_topology_steps(const drt_renderer") < text.index("triangle intersection segments (new")
    assert text.index("drt_renderer_intersect_triangles(drt_renderer") < text.index("sphere casts (new")
    between = text[text.index("drt_renderer_intersect_triangles(drt_renderer"):text.index("sphere casts (new")]
    assert between.count("/*") == 1
    # the measured figure is the one the restatement's test asserts
    from tests.test_intersect_ref import SCALE_RANGE
    assert "for 2^%d to 2^%d" % SCALE_RANGE in flat


def test_cpp_wrapper_compiles_and_links(tmp_path):
    src = tmp_path / "intersect_calls.cpp"
    src.write_text(r"""
#include <cstdio>
#include "DustRayTracer.hpp"
// the statements only -- main() runs none of them without arguments
int main(int argc, char **) {
    if (argc < 2) { std::printf("%zu %zu %zu %d\n", sizeof(drt_tri), sizeof(drt_isect), alignof(drt_isect), DRT_ABI_VERSION); return 0; }
    Scene scene;
    Renderer r(0);
    const drt_tri *tris = nullptr;
    const uint32_t *offsets = nullptr;
    drt_isect *out = nullptr;
    uint32_t *counts = nullptr;
    r.IntersectTriangles(scene, tris, offsets, out, 0u, counts, 0u);
    r.IntersectTriangles(scene, tris, offsets, nullptr, 0u, counts, 0u, nullptr);
    return 0;
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    exe = tmp_path / "intersect_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib_dir, "-ldrt_hip",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["48", "32", "4", "2"]
