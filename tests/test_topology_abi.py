"""The mesh-topology entry points of include/drt.h without a GPU: exported, bound, laid out as declared, the argument checks that come
before any device work in drt_renderer_chain_sections' order, the header states the rule, and the C++ wrappers compile and link."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import topology_ref as tr
from tests.scenes import ROOT

drt = pytest.importorskip("dustraytracer_amd")

NAMES = ("drt_renderer_shell_labels", "drt_renderer_boundary_loops", "drt_renderer_shell_terms", "drt_renderer_edge_adjacency",
         "drt_renderer_topology_steps")


def test_the_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(drt.LIB_PATH)
    P, U = ctypes.c_void_p, ctypes.c_uint32
    want = {"drt_renderer_shell_labels": [P, P, P, P, P], "drt_renderer_boundary_loops": [P, P, P, U, P, P],
            "drt_renderer_shell_terms": [P, P, P, P], "drt_renderer_edge_adjacency": [P, P, P, P], "drt_renderer_topology_steps": [P, P]}
    assert tuple(want) == NAMES
    for name, argtypes in want.items():
        assert hasattr(lib, name), name
        fn = getattr(drt._lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes == argtypes, name
    for method in ("shells", "boundaryLoops", "shellTerms", "shellMeasures", "topologySteps"):
        assert callable(getattr(drt.Renderer, method)), method
    assert drt.Shells._fields == ("label", "index", "count", "triangles", "open_edges", "bad_edges", "watertight")
    assert drt.LoopList._fields == ("splits", "closed", "half_edge", "prim", "edge", "shell", "end")
    assert drt.ShellMeasures._fields == ("area", "volume", "area_vector")
    assert drt._lib.drt_abi_version() == 2


def test_slot_and_term_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "drt.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu\n", sizeof(drt_loop_slot), offsetof(drt_loop_slot, half_edge), offsetof(drt_loop_slot, first),
           offsetof(drt_loop_slot, length), offsetof(drt_loop_slot, flags));
    printf("%zu %zu %zu %zu\n", sizeof(drt_shell_term), offsetof(drt_shell_term, c), offsetof(drt_shell_term, w), sizeof(double));
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0].split() == ["16", "0", "4", "8", "12"] and out[1].split() == ["32", "0", "24", "8"]
    assert tr.SLOT.itemsize == 16 and [tr.SLOT.fields[f][1] for f in ("half_edge", "first", "length", "flags")] == [0, 4, 8, 12]
    assert tr.TERM.itemsize == 32 and [tr.TERM.fields[f][1] for f in ("c", "w")] == [0, 24]


def test_the_argument_checks_come_in_the_chain_query_s_order():
    """The handles, the NULL pointers, the alignment and the capacity, before anything touches a device."""
    L = drt._lib
    sc = drt.Scene()
    INV = drt.ERR_INVALID
    labels, loops, terms, table, steps = (getattr(L, name) for name in NAMES)
    stand_in = ctypes.create_string_buffer(1 << 16)                              # a block of zeros stands in for the renderer
    h = ctypes.addressof(stand_in)
    buf = ctypes.create_string_buffer(256)
    B = (ctypes.addressof(buf) + 15) & ~15
    # the handles come first
    for call in (lambda r, s: labels(r, s, B, B, None), lambda r, s: loops(r, s, B, 4, B, None), lambda r, s: terms(r, s, B, None),
                 lambda r, s: table(r, s, B, None)):
        assert call(None, sc._h) == INV and b"null argument" in L.drt_last_error()
        assert call(h, None) == INV and b"null argument" in L.drt_last_error()
    assert steps(None, B) == INV and steps(h, None) == INV
    # the NULL pointers, before the alignment
    assert labels(h, sc._h, None, B + 1, None) == INV and b"null label" in L.drt_last_error()
    assert loops(h, sc._h, B + 4, 4, None, None) == INV and b"null count" in L.drt_last_error()
    assert terms(h, sc._h, None, None) == INV and b"null term" in L.drt_last_error()
    assert table(h, sc._h, None, None) == INV and b"null adjacency" in L.drt_last_error()
    # slots NULL iff capacity == 0
    assert loops(h, sc._h, None, 4, B, None) == INV and b"null iff" in L.drt_last_error()
    assert loops(h, sc._h, B, 0, B, None) == INV and b"null iff" in L.drt_last_error()
    assert loops(h, sc._h, None, 4, B + 1, None) == INV and b"null iff" in L.drt_last_error()      # ... before the alignment
    # the alignment: labels and counts 4 bytes, slots and terms 16
    for what, call in (("labels", lambda: labels(h, sc._h, B + 2, B, None)), ("label counts", lambda: labels(h, sc._h, B, B + 1, None)),
                       ("slots", lambda: loops(h, sc._h, B + 8, 4, B, None)), ("loop counts", lambda: loops(h, sc._h, B, 4, B + 2, None)),
                       ("loop counts, counting", lambda: loops(h, sc._h, None, 0, B + 3, None)), ("terms", lambda: terms(h, sc._h, B + 8, None)),
                       ("table", lambda: table(h, sc._h, B + 1, None))):
        assert call() == INV, what
        assert b"aligned" in L.drt_last_error(), what
    # fewer than 2^31 slots, after the alignment
    assert loops(h, sc._h, B, 0x80000000, B, None) == INV and b"slots per call" in L.drt_last_error()
    assert loops(h, sc._h, B + 4, 0x80000000, B, None) == INV and b"aligned" in L.drt_last_error()
    # the steps of a renderer that never labelled
    out = np.full(3, 7, np.uint32)
    assert steps(h, out.ctypes.data) == drt.OK and out.tolist() == [0, 0, 0]


def test_the_header_states_the_rule():
    text = open(os.path.join(ROOT, "include", "drt.h")).read()
    sec = text[text.index("mesh topology (new"):text.index("typedef struct drt_loop_slot ")]
    assert "sphere casts (new" not in sec and "section contours (new" not in sec
    flat = re.sub(r"\s*\n \*\s*", " ", sec)
    for phrase in ("Everything is in tree order", "adj is the table of drt_scene_edge_adjacency, exactly as it stands",
                   "any correct method gives the same bytes", "joined iff adj[3 * t + e] >= 0 and adj[3 * t + e] / 3 == t' for some e",
                   "A boundary edge (-1) and a non-manifold, flipped or zero-length edge (-2) join nothing",
                   "the three leaves of a book are three shells", "triangles that share only a vertex are separate shells",
                   "label[t] is the smallest triangle index of t's connected component", "counts = {shells, open half-edges, bad half-edges}",
                   "a shell is watertight iff both are zero", "the half-edges h = 3 * t + e with adj[h] == -1, in ascending h",
                   "runs from vertex e to vertex b = (e + 1) % 3 of t", "rotating about b through the adjacency; no coordinate is read",
                   "Start with g = 3 * t + (e + 1) % 3", "While adj[g] >= 0: g' = adj[g], t' = g' / 3, e' = g' % 3, g = 3 * t' + (e' + 1) % 3",
                   "If adj[g] == -1 then succ(h) = g", "If adj[g] == -2 the record has no successor and its exit status is 2",
                   "0 = linked, 2 = non-manifold or flipped", "twins pair half-edges one to one", "a path of degree at most 2",
                   "starts at an end of it and cannot cycle", "ends within the valence of b", "a step guard of 3 * n_triangles and treats its expiry as status 2",
                   "succ is injective", "simple paths and simple cycles", "a path starts at its record without a predecessor",
                   "a cycle starts at its smallest h, and is closed", "the loops are ordered by their first record",
                   "a loop carries that shell's label", "half_edge = the h that stands there", "first = the position of its loop's first record",
                   "bit 0 = the loop is closed, bits 1..3 = that record's exit status", "counts = {records, loops, closed loops}",
                   "a too small capacity truncates, and counts still holds the true numbers", "slots is NULL iff capacity == 0: a pure count",
                   "one 32-byte record per triangle", "after a device-only drt_renderer_refit these are the refitted positions",
                   "each component as a * b - c * d", "c.x = e1.y e2.z - e1.z e2.y, c.y = e1.z e2.x - e1.x e2.z, c.z = e1.x e2.y - e1.y e2.x",
                   "w = (v0.x * c.x + v0.y * c.y) + v0.z * c.z", "Every product and sum is rounded on its own, no contraction, no square root",
                   "The record is {c.x, c.y, c.z, w}", "dot(v0, cross(v0 + e1, v0 + e2)) == dot(v0, cross(e1, e2)) in exact arithmetic",
                   "w / 6 summed over a shell is its signed volume", "|c| / 2 is a triangle's area", "near zero for a watertight shell",
                   "depend on adj only", "keeps them beside its copy of adj across device refits, and drops them with that upload",
                   "no joining across non-manifold edges or by shared vertices", "no Euler characteristic, genus or vertex welding",
                   "no orientation repair", "the other queries are not filtered by shell", "no RendererGroup", "nothing on the command line",
                   "DRT_ERR_DEVICE if the labelling does not settle within its bound on steps",
                   "A scene without triangles is DRT_OK with zero counts", "counters, kernel info and kernel span are not touched"):
        assert phrase in flat, phrase
    # directly after the contours' declarations, before the sphere casts
    assert text.index("drt_renderer_chain_sections(drt_renderer") < text.index("mesh topology (new") < text.index("sphere casts (new")


def test_cpp_wrappers_compile_and_link(tmp_path):
    src = tmp_path / "topology_calls.cpp"
    src.write_text(r"""
#include <cstdio>
#include "DustRayTracer.hpp"
// the statements only -- main() runs none of them without arguments
int main(int argc, char **) {
    if (argc < 2) { std::printf("%zu %zu %zu %d\n", sizeof(drt_loop_slot), alignof(drt_loop_slot), sizeof(drt_shell_term), DRT_ABI_VERSION); return 0; }
    Scene scene;
    Renderer r(0);
    int32_t *labels = nullptr;
    uint32_t *counts = nullptr;
    drt_loop_slot *slots = nullptr;
    double *terms = nullptr;
    r.ShellLabels(scene, labels);
    r.ShellLabels(scene, labels, counts, nullptr);
    r.BoundaryLoops(scene, slots, 0u, counts);
    r.BoundaryLoops(scene, slots, 0u, counts, nullptr);
    r.ShellTerms(scene, terms);
    r.ShellTerms(scene, terms, nullptr);
    return 0;
}
""")
    lib_dir = os.path.dirname(drt.LIB_PATH)
    exe = tmp_path / "topology_calls"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib_dir, "-ldrt_hip",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["16", "4", "32", "2"]
