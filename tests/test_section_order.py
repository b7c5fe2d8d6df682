"""The host's check behind the ascending lists of plane sections (csrc/section_order.hpp, section_leaves_ascending), compiled on its
own without a device: a tree as the builder splits it gives true; the same tree with the children of one node exchanged, a leaf that
does not start where the one before ended, and references outside the arrays give false.  The entry point answers DRT_ERR_UNSUPPORTED
on false, and the public interface cannot build such a tree, so this is where the false branch is seen."""
import os
import subprocess

from tests.scenes import ROOT

PROGRAM = r"""
#include <cstdio>
#include "section_order.hpp"
using namespace drt;

static InnerNode node(uint32_t c1, uint32_t c2) { InnerNode n = {}; n.c1ref = c1; n.c2ref = c2; return n; }
static uint32_t leaf(uint32_t id) { return kLeafBit | id; }

// [0, 7) split as the builder does: root = ([0, 3), [3, 7)); [0, 3) = ([0, 1), [1, 3)); [3, 7) = ([3, 5), [5, 7)).  The records
// are stored in no particular order: inner 0 = the right half, 1 = the left half, 2 = the root; the leaves likewise.
static PackedScene builder_tree() {
    PackedScene ps;
    ps.leaves = { {5, 2}, {0, 1}, {3, 2}, {1, 2} };
    ps.inner = { node(leaf(2), leaf(0)), node(leaf(1), leaf(3)), node(1, 0) };
    ps.root_ref = 2;
    return ps;
}

int main() {
    PackedScene empty;
    std::printf("%d", (int)section_leaves_ascending(empty));                   // no root: nothing to list
    PackedScene one;
    one.leaves = { {0, 4} };
    one.root_ref = leaf(0);
    std::printf(" %d", (int)section_leaves_ascending(one));                    // the root is a leaf
    PackedScene ps = builder_tree();
    std::printf(" %d", (int)section_leaves_ascending(ps));
    for (int which = 0; which < 3; which++) {                                  // the children of one node exchanged
        PackedScene sw = builder_tree();
        const uint32_t t = sw.inner[which].c1ref; sw.inner[which].c1ref = sw.inner[which].c2ref; sw.inner[which].c2ref = t;
        std::printf(" %d", (int)section_leaves_ascending(sw));
    }
    PackedScene gap = builder_tree();
    gap.leaves[2].start = 4; gap.leaves[2].count = 1;                          // [3, 5) became [4, 5): triangle 3 is in no leaf
    std::printf(" %d", (int)section_leaves_ascending(gap));
    PackedScene lap = builder_tree();
    lap.leaves[3].count = 3;                                                   // [1, 3) became [1, 4): it overlaps the next leaf
    std::printf(" %d", (int)section_leaves_ascending(lap));
    PackedScene first = builder_tree();
    first.leaves[1].start = 9;                                                 // the first leaf may start anywhere; the second must follow it
    std::printf(" %d", (int)section_leaves_ascending(first));
    PackedScene wild = builder_tree();
    wild.inner[0].c2ref = leaf(17);                                            // a leaf reference outside the array
    std::printf(" %d", (int)section_leaves_ascending(wild));
    wild = builder_tree();
    wild.inner[1].c1ref = 40;                                                  // an interior reference outside the array
    std::printf(" %d", (int)section_leaves_ascending(wild));
    PackedScene loop = builder_tree();
    loop.inner[0].c1ref = 2;                                                   // a cycle: the walk ends
    std::printf(" %d\n", (int)section_leaves_ascending(loop));
    return 0;
}
"""


def test_the_leaf_order_check_tells_builder_trees_from_exchanged_children(tmp_path):
    src = tmp_path / "order.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "order"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "dustraytracer_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()
    #              empty one  tree swap0 swap1 swap2 gap  lap  first wild wild loop
    assert out == ["1", "1", "1", "0", "0", "0", "0", "0", "0", "0", "0", "0"]


def test_the_entry_point_refuses_a_tree_the_check_rejects():
    """The one caller: drt_capi_section.cpp returns DRT_ERR_UNSUPPORTED when the uploaded scene's flag is false, and copy_scene sets the
    flag from the walk above whenever it packs a scene."""
    csrc = os.path.join(ROOT, "dustraytracer_amd", "csrc")
    entry = open(os.path.join(csrc, "drt_capi_section.cpp")).read()
    assert entry.index("upload_scene(r, scene)") < entry.index("if (!r->leaves_ascending)") < entry.index("launch_section(")
    assert "return fail(DRT_ERR_UNSUPPORTED" in entry[entry.index("if (!r->leaves_ascending)"):entry.index("hipStream_t s =")]
    assert "r->leaves_ascending = section_leaves_ascending(ps);" in open(os.path.join(csrc, "drt_capi.cpp")).read()
