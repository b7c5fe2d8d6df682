// section_order.hpp -- the host's check that plane sections rest on (include/drt.h drt_renderer_plane_sections): whether the packed
// leaves, walked child 1 first, hold ascending triangle ranges.  Host code over device_scene.hpp only, so that a test can compile it
// on its own (tests/test_section_order.py).
#pragma once
#include <cstdint>
#include <vector>

#include "device_scene.hpp"

namespace drt {

// The leaves in the order the kernel's lists hold them -- child 1 before child 2, from the root -- start where the one before ended.
// The builder's split of [first, last) into [first, mid) and [mid, last) gives that; the kernel's lists are ascending only then.
// (Iterative: a tree may be as deep as it has leaves.  A reference outside the arrays, or more visits than the arrays have records,
// ends the walk with false: the scene's own validation has the say on such a tree, this walk only never calls it sorted.)
inline bool section_leaves_ascending(const PackedScene &ps) {
    if (ps.root_ref == kNoNode) return true;
    std::vector<uint32_t> stack{ ps.root_ref };
    size_t visits = 0;
    const size_t most = ps.inner.size() + ps.leaves.size();
    int64_t next = -1;                                          // where the next leaf has to start; -1 = anywhere (the first one)
    while (!stack.empty()) {
        const uint32_t ref = stack.back();
        stack.pop_back();
        if (++visits > most) return false;
        if (ref & kLeafBit) {
            const uint32_t id = ref & ~kLeafBit;
            if (id >= ps.leaves.size()) return false;
            const LeafRange &l = ps.leaves[id];
            if (l.count < 0 || (next >= 0 && l.start != next)) return false;
            next = (int64_t)l.start + l.count;
        } else {
            if (ref >= ps.inner.size()) return false;
            stack.push_back(ps.inner[ref].c2ref);               // child 1 is popped first
            stack.push_back(ps.inner[ref].c1ref);
        }
    }
    return true;
}

}  // namespace drt
