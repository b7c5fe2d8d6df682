// kernel_overlap.hip -- box overlap queries for gfx950: the triangles that touch each query box, an oriented box given as centre, half
// extents and three axes, in ascending triangle index, the first cap_i of them stored in the box's own segment of `prims`
// (drt_renderer_overlap_boxes).  The reference has no such query; include/drt.h states the rule, and every line below that computes
// a value cites the part of it that it implements (the arithmetic itself is in overlap.hpp).
//
//   bounds     ext[j] = (|axis[0][j]| half[0] + |axis[1][j]| half[1]) + |axis[2][j]| half[2], qmin = center - ext, qmax = center + ext,
//              once per query
//   cull       a node's box passes iff qmin[j] <= bmax[j] && bmin[j] <= qmax[j] on all three axes; a NaN bound fails, so a NaN query
//              fails at the root and lists nothing
//   traversal  the root is tested against the scene's root box, an interior node pushes each child that passes, child 2 first, a
//              leaf's triangles in order.  Each triangle lies in one leaf and the cull is constant, so the SET of listed triangles
//              does not depend on the order, and neither does the list: it is sorted by triangle index.
//   listed     Akenine-Moller's 13 separating axes in the box's frame on the stored (v0, e1, e2); touching counts.  No alpha test.
//   segment    list_hits': cap = offsets[i+1] > offsets[i] ? the difference : 0, clamped so that offsets[i] + cap <= prims_capacity;
//              slots 0 .. min(cap, total) - 1 the list, the rest of the cap slots -1; counts[i] = total.  Mode ANY has no segment:
//              the traversal ends at the first listed triangle and counts[i] is 0 or 1.
//
// Grid, claim and stack: query_frame.hpp.  One box per lane; stack entries ref, kRqLdsLevelsOccluded levels in LDS.
//
// Registers: a lane keeps the whole query -- the 15 floats of the box and its six world bounds -- for as long as it owns the box.
// The compiler's resource remarks give 57 VGPRs (ANY) and 64 (LIST), no scratch and no VGPR spills under the 64 of 8 waves per SIMD;
// reading the box's 64 bytes again at each leaf gives the same two numbers, because the peak is inside the triangle test, where the
// box is live either way, so the second read would buy nothing; and a lower occupancy bound does not change them either.
//
// The list: a box's segment in global memory IS its sorted list, 4-byte records.  The lane keeps base, cap, stored, total and, once
// stored == cap, the last stored index in a register, so a candidate that is not before the tail of a full list touches no memory.
// Any other candidate is inserted from the back: records move up by one slot while the candidate is smaller, and a full list drops
// its last record.  Only the owning lane reads or writes a segment, with plain vector loads and stores: no fences.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "device_scene.hpp"
#include "device_access.hpp"
#include "overlap.hpp"
#include "query_frame.hpp"

namespace drt {

namespace {

template <bool ANY>
__global__ __launch_bounds__(kRqThreads, kRqWavesPerSimd) void overlap_kernel(const SceneView sc, const OverlapArgs a) {
    constexpr int K = kRqLdsLevelsOccluded;
    __shared__ uint32_t s_ref[K][kRqThreads];
    const int tid = threadIdx.x;
    const uint32_t gthread = blockIdx.x * kRqThreads + tid;
    const StackLane st = {tid, gthread, gridDim.x * kRqThreads, a.frame.stack_levels, a.frame.stack_hbm};
    uint32_t shard = home_shard(gthread);
    int shards_empty = 0;

    int rid = -1;                                            // this lane's box, -1 = idle
    f3 qmin = mk3(0.f, 0.f, 0.f), qmax = mk3(0.f, 0.f, 0.f); // its world bounds
    uint32_t base = 0, cap = 0;                              // the box's segment: prims[base .. base + cap)
    uint32_t stored = 0, total = 0;                          // records in the segment (<= cap), listed triangles so far
    int tail = 0;                                            // prims[base + cap - 1], valid once stored == cap
    OverlapBox box = {};                                     // the query itself: only a leaf's triangle test reads it
    uint32_t sp = 0;

    for (;;) {
        // ---- refill: claim boxes for the idle lanes (wave-uniform) ----
        const uint64_t idle = __ballot(rid < 0);
        if (claim_due(shards_empty, idle, a.frame)) {
            const bool was_idle = rid < 0;
            const Claimed c = claim_take(shard, shards_empty, rid, idle, a.frame);
            shard = c.shard; shards_empty = c.shards_empty; rid = c.rid;
            if (was_idle && rid >= 0) {
                // a new box: four 16-byte loads (drt_box) for its world bounds, and in mode LIST the two offsets of its segment
                box = overlap_load_box(a.boxes, (uint32_t)rid);
                const f3 ext = overlap_extent(box);
                qmin = box.center - ext; qmax = box.center + ext;
                base = 0; cap = 0;
                if (!ANY) {
                    // cap = offsets[i+1] > offsets[i] ? the difference : 0, clamped so that offsets[i] + cap <= prims_capacity
                    const uint32_t o0 = a.offsets[(uint32_t)rid], o1 = a.offsets[(uint32_t)rid + 1u];
                    base = o0;
                    cap = o1 > o0 ? o1 - o0 : 0u;
                    const uint32_t room = o0 < a.prims_capacity ? a.prims_capacity - o0 : 0u;
                    cap = cap < room ? cap : room;
                }
                stored = 0; total = 0; sp = 0;
                // the root is tested against the scene's root box
                if (sc.root_ref != kNoNode && overlap_cull_passes(qmin, qmax, ld3(sc.root_min), ld3(sc.root_max))) {
                    s_ref[0][tid] = sc.root_ref; sp = 1;
                }
            }
        }
        if (claim_drained(shards_empty, rid)) break;

        // ---- one traversal step per busy lane ----
        if (rid >= 0 && sp > 0) {
            const uint32_t ref = stack_pop(s_ref, st, sp);
            if (ref & kLeafBit) {
                const LeafRange leaf = sc.leaves[ref & ~kLeafBit];
                for (int i = leaf.start; i < leaf.start + leaf.count; i++) {
                    const TriTest tri = load_tri(sc.tri_hot, i);
                    if (!overlap_triangle(box, tri.v0, tri.e1, tri.e2)) continue;       // listed iff none of the 13 axes separates
                    total++;
                    if (ANY) { sp = 0; break; }                                         // the traversal ends at the first listed triangle
                    // no room at all, or a full list whose tail the candidate does not come before: nothing touches memory
                    if (cap == 0u || (stored == cap && !(i < tail))) continue;
                    // the slot that opens: the next free one, or the last one of a full list (whose record is dropped)
                    uint32_t j = stored < cap ? stored++ : cap - 1u;
                    const bool is_tail = j == cap - 1u;                                 // what lands there is the new tail
                    int new_tail = i;
                    bool moved = false;
                    int32_t *const seg = a.prims + (size_t)base;
                    while (j > 0u) {                                                    // j <= cap - 1: inside the segment
                        const int32_t p = seg[j - 1u];
                        if (!(i < p)) break;
                        seg[j] = p;
                        if (!moved) { new_tail = p; moved = true; }
                        --j;
                    }
                    seg[j] = i;
                    if (is_tail) tail = new_tail;
                }
            } else {
                const ChildPair c = load_children(sc.inner, ref);
                const bool push1 = overlap_cull_passes(qmin, qmax, c.min1, c.max1);
                const bool push2 = overlap_cull_passes(qmin, qmax, c.min2, c.max2);
                stack_push(s_ref, st, sp, c.ref2, push2);                               // child 2 first
                stack_push(s_ref, st, sp, c.ref1, push1);
            }
        }

        // ---- a finished box: -1 behind its list, its total, and the lane is free ----
        if (rid >= 0 && sp == 0) {                                  // (rid < n: the claim never hands out more)
            if (!ANY)
                for (uint32_t j = stored; j < cap; j++) a.prims[(size_t)base + j] = -1;
            if (a.counts) a.counts[(uint32_t)rid] = total;
            rid = -1;
        }
    }
}

}  // namespace

hipError_t launch_overlap(const SceneView &sc, bool any_mode, const OverlapArgs &args, int num_cus, hipStream_t stream) {
    if (args.frame.n == 0) return hipSuccess;
    const uint32_t blocks = query_blocks(args.frame.n, num_cus);
    if (any_mode) hipLaunchKernelGGL(overlap_kernel<true>, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args);
    else hipLaunchKernelGGL(overlap_kernel<false>, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args);
    return hipGetLastError();
}

}  // namespace drt
