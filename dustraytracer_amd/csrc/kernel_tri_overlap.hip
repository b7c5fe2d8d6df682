// kernel_tri_overlap.hip -- triangle overlap queries for gfx950: the mesh triangles that each query triangle touches, in ascending
// triangle index, the first cap_i of them stored in the query's own segment of `prims` (drt_renderer_overlap_triangles).  The reference
// has no such query; include/drt.h states the rule, and every line below that computes a value cites the part of it that it
// implements (the arithmetic itself is in tri_overlap.hpp, the node cull in overlap.hpp).
//
//   validity   all nine coordinates satisfy fabsf(x) <= FLT_MAX; an invalid query pushes nothing and lists nothing
//   bounds     qmin[j] = min3(q0[j], q1[j], q2[j]), qmax likewise, once per query, exact
//   cull       the box query's: a node's box passes iff qmin[j] <= bmax[j] && bmin[j] <= qmax[j] on all three axes
//   traversal  the box query's: the root is tested against the scene's root box, an interior node pushes each child that passes,
//              child 2 first, a leaf's triangles in order.  The set of listed triangles does not depend on the order, and neither
//              does the list: it is sorted by triangle index.
//   listed     seventeen separating axes on the query and the stored (v0, e1, e2), relative to q0; touching counts
//   segment    drt_renderer_overlap_boxes': cap slots, the list, -1 behind it, counts[i] = total.  Mode ANY has no segment: the
//              traversal ends at the first listed triangle and counts[i] is 0 or 1.
//
// Grid, claim and stack: query_frame.hpp.  One query per lane; stack entries ref, kRqLdsLevelsOccluded levels in LDS.
//
// Registers: a lane keeps q0, a1, a2, g, nq and the six bounds -- 21 floats -- for as long as it owns the query.  The compiler's
// resource remarks give 82 VGPRs (ANY) and 89 (LIST), no scratch, no VGPR or SGPR spills, 5 waves per SIMD.  Under the 64 VGPRs of the
// other queries' 8 waves per SIMD the kernel does not fit: it spills 21 (ANY) and 30 (LIST) VGPRs to 80 and 112 bytes of scratch per
// lane, and no scratch is the requirement.  Tried at that bound, with the same spills each time: recomputing g and nq at the leaf
// instead of keeping them (the peak is inside the test, where they are live either way); seventeen early exits instead of three
// groups (as many VGPR spills, and 140 / 78 SGPR spills for the nested exec masks, which the groups bring to 0); a rolled loop over
// the axes (1 / 11 VGPR spills, but the runtime choice of A and E goes through 68 / 100 bytes of scratch).  Bounds of 7 and 6 waves
// still spill (72 VGPRs: 10 / 19 spilled; 80: 3 / 10); 5 is the first that does not, and 4 gives the same two numbers.  So the
// bound is 5 waves per SIMD, and the grid is 5 workgroups per CU.
//
// The list: kernel_overlap.hip's, record for record -- the segment in global memory IS the sorted list, 4-byte records, the owning
// lane alone reads and writes it with plain vector loads and stores, no fences.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "device_scene.hpp"
#include "device_access.hpp"
#include "tri_overlap.hpp"
#include "query_frame.hpp"

namespace drt {

namespace {

template <bool ANY>
__global__ __launch_bounds__(kRqThreads, kTriOverlapWavesPerSimd) void tri_overlap_kernel(const SceneView sc, const TriOverlapArgs a) {
    constexpr int K = kRqLdsLevelsOccluded;
    __shared__ uint32_t s_ref[K][kRqThreads];
    const int tid = threadIdx.x;
    const uint32_t gthread = blockIdx.x * kRqThreads + tid;
    const StackLane st = {tid, gthread, gridDim.x * kRqThreads, a.frame.stack_levels, a.frame.stack_hbm};
    uint32_t shard = home_shard(gthread);
    int shards_empty = 0;

    int rid = -1;                                            // this lane's query, -1 = idle
    f3 qmin = mk3(0.f, 0.f, 0.f), qmax = mk3(0.f, 0.f, 0.f); // its world bounds
    uint32_t base = 0, cap = 0;                              // the query's segment: prims[base .. base + cap)
    uint32_t stored = 0, total = 0;                          // records in the segment (<= cap), listed triangles so far
    int tail = 0;                                            // prims[base + cap - 1], valid once stored == cap
    TriOverlapQuery q = {};                                  // q0, a1, a2, g, nq: only a leaf's triangle test reads them
    uint32_t sp = 0;

    for (;;) {
        // ---- refill: claim queries for the idle lanes (wave-uniform) ----
        const uint64_t idle = __ballot(rid < 0);
        if (claim_due(shards_empty, idle, a.frame)) {
            const bool was_idle = rid < 0;
            const Claimed c = claim_take(shard, shards_empty, rid, idle, a.frame);
            shard = c.shard; shards_empty = c.shards_empty; rid = c.rid;
            if (was_idle && rid >= 0) {
                // a new query: three 16-byte loads (drt_tri), its bounds and edges, and in mode LIST the two offsets of its segment
                const TriOverlapVerts t = tri_overlap_load(a.tris, (uint32_t)rid);
                qmin = tri_overlap_min(t); qmax = tri_overlap_max(t);           // qmin[j] = min3(q0[j], q1[j], q2[j]): exact
                q = tri_overlap_query(t);
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
                // an invalid query (a coordinate with fabsf(x) > FLT_MAX or a NaN) pushes nothing; the root is tested against the
                // scene's root box
                if (tri_overlap_valid(t) && sc.root_ref != kNoNode && overlap_cull_passes(qmin, qmax, ld3(sc.root_min), ld3(sc.root_max))) {
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
                    if (!tri_overlap_triangle(q, tri.v0, tri.e1, tri.e2)) continue;     // listed iff none of the 17 axes separates
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

        // ---- a finished query: -1 behind its list, its total, and the lane is free ----
        if (rid >= 0 && sp == 0) {                                  // (rid < n: the claim never hands out more)
            if (!ANY)
                for (uint32_t j = stored; j < cap; j++) a.prims[(size_t)base + j] = -1;
            if (a.counts) a.counts[(uint32_t)rid] = total;
            rid = -1;
        }
    }
}

}  // namespace

hipError_t launch_tri_overlap(const SceneView &sc, bool any_mode, const TriOverlapArgs &args, int num_cus, hipStream_t stream) {
    if (args.frame.n == 0) return hipSuccess;
    const uint32_t blocks = query_blocks(args.frame.n, num_cus, kTriOverlapWavesPerSimd);
    if (any_mode) hipLaunchKernelGGL(tri_overlap_kernel<true>, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args);
    else hipLaunchKernelGGL(tri_overlap_kernel<false>, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args);
    return hipGetLastError();
}

}  // namespace drt
