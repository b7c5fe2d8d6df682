// kernel_intersect.hip -- triangle intersection segments for gfx950: the segment along which each query triangle cuts each mesh triangle
// it crosses, one 32-byte record per cutting pair in ascending triangle index, the first cap_i of them stored in the query's own segment
// of `out` (drt_renderer_intersect_triangles).  The reference has no such query; include/drt.h states the rule, and every line below
// that computes a value cites the part of it that it implements (the arithmetic itself is in intersect.hpp, the load, validity and
// bounds of a query in tri_overlap.hpp, the node cull in overlap.hpp, the cut point in section.hpp).
//
//   validity   all nine coordinates satisfy fabsf(x) <= FLT_MAX; an invalid query pushes nothing and lists nothing
//   bounds     qmin[j] = min3(q0[j], q1[j], q2[j]), qmax likewise, once per query, exact
//   cull       a node's box passes iff qmin[j] <= bmax[j] && bmin[j] <= qmax[j] on all three axes
//   traversal  the root is tested against the scene's root box, an interior node pushes each child that passes, child 2 first, a
//              leaf's triangles in order
//   classes    s_k = dot(nq, w_k - q0) and u_k = dot(nt, q_k - v0); a pair whose three s or three u are in one class has no record
//   segment    D = cross(nq, nt), its largest axis j, the four cut points, the overlap of the two intervals on axis j, oriented along D
//   list       drt_renderer_plane_sections' in mode LIST: cap slots, the records, the miss record behind them, counts[i] = total
//
// Grid, claim and stack: query_frame.hpp.  One query per lane; stack entries ref, kRqLdsLevelsOccluded levels in LDS.
//
// The list is appended to and never inserted into: child 1 is popped before child 2, and the entry point refuses a tree whose leaves,
// child 1 first, do not hold ascending triangle ranges (leaves_ascending), so a query's records arrive in ascending triangle index.
// A record is two 16-byte vector stores by the owning lane, which alone touches its segment; no fences.
//
// Two instantiations: STORE = false is the count pass (out_capacity == 0): it reads no offsets and stores no record, but runs the whole
// rule, because whether a record exists is decided by the last comparison of the cut points.
//
// Registers: a lane keeps q0, q1, q2, nq and the six bounds -- 18 floats -- for as long as it owns the query.  The compiler's resource
// remarks give 60 VGPRs for the count pass at any bound: it runs at the 8 waves per SIMD of the other queries.  The fill keeps the two
// 16-byte words of the record and the segment's base and capacity as well: under 64 VGPRs (8 waves) it spills 26 VGPRs and 8 SGPRs to
// 76 bytes of scratch per lane, under 72 (7 waves) 8 VGPRs to 36 bytes, and no scratch is the requirement; 6 waves is the first bound
// that does not spill (80 VGPRs, no scratch, no VGPR or SGPR spills), and 5 gives the same numbers.  So the bounds are 8 waves per
// SIMD (count) and 6 (fill), and the grids are 8 and 6 workgroups per CU.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "device_scene.hpp"
#include "device_access.hpp"
#include "intersect.hpp"
#include "query_frame.hpp"

namespace drt {

namespace {

template <bool STORE>
__global__ __launch_bounds__(kRqThreads, STORE ? kIntersectFillWavesPerSimd : kIntersectCountWavesPerSimd) void intersect_kernel(const SceneView sc, const IntersectArgs a) {
    constexpr int K = kRqLdsLevelsOccluded;
    __shared__ uint32_t s_ref[K][kRqThreads];
    const int tid = threadIdx.x;
    const uint32_t gthread = blockIdx.x * kRqThreads + tid;
    const StackLane st = {tid, gthread, gridDim.x * kRqThreads, a.frame.stack_levels, a.frame.stack_hbm};
    uint32_t shard = home_shard(gthread);
    int shards_empty = 0;
    float4 *const out = reinterpret_cast<float4 *>(a.out);

    int rid = -1;                                            // this lane's query, -1 = idle
    f3 qmin = mk3(0.f, 0.f, 0.f), qmax = mk3(0.f, 0.f, 0.f); // its world bounds
    uint32_t base = 0, cap = 0;                              // the query's segment: out[base .. base + cap)
    uint32_t total = 0;                                      // records so far; the first min(total, cap) are stored
    IntersectQuery q = {};                                   // q0, q1, q2, nq: only a leaf's pair test reads them
    uint32_t sp = 0;

    for (;;) {
        // ---- refill: claim queries for the idle lanes (wave-uniform) ----
        const uint64_t idle = __ballot(rid < 0);
        if (claim_due(shards_empty, idle, a.frame)) {
            const bool was_idle = rid < 0;
            const Claimed c = claim_take(shard, shards_empty, rid, idle, a.frame);
            shard = c.shard; shards_empty = c.shards_empty; rid = c.rid;
            if (was_idle && rid >= 0) {
                // a new query: three 16-byte loads (drt_tri), its bounds and normal, and the two offsets of its segment
                const TriOverlapVerts t = tri_overlap_load(a.tris, (uint32_t)rid);
                qmin = tri_overlap_min(t); qmax = tri_overlap_max(t);           // qmin[j] = min3(q0[j], q1[j], q2[j]): exact
                q = intersect_query(t);
                base = 0; cap = 0;
                if (STORE) {
                    // cap = offsets[i+1] > offsets[i] ? the difference : 0, clamped so that offsets[i] + cap <= out_capacity
                    const uint32_t o0 = a.offsets[(uint32_t)rid], o1 = a.offsets[(uint32_t)rid + 1u];
                    base = o0;
                    cap = o1 > o0 ? o1 - o0 : 0u;
                    const uint32_t room = o0 < a.out_capacity ? a.out_capacity - o0 : 0u;
                    cap = cap < room ? cap : room;
                }
                total = 0; sp = 0;
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
                    float4 r0, r1;
                    if (!intersect_segment(q, tri.v0, tri.e1, tri.e2, i, r0, r1)) continue;
                    // an append: the records of a query arrive in ascending triangle index (total < cap: inside the segment)
                    if (STORE && total < cap) {
                        float4 *const rec = out + 2 * ((size_t)base + total);
                        rec[0] = r0; rec[1] = r1;
                    }
                    total++;
                }
            } else {
                const ChildPair c = load_children(sc.inner, ref);
                const bool push1 = overlap_cull_passes(qmin, qmax, c.min1, c.max1);
                const bool push2 = overlap_cull_passes(qmin, qmax, c.min2, c.max2);
                stack_push(s_ref, st, sp, c.ref2, push2);                               // child 2 first
                stack_push(s_ref, st, sp, c.ref1, push1);
            }
        }

        // ---- a finished query: the miss record behind its list, its total, and the lane is free ----
        if (rid >= 0 && sp == 0) {                                  // (rid < n: the claim never hands out more)
            if (STORE) {
                const float4 miss0 = make_float4(0.f, 0.f, 0.f, __int_as_float(-1)), miss1 = make_float4(0.f, 0.f, 0.f, 0.f);
                for (uint32_t j = total < cap ? total : cap; j < cap; j++) {
                    float4 *const rec = out + 2 * ((size_t)base + j);
                    rec[0] = miss0; rec[1] = miss1;
                }
            }
            if (a.counts) a.counts[(uint32_t)rid] = total;
            rid = -1;
        }
    }
}

}  // namespace

hipError_t launch_intersect(const SceneView &sc, const IntersectArgs &args, int num_cus, hipStream_t stream) {
    if (args.frame.n == 0) return hipSuccess;
    const bool fill = args.out_capacity != 0;
    const uint32_t blocks = query_blocks(args.frame.n, num_cus, fill ? kIntersectFillWavesPerSimd : kIntersectCountWavesPerSimd);
    if (fill) hipLaunchKernelGGL(intersect_kernel<true>, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args);
    else hipLaunchKernelGGL(intersect_kernel<false>, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args);
    return hipGetLastError();
}

}  // namespace drt
