// kernel_tri_distance.hip -- triangle distance queries for gfx950: the mesh triangle nearest each query triangle, its squared
// distance and a witness pair of points (drt_renderer_triangle_distance).  The reference has no such query; include/drt.h states the
// rule, and every line below that computes a value cites the part of it that it implements (the arithmetic itself is in
// tri_distance.hpp, tri_overlap.hpp and near_list.hpp).
//
//   validity   tri_overlap.hpp's: all nine coordinates satisfy fabsf(x) <= FLT_MAX; an invalid query pushes nothing: the miss record
//   bounds     qmin[j] = min3(q0[j], q1[j], q2[j]), qmax likewise, once per query, exact
//   node       per axis d = max(max(bmin - qmax, 0), qmin - bmax), box2 = (dx dx + dy dy) + dz dz
//   pair       fifteen candidates relative to q0 -- 3 query vertices against the scene triangle, 3 scene vertices against the query
//              triangle, 9 edge pairs -- the smallest is d2; if the seventeen axes of the overlap predicate do not separate the
//              pair, d2 = 0 and feature = candidate | 16
//   traversal  drt_renderer_nearest's: best = max_dist^2; a popped entry is dropped unless box2 < best; a leaf's triangles in order,
//              strict <; an interior node pushes each child with box2 < best, the farther one (b1 > b2 -> child 1) first.  Mode ANY
//              ends the query at the first pair with d2 < best.
//
// Grid, claim and stack: query_frame.hpp.  One query per lane; stack entries {ref, box2}, kRqLdsLevelsClosest levels in LDS.
//
// Registers: a lane keeps q0, a1, a2, g, nq and the six bounds -- 21 floats -- and best, prim and feature for as long as it owns the
// query; the witness is not kept but made again from (prim, candidate) when the query ends.  The table of what was tried is in
// DESIGN 5.27; the bound is kTriDistanceWavesPerSimd waves per SIMD, and the grid is that many workgroups per CU.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "device_scene.hpp"
#include "device_access.hpp"
#include "tri_distance.hpp"
#include "query_frame.hpp"

namespace drt {

namespace {

template <bool ANY>
__global__ __launch_bounds__(kRqThreads, kTriDistanceWavesPerSimd) void tri_distance_kernel(const SceneView sc, const TriDistanceArgs a) {
    constexpr int K = kRqLdsLevelsClosest;
    __shared__ uint32_t s_ref[K][kRqThreads];
    __shared__ float s_box2[K][kRqThreads];
    const int tid = threadIdx.x;
    const uint32_t gthread = blockIdx.x * kRqThreads + tid;
    const StackLane st = {tid, gthread, gridDim.x * kRqThreads, a.frame.stack_levels, a.frame.stack_hbm};
    uint32_t shard = home_shard(gthread);
    int shards_empty = 0;

    int rid = -1;                                            // this lane's query, -1 = idle
    f3 qmin = mk3(0.f, 0.f, 0.f), qmax = mk3(0.f, 0.f, 0.f); // its world bounds
    TriOverlapQuery q = {};                                  // q0, a1, a2, g, nq: only a leaf's pair test reads them
    float best = 0.f;                                        // the nearest so far (prim -1 = none): best = its d2, else max_dist^2
    int best_prim = -1, best_feature = 0;
    uint32_t sp = 0;

    for (;;) {
        // ---- refill: claim queries for the idle lanes (wave-uniform) ----
        const uint64_t idle = __ballot(rid < 0);
        if (claim_due(shards_empty, idle, a.frame)) {
            const bool was_idle = rid < 0;
            const Claimed c = claim_take(shard, shards_empty, rid, idle, a.frame);
            shard = c.shard; shards_empty = c.shards_empty; rid = c.rid;
            if (was_idle && rid >= 0) {
                // a new query: three 16-byte loads (drt_tri), its bounds and edges, and its max_dist (null: infinite)
                const TriOverlapVerts t = tri_overlap_load(a.tris, (uint32_t)rid);
                qmin = tri_overlap_min(t); qmax = tri_overlap_max(t);           // qmin[j] = min3(q0[j], q1[j], q2[j]): exact
                q = tri_overlap_query(t);
                const float md = a.max_dist ? a.max_dist[(uint32_t)rid] : __builtin_inff();
                best = md * md; best_prim = -1; best_feature = 0; sp = 0;
                // an invalid query (a coordinate with fabsf(x) > FLT_MAX or a NaN) pushes nothing; the root goes on the stack with
                // its box2: culled at its pop
                if (tri_overlap_valid(t) && sc.root_ref != kNoNode) {
                    s_ref[0][tid] = sc.root_ref; s_box2[0][tid] = tri_distance_box2(ld3(sc.root_min), ld3(sc.root_max), qmin, qmax); sp = 1;
                }
            }
        }
        if (claim_drained(shards_empty, rid)) break;

        // ---- one traversal step per busy lane ----
        if (rid >= 0 && sp > 0) {
            float box2;
            const uint32_t ref = stack_pop(s_ref, s_box2, st, sp, box2);
            if (box2 < best) {
                if (ref & kLeafBit) {
                    const LeafRange leaf = sc.leaves[ref & ~kLeafBit];
                    for (int i = leaf.start; i < leaf.start + leaf.count; i++) {
                        const TriTest tri = load_tri(sc.tri_hot, i);
                        int feature;
                        float d2 = tri_distance_candidates(q, tri.v0, tri.e1, tri.e2, feature);
                        // the seventeen axes do not separate the pair: it touches, whatever the candidates say
                        if (tri_overlap_triangle(q, tri.v0, tri.e1, tri.e2)) { d2 = 0.0f; feature |= 16; }
                        if (d2 < best) {                                                              // NaN never wins
                            best = d2; best_prim = i; best_feature = feature;
                            // mode ANY: the first pair within the distance; a pair that touches: nothing passes d2 < 0 or box2 < 0 any more
                            if (ANY || d2 == 0.0f) { sp = 0; break; }
                        }
                    }
                } else {
                    const ChildPair c = load_children(sc.inner, ref);
                    const float b1 = tri_distance_box2(c.min1, c.max1, qmin, qmax);
                    const float b2 = tri_distance_box2(c.min2, c.max2, qmin, qmax);
                    const bool push1 = b1 < best, push2 = b2 < best;
                    push_far_first(s_ref, s_box2, st, sp, c.ref1, b1, push1, c.ref2, b2, push2);        // farther child first
                }
            }
        }

        // ---- finished lanes write their result and go idle ----
        if (rid >= 0 && sp == 0) {                                  // (rid < n: the claim never hands out more)
            float4 o0 = make_float4(0.f, 0.f, 0.f, best), o1 = make_float4(0.f, 0.f, 0.f, __int_as_float(-1)), o2 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (best_prim >= 0) {
                // the witness is that of the winning (prim, candidate): the same operations on the same values as the test
                const TriTest tri = load_tri(sc.tri_hot, best_prim);
                f3 cq, ct;
                float u, v;
                tri_distance_witness(q, tri.v0, tri.e1, tri.e2, best_feature & 15, cq, ct, u, v);
                const f3 pq = q.q0 + cq, pt = q.q0 + ct;            // point_q = q0 + c_query, point_t = q0 + c_scene
                o0 = make_float4(pq.x, pq.y, pq.z, best);
                o1 = make_float4(pt.x, pt.y, pt.z, __int_as_float(best_prim));
                o2 = make_float4(u, v, __int_as_float(best_feature), 0.f);
            }
            float4 *out = reinterpret_cast<float4 *>(a.out) + 3 * (size_t)(uint32_t)rid;
            out[0] = o0; out[1] = o1; out[2] = o2;
            rid = -1; best_prim = -1;
        }
    }
}

}  // namespace

hipError_t launch_tri_distance(const SceneView &sc, bool any_mode, const TriDistanceArgs &args, int num_cus, hipStream_t stream) {
    if (args.frame.n == 0) return hipSuccess;
    const uint32_t blocks = query_blocks(args.frame.n, num_cus, kTriDistanceWavesPerSimd);
    if (any_mode) hipLaunchKernelGGL(tri_distance_kernel<true>, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args);
    else hipLaunchKernelGGL(tri_distance_kernel<false>, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args);
    return hipGetLastError();
}

}  // namespace drt
