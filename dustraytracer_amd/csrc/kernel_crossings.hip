// kernel_crossings.hip -- crossing counts for gfx950: every triangle a ray passes through, and what follows from the count -- the
// inside vote of a point and the sign of a nearest record (drt_renderer_crossings / _inside / _signed_distance).  The reference
// has no such query; include/drt.h states the rule, and every line below that computes a value cites the part of it that it
// implements.
//
//   crossing   tri_intersect_flat's test (crossings.hpp restates it with det handed out); a triangle counts iff it hits,
//              t > tmin and t < tmax; count += 1, winding += det < 0 ? +1 : -1.  No alpha test.
//   traversal  drt_renderer_occluded's without the early exit: the root is skipped if d < 0 || d > tmax, a child is pushed iff
//              d >= 0 && !(d > tmax), the farther one first.  Each triangle lies in one leaf: the order does not matter.
//   vote       three rays from the point, tmin = 0, tmax = +inf, directions kInsideDirs; ray j votes inside iff count_j is odd
//              (rule 0) or winding_j != 0 (rule 1); the answer is the number of votes, inside = 2 or more
//
// Grid, claim and stack: query_frame.hpp.  One query per lane; stack entries ref, kRqLdsLevelsOccluded levels in LDS.
//
// Point mode keeps a lane on its point for all three rays: when the stack empties the lane banks the ray's vote in a register and
// starts the next direction on the same trip, and it stores once, after the third.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "device_scene.hpp"
#include "device_access.hpp"
#include "crossings.hpp"
#include "query_frame.hpp"

namespace drt {

namespace {

DRT_DEV f3 inside_dir(int j) {
    return mk3(j == 0 ? kInsideDirs[0][0] : (j == 1 ? kInsideDirs[1][0] : kInsideDirs[2][0]),
               j == 0 ? kInsideDirs[0][1] : (j == 1 ? kInsideDirs[1][1] : kInsideDirs[2][1]),
               j == 0 ? kInsideDirs[0][2] : (j == 1 ? kInsideDirs[1][2] : kInsideDirs[2][2]));
}

template <bool POINTS>
__global__ __launch_bounds__(kRqThreads, kRqWavesPerSimd) void crossings_kernel(const SceneView sc, const CrossingsArgs a, const CrossingsOut kind) {
    constexpr int K = kRqLdsLevelsOccluded;
    __shared__ uint32_t s_ref[K][kRqThreads];
    const int tid = threadIdx.x;
    const uint32_t gthread = blockIdx.x * kRqThreads + tid;
    const StackLane st = {tid, gthread, gridDim.x * kRqThreads, a.frame.stack_levels, a.frame.stack_hbm};
    uint32_t shard = home_shard(gthread);
    int shards_empty = 0;

    int rid = -1;                                            // this lane's query, -1 = idle
    Ray ray;
    float tmin = 0.f, tmax = 0.f;
    uint32_t count = 0;                                      // of the ray under way
    int winding = 0;
    int dir_index = 0;                                       // point mode: which of the three rays is under way,
    uint32_t votes = 0;                                      //   and the rays before it that voted inside
    uint32_t sp = 0;

    // a ray starts: its counts are zero and the root goes on the stack unless d < 0 || d > tmax (occluded's root rule)
    auto start_ray = [&](f3 org, f3 dir) {
        ray = make_ray(org, dir);
        count = 0; winding = 0; sp = 0;
        if (sc.root_ref != kNoNode) {
            const float droot = slab_intersect(ld3(sc.root_min), ld3(sc.root_max), ray);
            if (!(droot < 0 || droot > tmax)) { s_ref[0][tid] = sc.root_ref; sp = 1; }
        }
    };

    for (;;) {
        // ---- refill: claim queries for the idle lanes (wave-uniform) ----
        const uint64_t idle = __ballot(rid < 0);
        if (claim_due(shards_empty, idle, a.frame)) {
            const bool was_idle = rid < 0;
            const Claimed c = claim_take(shard, shards_empty, rid, idle, a.frame);
            shard = c.shard; shards_empty = c.shards_empty; rid = c.rid;
            if (was_idle && rid >= 0) {
                if (POINTS) {
                    // a new point: one 16-byte load (drt_point = p, max_dist; max_dist is not used); the first of its three rays
                    const float4 q = reinterpret_cast<const float4 *>(a.in)[(uint32_t)rid];
                    tmin = 0.f; tmax = __builtin_inff();
                    dir_index = 0; votes = 0;
                    start_ray(mk3(q.x, q.y, q.z), inside_dir(0));
                } else {
                    // a new ray: two 16-byte loads (drt_ray = org, tmin, dir, tmax)
                    const float4 *r = reinterpret_cast<const float4 *>(a.in) + 2 * (size_t)(uint32_t)rid;
                    const float4 o = r[0], d = r[1];
                    tmin = o.w; tmax = d.w;
                    start_ray(mk3(o.x, o.y, o.z), mk3(d.x, d.y, d.z));
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
                    float t, det;
                    const bool h = tri_intersect_det(ray, tri.v0, tri.e1, tri.e2, t, det);
                    if (h && t > tmin && t < tmax) { count++; winding += det < 0.0f ? 1 : -1; }
                }
            } else {
                const ChildPair c = load_children(sc.inner, ref);
                const float d1 = slab_intersect(c.min1, c.max1, ray);
                const float d2 = slab_intersect(c.min2, c.max2, ray);
                const bool push1 = d1 >= 0 && !(d1 > tmax), push2 = d2 >= 0 && !(d2 > tmax);
                push_far_first(s_ref, st, sp, c.ref1, d1, push1, c.ref2, d2, push2);            // farther child first
            }
        }

        // ---- a finished ray: the result (ray mode), or its vote and the point's next ray or result (point mode) ----
        if (rid >= 0 && sp == 0) {                                  // (rid < n: the claim never hands out more)
            if (POINTS) {
                votes += (a.rule != 0u ? winding != 0 : (count & 1u) != 0u) ? 1u : 0u;
                if (++dir_index < 3) {
                    start_ray(ray.orig, inside_dir(dir_index));     // (a ray that misses the root is finished on the next trip)
                } else {
                    if (kind == CrossingsOut::votes) reinterpret_cast<uint8_t *>(a.out)[(uint32_t)rid] = (uint8_t)votes;
                    else reinterpret_cast<float *>(a.out)[8 * (size_t)(uint32_t)rid + 7] = votes >= 2u ? -1.0f : 1.0f;
                    rid = -1;
                }
            } else {
                reinterpret_cast<uint2 *>(a.out)[(uint32_t)rid] = make_uint2(count, (uint32_t)winding);
                rid = -1;
            }
        }
    }
}

}  // namespace

hipError_t launch_crossings(const SceneView &sc, CrossingsOut kind, const CrossingsArgs &args, int num_cus, hipStream_t stream) {
    if (args.frame.n == 0) return hipSuccess;
    const uint32_t blocks = query_blocks(args.frame.n, num_cus);
    if (kind == CrossingsOut::crossings) hipLaunchKernelGGL(crossings_kernel<false>, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args, kind);
    else hipLaunchKernelGGL(crossings_kernel<true>, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args, kind);
    return hipGetLastError();
}

}  // namespace drt
