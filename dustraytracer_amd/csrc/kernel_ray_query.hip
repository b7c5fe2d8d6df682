// kernel_ray_query.hip -- batched ray queries for gfx950: closest hit and occlusion for arrays of rays
// (drt_renderer_trace_rays / drt_renderer_occluded).
//
// Reference: TraceRay / RayTest (Kernel/TraceRay.cu:15-38) over traverseBVH / traverseBVH_raytest
// (BVH/BVHTraversal.cuh:14-134), with a per-ray interval [tmin, tmax] (include/drt.h states the contract):
//   closest   closest.t starts at tmax (TraceRay.cu:18); a popped node is culled by !(-1 < d && d < tmax) (:38 with the
//             interval (-1, tmax)); a triangle hit also needs t > tmin, tested before AnyHit (the reference's TODO at :37)
//   occluded  the root is skipped if d < 0 || d > tmax (:95-103), a child is pushed iff d >= 0 && !(d > tmax) (:122-129),
//             a triangle counts iff t > tmin && t < tmax && AnyHit (:107-115)
// The leaf arithmetic is the renderer's: make_ray, slab_intersect, tri_intersect_flat, any_hit, load_children, load_tri.
//
// Grid, claim and stack: query_frame.hpp.  One ray per lane; stack entries {ref, entry distance} (closest) or ref (occluded).
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "device_scene.hpp"
#include "device_access.hpp"
#include "query_frame.hpp"

namespace drt {

namespace {

template <bool OCC>
__global__ __launch_bounds__(kRqThreads, kRqWavesPerSimd) void ray_query_kernel(const SceneView sc, const RayQueryArgs a) {
    constexpr int K = OCC ? kRqLdsLevelsOccluded : kRqLdsLevelsClosest;
    __shared__ uint32_t s_ref[K][kRqThreads];
    __shared__ float s_dist[OCC ? 1 : K][kRqThreads];
    const int tid = threadIdx.x;
    const uint32_t gthread = blockIdx.x * kRqThreads + tid;
    const StackLane st = {tid, gthread, gridDim.x * kRqThreads, a.frame.stack_levels, a.frame.stack_hbm};
    uint32_t shard = home_shard(gthread);
    int shards_empty = 0;

    int rid = -1;                                            // this lane's ray, -1 = idle
    Ray ray;
    float tmin = 0.f, tmax = 0.f;
    float best_t = 0.f, best_u = 0.f, best_v = 0.f;          // closest: the hit so far (prim -1 = none)
    int best_prim = -1;
    bool occluded = false;
    uint32_t sp = 0;

    for (;;) {
        // ---- refill: claim rays for the idle lanes (wave-uniform) ----
        const uint64_t idle = __ballot(rid < 0);
        if (claim_due(shards_empty, idle, a.frame)) {
            const bool was_idle = rid < 0;
            const Claimed c = claim_take(shard, shards_empty, rid, idle, a.frame);
            shard = c.shard; shards_empty = c.shards_empty; rid = c.rid;
            if (was_idle && rid >= 0) {
                // a new ray: two 16-byte loads (drt_ray = org, tmin, dir, tmax)
                const float4 *r = reinterpret_cast<const float4 *>(a.rays) + 2 * (size_t)(uint32_t)rid;
                const float4 o = r[0], d = r[1];
                ray = make_ray(mk3(o.x, o.y, o.z), mk3(d.x, d.y, d.z));
                tmin = o.w; tmax = d.w;
                best_t = tmax; best_prim = -1; best_u = 0.f; best_v = 0.f;                         // TraceRay.cu:18
                if (sc.root_ref != kNoNode) {
                    const float droot = slab_intersect(ld3(sc.root_min), ld3(sc.root_max), ray);
                    if (OCC) {
                        if (!(droot < 0 || droot > tmax)) { s_ref[0][tid] = sc.root_ref; sp = 1; }   // :95-103 with tmax
                    } else {
                        s_ref[0][tid] = sc.root_ref; s_dist[0][tid] = droot; sp = 1;              // culled at its pop (:38)
                    }
                }
            }
        }
        if (claim_drained(shards_empty, rid)) break;

        // ---- one traversal step per busy lane ----
        if (rid >= 0 && sp > 0 && !occluded) {
            uint32_t ref;
            float dist = 0.f;
            if constexpr (OCC) ref = stack_pop(s_ref, st, sp);
            else ref = stack_pop(s_ref, s_dist, st, sp, dist);
            bool visit = true;
            if (!OCC) {
                if (!(-1.0f < dist && dist < tmax)) visit = false;                         // :38 interval (-1, tmax)
                else if (best_prim >= 0 && best_t < dist) visit = false;                   // :41
            }
            if (visit) {
                if (ref & kLeafBit) {
                    const LeafRange leaf = sc.leaves[ref & ~kLeafBit];
                    for (int i = leaf.start; i < leaf.start + leaf.count; i++) {            // :46-57 / :107-115
                        const TriTest tri = load_tri(sc.tri_hot, i);
                        float t, u, v;
                        const bool h = tri_intersect_flat(ray, tri.v0, tri.e1, tri.e2, t, u, v);
                        if (OCC) {
                            if (h && t > tmin && t < tmax && any_hit(sc, i, mk3(1.0f - u - v, u, v))) { occluded = true; break; }
                        } else if (h && t < best_t && t > tmin) {
                            if (!any_hit(sc, i, mk3(1.0f - u - v, u, v))) continue;
                            best_t = t; best_prim = i; best_u = u; best_v = v;
                        }
                    }
                } else {
                    const ChildPair c = load_children(sc.inner, ref);
                    const float d1 = slab_intersect(c.min1, c.max1, ray);
                    const float d2 = slab_intersect(c.min2, c.max2, ray);
                    bool push1, push2;
                    if (OCC) { push1 = d1 >= 0 && !(d1 > tmax); push2 = d2 >= 0 && !(d2 > tmax); }      // :122-129 with tmax
                    else { push1 = d1 >= 0 && d1 < best_t; push2 = d2 >= 0 && d2 < best_t; }             // :63-70
                    if constexpr (OCC) push_far_first(s_ref, st, sp, c.ref1, d1, push1, c.ref2, d2, push2);
                    else push_far_first(s_ref, s_dist, st, sp, c.ref1, d1, push1, c.ref2, d2, push2);
                }
            }
        }

        // ---- finished lanes write their result and go idle ----
        if (rid >= 0 && (sp == 0 || occluded)) {                    // (rid < n: the claim never hands out more)
            if (OCC) {
                reinterpret_cast<uint8_t *>(a.out)[(uint32_t)rid] = occluded ? 1 : 0;
            } else {
                const bool hit = best_prim >= 0;
                reinterpret_cast<float4 *>(a.out)[(uint32_t)rid] =
                    make_float4(best_t, __int_as_float(hit ? best_prim : -1), hit ? best_u : 0.f, hit ? best_v : 0.f);
            }
            rid = -1; sp = 0; occluded = false; best_prim = -1;
        }
    }
}

}  // namespace

hipError_t launch_ray_query(const SceneView &sc, bool occluded_query, const RayQueryArgs &args, int num_cus, hipStream_t stream,
                            const char **kernel_name) {
    if (args.frame.n == 0) return hipSuccess;
    const uint32_t blocks = query_blocks(args.frame.n, num_cus);
    if (occluded_query) {
        if (kernel_name) *kernel_name = "ray_query<occluded>";
        hipLaunchKernelGGL(ray_query_kernel<true>, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args);
    } else {
        if (kernel_name) *kernel_name = "ray_query<closest>";
        hipLaunchKernelGGL(ray_query_kernel<false>, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args);
    }
    return hipGetLastError();
}

}  // namespace drt
