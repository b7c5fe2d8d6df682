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
// Shape: persistent grid (8 workgroups of 256 threads per CU = 8 waves per SIMD), one ray per lane, "while-while with
// dynamic fetch" (Aila & Laine 2009): every trip of a wave's loop is one traversal step (one node popped per lane), and when
// at least `refill_min` lanes are idle the wave claims that many rays with ONE atomic on one of kRqShards sharded heads
// (ballot / mbcnt hand the claim out).  refill_min = 64 is the plain form (a wave takes 64 new rays only once all are done).
// Traversal stack: entry [level][thread] -- the bottom kRqLdsLevels levels in LDS (one bank per lane), the rest in a
// renderer-owned HBM array with the same coalesced [level][thread] layout.  32-bit node references throughout.
// A result depends only on its ray and the scene: traversal order is per lane, the claim only decides who runs it.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "device_scene.hpp"
#include "device_access.hpp"
#include "ray_query.hpp"

namespace drt {

namespace {

// rank of this lane among the lanes set in `mask` (v_mbcnt): the claim hands rays to idle lanes in lane order
DRT_DEV int lane_rank(uint64_t mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

template <bool OCC>
__global__ __launch_bounds__(kRqThreads, kRqWavesPerSimd) void ray_query_kernel(const SceneView sc, const RayQueryArgs a) {
    constexpr int K = OCC ? kRqLdsLevelsOccluded : kRqLdsLevelsClosest;
    __shared__ uint32_t s_ref[K][kRqThreads];
    __shared__ float s_dist[OCC ? 1 : K][kRqThreads];
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t gthread = blockIdx.x * kRqThreads + tid, gthreads = gridDim.x * kRqThreads;
    uint32_t shard = (gthread >> 6) % kRqShards;            // home shard of this wave; on to the next one when it is empty
    int shards_empty = 0;
    const uint32_t levels = a.stack_levels;                  // = tree depth: the stack never holds more entries

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
        const uint32_t n_idle = (uint32_t)__popcll(idle);
        if (shards_empty < kRqShards && (n_idle >= a.refill_min || n_idle == 64u)) {
            const int my_rank = lane_rank(idle);
            const bool was_idle = rid < 0;
            uint32_t filled = 0;
            while (filled < n_idle && shards_empty < kRqShards) {
                const uint32_t want = n_idle - filled;
                const uint32_t s_begin = (uint32_t)((uint64_t)a.n * shard / kRqShards);
                const uint32_t len = (uint32_t)((uint64_t)a.n * (shard + 1) / kRqShards) - s_begin;
                // lane 0 claims and clips the claim to the shard; start / got go to the wave (64-bit signed arithmetic: the
                // shard's remainder len - b is negative once other waves have emptied it)
                int64_t start = 0, got = 0;
                if (lane == 0) {
                    const int64_t b = (int64_t)atomicAdd(a.heads + shard * kRqShardStride, want);
                    const int64_t left = (int64_t)len - b;
                    if (left > 0) { start = (int64_t)s_begin + b; got = left < (int64_t)want ? left : (int64_t)want; }
                }
                start = __shfl(start, 0);
                got = __shfl(got, 0);
                if (got <= 0) { shard = (shard + 1) % kRqShards; shards_empty++; continue; }
                const int64_t k = (int64_t)my_rank - (int64_t)filled;
                if (was_idle && k >= 0 && k < got && start + k < (int64_t)a.n) rid = (int)(start + k);
                filled += (uint32_t)got;
            }
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
        if (shards_empty >= kRqShards && __ballot(rid >= 0) == 0) break;

        // ---- one traversal step per busy lane ----
        if (rid >= 0 && sp > 0 && !occluded) {
            --sp;
            uint32_t ref;
            float dist = 0.f;
            if (sp < (uint32_t)K) {
                ref = s_ref[sp][tid];
                if (!OCC) dist = s_dist[sp][tid];
            } else if (OCC) {
                ref = a.stack_hbm[(size_t)(sp - K) * gthreads + gthread];
            } else {
                const uint2 e = reinterpret_cast<const uint2 *>(a.stack_hbm)[(size_t)(sp - K) * gthreads + gthread];
                ref = e.x; dist = __uint_as_float(e.y);
            }
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
                    const bool far1 = d1 > d2;                                                            // farther child first
                    const uint32_t ra = far1 ? c.ref1 : c.ref2, rb = far1 ? c.ref2 : c.ref1;
                    const float da = far1 ? d1 : d2, db = far1 ? d2 : d1;
                    const bool pa = far1 ? push1 : push2, pb = far1 ? push2 : push1;
#pragma unroll
                    for (int k = 0; k < 2; k++) {
                        const bool p = k == 0 ? pa : pb;
                        if (p && sp < levels) {
                            const uint32_t r = k == 0 ? ra : rb;
                            const float d = k == 0 ? da : db;
                            if (sp < (uint32_t)K) {
                                s_ref[sp][tid] = r;
                                if (!OCC) s_dist[sp][tid] = d;
                            } else if (OCC) {
                                a.stack_hbm[(size_t)(sp - K) * gthreads + gthread] = r;
                            } else {
                                reinterpret_cast<uint2 *>(a.stack_hbm)[(size_t)(sp - K) * gthreads + gthread] = make_uint2(r, __float_as_uint(d));
                            }
                            ++sp;
                        }
                    }
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
    if (args.n == 0) return hipSuccess;
    const uint32_t want = (args.n + kRqThreads - 1) / kRqThreads;
    const uint32_t blocks = std::min<uint32_t>(want, (uint32_t)ray_query_max_blocks(num_cus));
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
