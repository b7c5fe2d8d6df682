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
// Shape: kernel_nearest.hip's.  Persistent grid of 256-thread workgroups, one query per lane, every trip of a wave's loop pops one
// node per lane, and when at least `refill_min` lanes are idle the wave claims that many queries with ONE atomic on one of kRqShards
// sharded heads.  Traversal stack: entry {ref, box2} at [level][thread] -- the bottom kRqLdsLevelsClosest levels in LDS, the rest in
// the renderer's HBM array with the same coalesced layout.  A result depends only on its query and the scene.
//
// Registers: a lane keeps q0, a1, a2, g, nq and the six bounds -- 21 floats -- and best, prim and feature for as long as it owns the
// query; the witness is not kept but made again from (prim, candidate) when the query ends.  The table of what was tried is in
// DESIGN 5.27; the bound is kTriDistanceWavesPerSimd waves per SIMD, and the grid is that many workgroups per CU.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "device_scene.hpp"
#include "device_access.hpp"
#include "tri_distance.hpp"

namespace drt {

namespace {

// rank of this lane among the lanes set in `mask` (v_mbcnt): the claim hands queries to idle lanes in lane order
DRT_DEV int lane_rank(uint64_t mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

template <bool ANY>
__global__ __launch_bounds__(kRqThreads, kTriDistanceWavesPerSimd) void tri_distance_kernel(const SceneView sc, const TriDistanceArgs a) {
    constexpr int K = kRqLdsLevelsClosest;
    __shared__ uint32_t s_ref[K][kRqThreads];
    __shared__ float s_box2[K][kRqThreads];
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t gthread = blockIdx.x * kRqThreads + tid, gthreads = gridDim.x * kRqThreads;
    uint32_t shard = (gthread >> 6) % kRqShards;            // home shard of this wave; on to the next one when it is empty
    int shards_empty = 0;
    const uint32_t levels = a.stack_levels;                  // = tree depth: the stack never holds more entries

    int rid = -1;                                            // this lane's query, -1 = idle
    f3 qmin = mk3(0.f, 0.f, 0.f), qmax = mk3(0.f, 0.f, 0.f); // its world bounds
    TriOverlapQuery q = {};                                  // q0, a1, a2, g, nq: only a leaf's pair test reads them
    float best = 0.f;                                        // the nearest so far (prim -1 = none): best = its d2, else max_dist^2
    int best_prim = -1, best_feature = 0;
    uint32_t sp = 0;

    for (;;) {
        // ---- refill: claim queries for the idle lanes (wave-uniform) ----
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
        if (shards_empty >= kRqShards && __ballot(rid >= 0) == 0) break;

        // ---- one traversal step per busy lane ----
        if (rid >= 0 && sp > 0) {
            --sp;
            uint32_t ref;
            float box2;
            if (sp < (uint32_t)K) {
                ref = s_ref[sp][tid]; box2 = s_box2[sp][tid];
            } else {
                const uint2 e = reinterpret_cast<const uint2 *>(a.stack_hbm)[(size_t)(sp - K) * gthreads + gthread];
                ref = e.x; box2 = __uint_as_float(e.y);
            }
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
                    const bool far1 = b1 > b2;                                                        // farther child first
                    const uint32_t ra = far1 ? c.ref1 : c.ref2, rb = far1 ? c.ref2 : c.ref1;
                    const float da = far1 ? b1 : b2, db = far1 ? b2 : b1;
                    const bool pa = far1 ? push1 : push2, pb = far1 ? push2 : push1;
#pragma unroll
                    for (int k = 0; k < 2; k++) {
                        const bool push = k == 0 ? pa : pb;
                        if (push && sp < levels) {
                            const uint32_t r = k == 0 ? ra : rb;
                            const float d = k == 0 ? da : db;
                            if (sp < (uint32_t)K) {
                                s_ref[sp][tid] = r; s_box2[sp][tid] = d;
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
    if (args.n == 0) return hipSuccess;
    const uint32_t want = (args.n + kRqThreads - 1) / kRqThreads;
    // kTriDistanceWavesPerSimd workgroups per CU (4 waves each, one per SIMD): never more than ray_query_max_blocks, whose HBM stack it uses
    const uint32_t resident = (uint32_t)std::max(1, num_cus) * (uint32_t)kTriDistanceWavesPerSimd;
    const uint32_t blocks = std::min<uint32_t>(want, std::min<uint32_t>(resident, (uint32_t)ray_query_max_blocks(num_cus)));
    if (any_mode) hipLaunchKernelGGL(tri_distance_kernel<true>, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args);
    else hipLaunchKernelGGL(tri_distance_kernel<false>, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args);
    return hipGetLastError();
}

}  // namespace drt
