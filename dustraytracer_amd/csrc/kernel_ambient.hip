// kernel_ambient.hip -- ambient occlusion for gfx950: cosine-weighted visibility at surface points (drt_renderer_ambient_occlusion;
// include/drt.h states the rule, ambient.hpp holds it).
//
// Every sample of every point is one occlusion ray: made in registers from (point, sample), traced by the occlusion traversal of
// kernel_ray_query.hip (traverseBVH_raytest, BVH/BVHTraversal.cuh:76-134, with the tmax culls of drt_renderer_occluded), reduced in the
// wave.  No ray and no per-sample result is ever stored.
//
// Shape: the occlusion ray query's persistent grid (8 workgroups of 256 threads per CU).  The work unit is a tile of 64 lanes
// (ambient.hpp: 64 samples of one point, 64 / S whole points, or one point with idle lanes); a wave claims one tile with ONE atomic on
// one of kRqShards sharded 64-bit heads, once all its lanes are done (the plain form, refill_min = 64), and its lanes then take one
// traversal step per trip until none has a node left.  Traversal stack: entry [level][thread] -- the bottom kRqLdsLevelsOccluded levels
// in LDS (one bank per lane), the rest in the renderer's HBM stack array.  Reduction: `open` from the ballot of the open lanes, `bent`
// by __shfl_xor butterflies over the lanes of a point (log2 S steps in a packed tile, 6 otherwise).  One lane per point writes the
// 16-byte record with a plain store (S <= 64) or adds to it with four integer atomics whose value is not read (S > 64: several tiles per
// point; ambient_init_kernel zeroed the record).  Integer sums only: a record is the same bytes whatever the claim order was.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "device_scene.hpp"
#include "device_access.hpp"
#include "ray_query.hpp"
#include "ambient.hpp"

namespace drt {

namespace {

// Skipped points get their record here, not from the tracing kernel; the others get zeros where that kernel adds to them
__global__ __launch_bounds__(256) void ambient_init_kernel(const AmbientArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    const bool live = ao_live(a.pts[i].max_dist);
    if (!live) reinterpret_cast<int4 *>(a.out)[i] = make_int4(-1, 0, 0, 0);
    else if (a.samples > 64u) reinterpret_cast<int4 *>(a.out)[i] = make_int4(0, 0, 0, 0);
}

// STATS: lane 0 of every wave counts its trips and the lanes that took a step in them into stats[0..1] (the measurement of DESIGN 5.30)
template <bool STATS>
__global__ __launch_bounds__(kRqThreads, kRqWavesPerSimd) void ambient_kernel(const SceneView sc, const AmbientArgs a,
                                                                              unsigned long long *stats) {
    constexpr int K = kRqLdsLevelsOccluded;
    __shared__ uint32_t s_ref[K][kRqThreads];
    const int tid = threadIdx.x;
    const uint32_t lane = (uint32_t)tid & 63u;
    const uint32_t gthread = blockIdx.x * kRqThreads + tid, gthreads = gridDim.x * kRqThreads;
    const uint32_t levels = a.stack_levels;                  // = tree depth: the stack never holds more entries
    const AoTiling tl = ao_tiling(a.samples);
    const uint64_t count = ao_tile_count(tl, a.n);
    uint32_t shard = (gthread >> 6) % kRqShards;            // home shard of this wave; on to the next one when it is empty
    int shards_empty = 0;
    unsigned long long trips = 0, steps = 0;

    for (;;) {
        // ---- claim one tile (wave-uniform) ----
        uint64_t tile = 0;
        bool got = false;
        while (shards_empty < kRqShards) {
            const uint64_t s_begin = ao_shard_begin(count, shard, kRqShards);
            const uint64_t len = ao_shard_begin(count, shard + 1, kRqShards) - s_begin;
            unsigned long long b = 0;
            if (lane == 0) b = atomicAdd(a.heads + shard * kAoHeadStride, 1ull);
            b = __shfl(b, 0);
            if (b < len) { tile = s_begin + b; got = true; break; }
            shard = (shard + 1) % kRqShards; shards_empty++;
        }
        if (!got) break;

        // ---- this lane's ray, made where it is used ----
        uint32_t point = 0, sample = 0;
        const bool active = ao_tile_lane(tl, tile, lane, a.n, point, sample);
        bool tracing = false;
        float d[3] = { 0.f, 0.f, 0.f };
        Ray ray;
        float tmax = 0.f;
        uint32_t sp = 0;
        bool occluded = false;
        if (active) {
            const float4 *q = reinterpret_cast<const float4 *>(a.pts) + 2 * (size_t)point;
            const float4 q0 = q[0], q1 = q[1];
            AoPoint pt;
            pt.p[0] = q0.x; pt.p[1] = q0.y; pt.p[2] = q0.z; pt.max_dist = q0.w;
            pt.n[0] = q1.x; pt.n[1] = q1.y; pt.n[2] = q1.z; pt.bias = q1.w;
            tracing = ao_live(pt.max_dist);
            if (tracing) {
                float o[3];
                ao_ray(pt, a.seed_hash, a.first + point, sample, o, d);
                ray = make_ray(mk3(o[0], o[1], o[2]), mk3(d[0], d[1], d[2]));
                tmax = pt.max_dist;
                if (sc.root_ref != kNoNode) {
                    const float droot = slab_intersect(ld3(sc.root_min), ld3(sc.root_max), ray);
                    if (!(droot < 0 || droot > tmax)) { s_ref[0][tid] = sc.root_ref; sp = 1; }      // :95-103 with tmax
                }
            }
        }

        // ---- one traversal step per busy lane and trip (ray_query_kernel<true>'s, tmin = 0) ----
        for (;;) {
            const bool busy = sp > 0 && !occluded;
            const uint64_t busy_mask = __ballot(busy);
            if (busy_mask == 0) break;
            if (STATS) { trips += 1; steps += (unsigned long long)__popcll(busy_mask); }
            if (busy) {
                --sp;
                const uint32_t ref = sp < (uint32_t)K ? s_ref[sp][tid] : a.stack_hbm[(size_t)(sp - K) * gthreads + gthread];
                if (ref & kLeafBit) {
                    const LeafRange leaf = sc.leaves[ref & ~kLeafBit];
                    for (int i = leaf.start; i < leaf.start + leaf.count; i++) {            // :107-115
                        const TriTest tri = load_tri(sc.tri_hot, i);
                        float t, u, v;
                        const bool h = tri_intersect_flat(ray, tri.v0, tri.e1, tri.e2, t, u, v);
                        if (h && t > 0.0f && t < tmax && any_hit(sc, i, mk3(1.0f - u - v, u, v))) { occluded = true; break; }
                    }
                } else {
                    const ChildPair c = load_children(sc.inner, ref);
                    const float d1 = slab_intersect(c.min1, c.max1, ray);
                    const float d2 = slab_intersect(c.min2, c.max2, ray);
                    const bool push1 = d1 >= 0 && !(d1 > tmax), push2 = d2 >= 0 && !(d2 > tmax);      // :122-129 with tmax
                    const bool far1 = d1 > d2;                                                            // farther child first
                    const uint32_t ra = far1 ? c.ref1 : c.ref2, rb = far1 ? c.ref2 : c.ref1;
                    const bool pa = far1 ? push1 : push2, pb = far1 ? push2 : push1;
#pragma unroll
                    for (int k = 0; k < 2; k++) {
                        const bool p = k == 0 ? pa : pb;
                        if (p && sp < levels) {
                            const uint32_t r = k == 0 ? ra : rb;
                            if (sp < (uint32_t)K) s_ref[sp][tid] = r;
                            else a.stack_hbm[(size_t)(sp - K) * gthreads + gthread] = r;
                            ++sp;
                        }
                    }
                }
            }
        }

        // ---- reduce over the lanes of a point; its first lane writes ----
        const bool open = tracing && !occluded;
        const uint64_t open_mask = __ballot(open);
        int32_t b0 = open ? ao_bent_term(d[0]) : 0, b1 = open ? ao_bent_term(d[1]) : 0, b2 = open ? ao_bent_term(d[2]) : 0;
        for (uint32_t off = 1; off < tl.seg; off <<= 1) {
            b0 += __shfl_xor(b0, (int)off);
            b1 += __shfl_xor(b1, (int)off);
            b2 += __shfl_xor(b2, (int)off);
        }
        if (tracing && (lane & (tl.seg - 1u)) == 0u) {           // (tracing is one value over a point's lanes: its first lane has sample 0 or 64 t)
            const uint64_t mine = tl.seg == 64u ? open_mask : (open_mask >> lane) & ((1ull << tl.seg) - 1ull);
            const int32_t n_open = (int32_t)__popcll(mine);
            if (a.samples <= 64u) {
                reinterpret_cast<int4 *>(a.out)[point] = make_int4(n_open, b0, b1, b2);
            } else {
                int32_t *rec = reinterpret_cast<int32_t *>(a.out + point);
                atomicAdd(rec + 0, n_open);
                atomicAdd(rec + 1, b0);
                atomicAdd(rec + 2, b1);
                atomicAdd(rec + 3, b2);
            }
        }
    }
    if (STATS && lane == 0) { atomicAdd(stats + 0, trips); atomicAdd(stats + 1, steps); }
}

}  // namespace

hipError_t launch_ambient_init(const AmbientArgs &args, hipStream_t stream) {
    if (args.n == 0) return hipSuccess;
    hipLaunchKernelGGL(ambient_init_kernel, dim3((args.n + 255u) / 256u), dim3(256), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_ambient(const SceneView &sc, const AmbientArgs &args, int num_cus, unsigned long long *stats, hipStream_t stream) {
    if (args.n == 0) return hipSuccess;
    const uint64_t tiles = ao_tile_count(ao_tiling(args.samples), args.n);
    const uint64_t want = (tiles + kRqThreads / 64 - 1) / (kRqThreads / 64);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(want, (uint64_t)ray_query_max_blocks(num_cus));
    if (stats) hipLaunchKernelGGL(ambient_kernel<true>, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args, stats);
    else hipLaunchKernelGGL(ambient_kernel<false>, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args, stats);
    return hipGetLastError();
}

}  // namespace drt
