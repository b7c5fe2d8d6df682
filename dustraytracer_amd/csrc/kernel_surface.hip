// kernel_surface.hip -- surface lookups and area-weighted sampling for gfx950 (drt_renderer_surface_lookup, _surface_weights and
// _sample_surface).  The reference has no such query; include/drt.h states the rules and surface.hpp holds them as per-record
// routines, which the kernels below only distribute.  None of them walks the BVH: they read the renderer's device copy of the scene.
//
//   lookup   one lane per reference over a grid-stride loop: the 16-byte reference, the TriHot / TriCold / MatDev / MatExt / TexDev
//            records, one texel, nine normals; six 16-byte stores.  No atomics, no LDS, no scratch.
//   weights  amax     every workgroup reduces its triangles' a = |cross(e1, e2)| in LDS and folds the maximum into one word with an
//                     integer atomicMax on the bits (a >= 0 and finite: the bits order as the values do, and a maximum does not
//                     depend on the order)
//            totals   workgroup b sums the integer weights q of triangles [b B, (b + 1) B), B = kSurfScanBlock, one per thread
//            offsets  ONE workgroup turns the block totals into exclusive offsets, B at a trip with a running carry
//            cdf      workgroup b scans its B weights and adds its offset
//            Four launches in stream order.  No workgroup waits for another within a launch: no look-back, no flag, no spin.  The
//            sums are integers, so the table is the same bytes whatever the shape.
//   sample   one lane per sample: four hashes, a binary search in the table (about log2(n_tris) dependent 8-byte loads), one
//            16-byte store
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_scene.hpp"
#include "surface.hpp"

namespace drt {

namespace {

__global__ __launch_bounds__(kSurfThreads) void surface_lookup_kernel(const SceneView sc, const SurfaceArgs a) {
    const uint32_t stride = gridDim.x * kSurfThreads;
    for (uint32_t i = blockIdx.x * kSurfThreads + threadIdx.x; i < a.n; i += stride) {
        const float4 ref = reinterpret_cast<const float4 *>(a.refs)[i];            // {t, prim, u, v}: t is not read
        const SurfRecord rec = surface_lookup_one(sc, a, __float_as_int(ref.y), ref.z, ref.w);
        uint4 *out = reinterpret_cast<uint4 *>(a.out + i);
#pragma unroll
        for (int k = 0; k < 6; k++) out[k] = make_uint4(rec.q[k].x, rec.q[k].y, rec.q[k].z, rec.q[k].w);
    }
}

__global__ __launch_bounds__(kSurfThreads) void surface_amax_kernel(const SurfaceScanArgs a) {
    __shared__ uint32_t s_max[kSurfThreads];
    const uint32_t stride = gridDim.x * kSurfThreads;
    uint32_t best = 0;
    for (uint32_t i = blockIdx.x * kSurfThreads + threadIdx.x; i < a.n_tris; i += stride)
        best = max(best, __float_as_uint(surface_area2(a.hot[i])));               // (a >= +0: the bits order as the values)
    s_max[threadIdx.x] = best;
    __syncthreads();
    for (int half = kSurfThreads / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) s_max[threadIdx.x] = max(s_max[threadIdx.x], s_max[threadIdx.x + half]);
        __syncthreads();
    }
    if (threadIdx.x == 0 && s_max[0]) atomicMax(a.amax_bits, s_max[0]);
}

// this thread's weight: triangle blockIdx.x * B + threadIdx.x, 0 behind the last one and everywhere when amax == 0
__device__ __forceinline__ uint64_t weight_of_thread(const SurfaceScanArgs &a, uint32_t &index) {
    index = blockIdx.x * kSurfScanBlock + threadIdx.x;
    const uint32_t amax_bits = *a.amax_bits;
    if (index >= a.n_tris || amax_bits == 0) return 0;
    return surface_weight(surface_area2(a.hot[index]), surface_exponent(amax_bits));
}

// inclusive sum over the workgroup's kSurfScanBlock threads (Hillis-Steele between two LDS rows); s is free again after the
// barrier the caller places before its next use
__device__ __forceinline__ uint64_t block_inclusive_scan(uint64_t v, uint64_t (*s)[kSurfScanBlock]) {
    const uint32_t t = threadIdx.x;
    int cur = 0;
    s[0][t] = v;
    __syncthreads();
    for (uint32_t off = 1; off < kSurfScanBlock; off <<= 1) {
        uint64_t x = s[cur][t];
        if (t >= off) x += s[cur][t - off];
        s[cur ^ 1][t] = x;
        cur ^= 1;
        __syncthreads();
    }
    return s[cur][t];
}

__global__ __launch_bounds__(kSurfThreads) void surface_totals_kernel(const SurfaceScanArgs a) {
    __shared__ uint64_t s[2][kSurfScanBlock];
    uint32_t index;
    const uint64_t sum = block_inclusive_scan(weight_of_thread(a, index), s);
    if (threadIdx.x == kSurfScanBlock - 1) a.block_totals[blockIdx.x] = sum;
}

__global__ __launch_bounds__(kSurfThreads) void surface_offsets_kernel(uint64_t *block_totals, uint32_t n_blocks) {
    __shared__ uint64_t s[2][kSurfScanBlock];
    __shared__ uint64_t s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n_blocks; base += kSurfScanBlock) {
        const uint32_t b = base + threadIdx.x;
        const uint64_t v = b < n_blocks ? block_totals[b] : 0;
        const uint64_t incl = block_inclusive_scan(v, s);
        const uint64_t carry = s_carry;
        if (b < n_blocks) block_totals[b] = carry + (incl - v);                    // exclusive: the sum of the blocks in front
        __syncthreads();                                                           // everyone has read s_carry and s
        if (threadIdx.x == kSurfScanBlock - 1) s_carry = carry + incl;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kSurfThreads) void surface_cdf_kernel(const SurfaceScanArgs a) {
    __shared__ uint64_t s[2][kSurfScanBlock];
    uint32_t index;
    const uint64_t incl = block_inclusive_scan(weight_of_thread(a, index), s);
    if (index < a.n_tris) a.cdf[index] = a.block_totals[blockIdx.x] + incl;
}

__global__ __launch_bounds__(kSurfThreads) void surface_sample_kernel(const uint64_t *cdf, uint32_t n_tris, uint32_t seed_hash, uint32_t first,
                                                                      SurfRef *out, uint32_t n) {
    const uint32_t stride = gridDim.x * kSurfThreads;
    for (uint32_t k = blockIdx.x * kSurfThreads + threadIdx.x; k < n; k += stride) {
        const SurfRef r = surface_sample_one(seed_hash, first + k, cdf, n_tris);   // (first + n <= 2^32: no wrap)
        reinterpret_cast<float4 *>(out)[k] = make_float4(r.t, __int_as_float(r.prim), r.u, r.v);
    }
}

// enough workgroups for every item, at most 8 per CU (2048 lanes a CU: what fits at these kernels' register counts)
uint32_t grid_for(uint32_t n, int num_cus) {
    const uint32_t want = (n + kSurfThreads - 1) / kSurfThreads;
    return std::max<uint32_t>(1, std::min<uint32_t>(want, (uint32_t)std::max(1, num_cus) * 8u));
}

}  // namespace

hipError_t launch_surface_lookup(const SceneView &sc, const SurfaceArgs &args, int num_cus, hipStream_t stream) {
    if (args.n == 0) return hipSuccess;
    hipLaunchKernelGGL(surface_lookup_kernel, dim3(grid_for(args.n, num_cus)), dim3(kSurfThreads), 0, stream, sc, args);
    return hipGetLastError();
}

hipError_t launch_surface_weights(const SurfaceScanArgs &args, hipStream_t stream) {
    if (args.n_tris == 0) return hipSuccess;
    static_assert(kSurfScanBlock == (uint32_t)kSurfThreads, "one triangle per thread");
    const uint32_t n_blocks = (args.n_tris + kSurfScanBlock - 1) / kSurfScanBlock;
    hipError_t e = hipMemsetAsync(args.amax_bits, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(surface_amax_kernel, dim3(std::min<uint32_t>(n_blocks, 2048u)), dim3(kSurfThreads), 0, stream, args);
    hipLaunchKernelGGL(surface_totals_kernel, dim3(n_blocks), dim3(kSurfThreads), 0, stream, args);
    hipLaunchKernelGGL(surface_offsets_kernel, dim3(1), dim3(kSurfThreads), 0, stream, args.block_totals, n_blocks);
    hipLaunchKernelGGL(surface_cdf_kernel, dim3(n_blocks), dim3(kSurfThreads), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_surface_sample(const uint64_t *cdf, uint32_t n_tris, uint32_t seed, uint32_t first, SurfRef *out, uint32_t n, int num_cus,
                                 hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(surface_sample_kernel, dim3(grid_for(n, num_cus)), dim3(kSurfThreads), 0, stream, cdf, n_tris, surf_pcg(seed), first,
                       out, n);
    return hipGetLastError();
}

}  // namespace drt
