// kernel_adaptive.hip -- adaptive sampling for gfx950 (drt_renderer_render_adaptive; the rule is stated in include/drt.h).
//
// A call runs: weights_kernel (one lane per pixel: the weight q from the pixel's moments, Q = sum q and the active count reduced
// per wave, then per workgroup through LDS, then ONE 64-bit and one 32-bit atomic per workgroup: integer sums, so exact in any
// order), counts_kernel (the sample count of every pixel from q, Q and the parameters, and the sum of each block of kScanBlock
// counts), scan_block_sums_kernel + offsets_kernel (the exclusive prefix sum of the counts: a two-level block scan), and per pixel
// range rays_kernel (the ragged ray list), the radiance kernel (kernel_radiance.hip, untouched) and fold_kernel.
//
// The scan is two-level, not decoupled look-back: the levels are separate launches, so no workgroup ever waits for another one
// inside a launch (nothing depends on residency or on dispatch order).  Level 2 is one workgroup that walks the block sums in
// chunks of kScanBlock with a carry, so two levels serve any pixel count (2^31 pixels = 2^21 block sums = 2048 chunks).
//
// The ray list has one lane per RAY, which finds its pixel by bisection in the offsets: every lane does the same work whatever the
// counts are, and a wave's stores are 2 x 1 KiB contiguous.  (One lane per pixel with a loop over its count would make a wave as slow
// as its largest count -- adaptive counts differ by design, up to max_spp : 0 -- and stride its stores by 32 B x count.)  The fold
// has one lane per PIXEL because its sums are ordered per pixel; it reads 16 B per sample and does eight flops.
//
// Everything is fp32 with one rounding per operation (-ffp-contract=off, correctly rounded divide and sqrt), so the state, the
// weights and the image are reproducible bit for bit (tests/adaptive_ref.py restates them in numpy).
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "device_scene.hpp"
#include "device_access.hpp"
#include "adaptive.hpp"

namespace drt {

namespace {

DRT_DEV float luminance(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }      // drt.h's lum()

template <class T>
DRT_DEV T wave_sum(T v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    return v;                                            // lane 0 holds the wave's sum
}
DRT_DEV uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = max(v, (uint32_t)__shfl_down(v, d, 64));
    return v;
}

// The weight of a pixel (drt.h "Weight of a pixel")
DRT_DEV uint32_t pixel_weight(uint32_t n, float m1, float m2, float target_error, float luma_floor) {
    if (n < 2u) return kAdaptiveCap;
    const float fn = (float)n;
    const float mean = m1 / fn;
    const float var = fmaxf(m2 / fn - mean * mean, 0.0f);
    const float w = sqrtf(var / fn) / (mean + luma_floor);
    if (target_error > 0.0f && w <= target_error) return 0u;
    const float s = w * 65536.0f;
    return s < 16777215.0f ? (uint32_t)s : kAdaptiveCap;       // (NaN and +inf fail the comparison: the cap)
}

// ---- stage 1: weights, Q and the active count ----
__global__ __launch_bounds__(256) void weights_kernel(const AdaptivePlanArgs a) {
    __shared__ unsigned long long s_q[4];
    __shared__ uint32_t s_active[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t q = 0;
    if (i < a.pixels) {
        if (a.state0) {
            const float4 s0 = a.state0[i], s1 = a.state1[i];
            q = pixel_weight(__float_as_uint(s0.w), s1.x, s1.y, a.target_error, a.luma_floor);
            a.q[i] = q;
        } else {
            q = a.q[i];
        }
    }
    const unsigned long long wq = wave_sum<unsigned long long>(q);
    const uint32_t wa = wave_sum<uint32_t>(q > 0u ? 1u : 0u);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_q[wave] = wq; s_active[wave] = wa; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long bq = (s_q[0] + s_q[1]) + (s_q[2] + s_q[3]);
        const uint32_t ba = (s_active[0] + s_active[1]) + (s_active[2] + s_active[3]);
        if (bq) atomicAdd(&a.totals->Q, bq);
        if (ba) atomicAdd(&a.totals->active, ba);
    }
}

// The count of a pixel (drt.h "Counts")
DRT_DEV uint32_t pixel_count(const AdaptivePlanArgs &a, uint32_t q, unsigned long long Q) {
    if (Q == 0ull && !a.thresholded) return min(a.max_spp, a.min_spp + a.extra / a.pixels);
    if (q == 0u) return a.thresholded ? 0u : a.min_spp;
    return min(a.max_spp, a.min_spp + (uint32_t)((unsigned long long)a.extra * q / Q));
}

// The exclusive prefix of this lane's `mine` among the workgroup's kScanThreads lanes; *total = the workgroup's sum.
// s_wave: one word per wave.  Ends with a barrier, so it may be called again at once.
DRT_DEV uint32_t block_exclusive(uint32_t mine, uint32_t *s_wave, uint32_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kScanThreads / 64; w++) {
        const uint32_t t = s_wave[w];
        if (w < wave) before += t;
        all += t;
    }
    __syncthreads();
    *total = all;
    return before + incl - mine;
}

// ---- stage 2: counts, and the sum of every block of kScanBlock of them ----
__global__ __launch_bounds__(kScanThreads) void counts_kernel(const AdaptivePlanArgs a) {
    __shared__ uint32_t s_wave[kScanThreads / 64], s_max[kScanThreads / 64];
    const unsigned long long Q = a.totals->Q;
    const uint32_t first = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    uint32_t sum = 0, mx = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
        const uint32_t i = first + k;
        if (i < a.pixels) {
            const uint32_t c = pixel_count(a, a.q[i], Q);
            a.counts[i] = c;
            sum += c;
            mx = max(mx, c);
        }
    }
    const uint32_t ws = wave_sum<uint32_t>(sum), wm = wave_max(mx);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_wave[wave] = ws; s_max[wave] = wm; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.block_sums[blockIdx.x] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
        const uint32_t bm = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
        if (bm) atomicMax(&a.totals->max_count, bm);
    }
}

// ---- stage 3, level 2: the block sums become their own exclusive prefix sum, in place; one workgroup ----
__global__ __launch_bounds__(kScanThreads) void scan_block_sums_kernel(const AdaptivePlanArgs a, uint32_t n_blocks) {
    __shared__ uint32_t s_wave[kScanThreads / 64];
    uint32_t carry = 0;
    for (uint32_t chunk = 0; chunk < n_blocks; chunk += kScanBlock) {
        const uint32_t first = chunk + threadIdx.x * kScanItems;
        uint32_t v[kScanItems], mine = 0;
#pragma unroll
        for (int k = 0; k < kScanItems; k++) {
            v[k] = first + k < n_blocks ? a.block_sums[first + k] : 0u;
            mine += v[k];
        }
        uint32_t total;
        uint32_t run = carry + block_exclusive(mine, s_wave, &total);
#pragma unroll
        for (int k = 0; k < kScanItems; k++) {
            if (first + k < n_blocks) a.block_sums[first + k] = run;
            run += v[k];
        }
        carry += total;
    }
    if (threadIdx.x == 0) a.totals->total = carry;
}

// ---- stage 3, level 1: offsets = the exclusive prefix sum of the counts ----
__global__ __launch_bounds__(kScanThreads) void offsets_kernel(const AdaptivePlanArgs a) {
    __shared__ uint32_t s_wave[kScanThreads / 64];
    const uint32_t first = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    uint32_t v[kScanItems], mine = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
        v[k] = first + k < a.pixels ? a.counts[first + k] : 0u;
        mine += v[k];
    }
    uint32_t total;
    uint32_t run = a.block_sums[blockIdx.x] + block_exclusive(mine, s_wave, &total);
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
        if (first + k < a.pixels) a.offsets[first + k] = run;
        run += v[k];
    }
}

// ---- stage 4: the ray list of a pixel range; one lane per ray ----
__global__ __launch_bounds__(256) void rays_kernel(const AdaptiveRangeArgs a) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= a.n_rays) return;
    const uint32_t g = a.ray_base + j;
    // the last pixel of the range whose offset is <= g: the one that owns sample g (pixels without samples share their
    // successor's offset, so they are never the last one)
    uint32_t lo = a.pixel_first, hi = a.pixel_end;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a.offsets[mid] <= g) lo = mid; else hi = mid;
    }
    const uint32_t p = lo;
    const uint32_t frame = __float_as_uint(a.state0[p].w) + (g - a.offsets[p]) + 1u;       // n + k
    const uint32_t x = p % a.width, y = p / a.width;
    FrameParams fp;                                      // (camera_rays_kernel's rule, kernel_radiance.hip)
    for (int k = 0; k < 3; k++) {
        fp.cam_pos[k] = a.cam.cam_pos[k]; fp.fwd_focus[k] = a.cam.fwd_focus[k]; fp.horizontal[k] = a.cam.horizontal[k];
        fp.vertical[k] = a.cam.vertical[k]; fp.disk_u[k] = a.cam.disk_u[k]; fp.disk_v[k] = a.cam.disk_v[k];
    }
    fp.defocus = a.cam.defocus;
    f2 screen_uv;
    screen_uv.x = ((float)x / (float)a.width) * 2 - 1;
    screen_uv.y = ((float)y / (float)a.height) * 2 - 1;
    uint32_t seed = x + y * a.width;
    seed *= frame;
    const Ray r = camera_get_ray(fp, screen_uv, seed);
    float4 *o = reinterpret_cast<float4 *>(a.rays) + 2 * (size_t)j;
    o[0] = make_float4(r.orig.x, r.orig.y, r.orig.z, __uint_as_float(seed));
    o[1] = make_float4(r.dir.x, r.dir.y, r.dir.z, a.cam.exposure);
}

// ---- stage 6: the samples folded into the state in sample order, and the image; one lane per pixel, no atomics ----
__global__ __launch_bounds__(256) void fold_kernel(const AdaptiveRangeArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.pixel_end - a.pixel_first) return;
    const uint32_t p = a.pixel_first + i;
    float4 s0 = a.state0[p], s1 = a.state1[p];
    uint32_t c = a.counts[p];
    const uint32_t base = a.offsets[p] - a.ray_base;
    if (base > a.n_rays || c > a.n_rays - base) c = 0;       // (never: the range holds all of its pixels' samples)
    for (uint32_t k = 0; k < c; k++) {
        const float4 s = a.samples[base + k];
        s0.x = s0.x + s.x; s0.y = s0.y + s.y; s0.z = s0.z + s.z;
        const float Y = luminance(s.x, s.y, s.z);
        s1.x = s1.x + Y;
        s1.y = s1.y + Y * Y;
    }
    const uint32_t n = __float_as_uint(s0.w) + c;
    s0.w = __uint_as_float(n);
    s1.z = __uint_as_float(a.q[p]);
    s1.w = __uint_as_float(c);
    a.state0[p] = s0;
    a.state1[p] = s1;
    const float fn = (float)n;
    a.rgba[p] = n ? make_float4(s0.x / fn, s0.y / fn, s0.z / fn, 1.0f) : make_float4(0.f, 0.f, 0.f, 1.0f);
}

}  // namespace

hipError_t launch_adaptive_plan(const AdaptivePlanArgs &a, hipStream_t stream) {
    if (a.pixels == 0) return hipSuccess;
    const uint32_t n_blocks = (a.pixels + kScanBlock - 1) / kScanBlock;
    hipLaunchKernelGGL(weights_kernel, dim3((a.pixels + 255u) / 256u), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(counts_kernel, dim3(n_blocks), dim3(kScanThreads), 0, stream, a);
    hipLaunchKernelGGL(scan_block_sums_kernel, dim3(1), dim3(kScanThreads), 0, stream, a, n_blocks);
    hipLaunchKernelGGL(offsets_kernel, dim3(n_blocks), dim3(kScanThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_adaptive_rays(const AdaptiveRangeArgs &a, hipStream_t stream) {
    if (a.n_rays == 0) return hipSuccess;
    hipLaunchKernelGGL(rays_kernel, dim3((a.n_rays + 255u) / 256u), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_adaptive_fold(const AdaptiveRangeArgs &a, hipStream_t stream) {
    const uint32_t n = a.pixel_end - a.pixel_first;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(fold_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace drt
