// kernel_upscale.hip -- joint-bilateral upsampling steered by the first-hit guides, for gfx950 (drt_renderer_upscale; the rule and
// its order are those of include/drt.h, restated in tests/upscale_ref.py).
//
// upscale_kernel: one output pixel per lane, a wave per 8x8 tile of the OUTPUT image (as guide_kernel and temporal_reproject_kernel),
// so that the low-resolution taps of neighbouring lanes fall in the same cache lines: a tile reads at most a 5x5 patch of source
// pixels in stage 1, which the 64 lanes share through the vector L1 -- no LDS, no atomics, no barrier.  Per lane: two 16-byte loads
// for its own guide, per tap the 16-byte key half of the source guide (normal, prim) first and the other half and the colour only
// when the tap is valid, one 16-byte store.  Memory-bound: 48 B per output pixel of compulsory traffic plus the source image once.
// Stage 2 (the 4x4 search) runs only for lanes none of whose four taps was accepted -- silhouettes; the branch is divergent and rare.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "upscale.hpp"

namespace drt {

namespace {

constexpr int kUpThreads = 256;                  // 4 waves, one 8x8 output tile each

// The output pixel's own guide and what is derived from it once
struct UpCentre {
    f3 albedo, normal;
    float t, inv_dz;             // 1 / (sigma_depth * t)
    bool miss;
};

// A tap: is it valid, its value v(q) and its distance e from the output pixel (drt.h, step 2); qx, qy are clamped by the caller
DRT_DEV bool upscale_tap(const UpscaleArgs &a, const UpCentre &p, int qx, int qy, f3 &v, float &e) {
    const size_t q = (size_t)qx + (size_t)qy * a.width;
    const float4 *gl = reinterpret_cast<const float4 *>(a.guides_lo) + 2 * q;
    const float4 g1 = gl[1];
    if ((__float_as_int(g1.w) < 0) != p.miss) return false;
    const float4 g0 = gl[0], c = a.color[q];
    v = mk3(c.x, c.y, c.z);
    if (a.demodulate) v = mk3(c.x / fmaxf(g0.x, a.albedo_floor), c.y / fmaxf(g0.y, a.albedo_floor), c.z / fmaxf(g0.z, a.albedo_floor));
    e = 0.f;
    if (!p.miss) {
        const f3 dn = p.normal - mk3(g1.x, g1.y, g1.z);
        const float dz = (g0.w - p.t) * p.inv_dz;
        e = dot(dn, dn) * a.k_normal + dz * dz;
        if (!a.demodulate) {
            const f3 da = p.albedo - mk3(g0.x, g0.y, g0.z);
            e = e + dot(da, da) * a.k_albedo;
        }
    }
    return true;
}

__global__ __launch_bounds__(kUpThreads) void upscale_kernel(const UpscaleArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t tiles_x = (a.out_width + 7) / 8, tiles = tiles_x * ((a.out_height + 7) / 8);
    const uint32_t tile = blockIdx.x * (kUpThreads / 64) + threadIdx.x / 64;
    if (tile >= tiles) return;
    const uint32_t X = (tile % tiles_x) * 8 + (uint32_t)(lane & 7), Y = (tile / tiles_x) * 8 + (uint32_t)(lane >> 3);
    if (X >= a.out_width || Y >= a.out_height) return;
    const int W = (int)a.width, H = (int)a.height;
    const size_t P = (size_t)X + (size_t)Y * a.out_width;
    const float4 h0 = reinterpret_cast<const float4 *>(a.guides_hi)[2 * P], h1 = reinterpret_cast<const float4 *>(a.guides_hi)[2 * P + 1];
    UpCentre p;
    p.albedo = mk3(h0.x, h0.y, h0.z);
    p.normal = mk3(h1.x, h1.y, h1.z);
    p.t = h0.w;
    p.inv_dz = 1.0f / (a.sigma_depth * h0.w);
    p.miss = __float_as_int(h1.w) < 0;

    const float fx = ((float)X * (float)a.width) / (float)a.out_width, fy = ((float)Y * (float)a.height) / (float)a.out_height;
    const float flx = floorf(fx), fly = floorf(fy);
    const int x0 = (int)flx, y0 = (int)fly;
    const float wx1 = fx - flx, wy1 = fy - fly, wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;

    // Stage 1: the four bilinear taps, each weighted by expf(-e); a tap takes part only if e <= 16 (no expf decides a branch)
    float S = 0.f;
    f3 A = mk3(0, 0, 0), o;
    bool any = false;
#pragma unroll
    for (int j = 0; j < 2; j++) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const float b = (i ? wx1 : wx0) * (j ? wy1 : wy0);
            f3 v;
            float e;
            if (!upscale_tap(a, p, min(x0 + i, W - 1), min(y0 + j, H - 1), v, e)) continue;
            if (!(b > 0.f) || !(e <= 16.0f)) continue;
            const float w = b * expf(-e);
            S += w;
            A = A + v * w;
            any = true;
        }
    }
    if (any) {
        o = A / S;
    } else {
        // Stage 2: the closest valid tap of the 4x4 window (the first one wins a tie, a NaN distance never wins)
        float best = 0.f;
        bool have = false;
        for (int dy = -1; dy <= 2; dy++) {
            const int qy = min(max(y0 + dy, 0), H - 1);
            for (int dx = -1; dx <= 2; dx++) {
                const int qx = min(max(x0 + dx, 0), W - 1);
                f3 v;
                float e;
                if (!upscale_tap(a, p, qx, qy, v, e)) continue;
                if (have ? e < best : e == e) {
                    best = e;
                    o = v;
                    have = true;
                }
            }
        }
        if (!have) {
            // Stage 3: nothing comparable in the window: the nearest source pixel
            const size_t q = (size_t)min(x0 + (wx1 > 0.5f ? 1 : 0), W - 1) + (size_t)min(y0 + (wy1 > 0.5f ? 1 : 0), H - 1) * a.width;
            const float4 c = a.color[q];
            o = mk3(c.x, c.y, c.z);
            if (a.demodulate) {
                const float4 g0 = reinterpret_cast<const float4 *>(a.guides_lo)[2 * q];
                o = mk3(c.x / fmaxf(g0.x, a.albedo_floor), c.y / fmaxf(g0.y, a.albedo_floor), c.z / fmaxf(g0.z, a.albedo_floor));
            }
        }
    }
    if (a.demodulate) o = mk3(o.x * fmaxf(p.albedo.x, a.albedo_floor), o.y * fmaxf(p.albedo.y, a.albedo_floor), o.z * fmaxf(p.albedo.z, a.albedo_floor));
    a.out[P] = make_float4(o.x, o.y, o.z, 1.0f);
}

}  // namespace

hipError_t launch_upscale(const UpscaleArgs &args, hipStream_t stream) {
    const uint32_t tiles = ((args.out_width + 7) / 8) * ((args.out_height + 7) / 8);
    if (tiles == 0 || args.width == 0 || args.height == 0) return hipSuccess;
    hipLaunchKernelGGL(upscale_kernel, dim3((tiles + kUpThreads / 64 - 1) / (kUpThreads / 64)), dim3(kUpThreads), 0, stream, args);
    return hipGetLastError();
}

}  // namespace drt
