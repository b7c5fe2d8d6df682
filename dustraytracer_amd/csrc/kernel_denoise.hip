// kernel_denoise.hip -- first-hit guide buffers and the edge-avoiding a-trous filter for gfx950 (drt_renderer_render_guides,
// drt_renderer_denoise).
//
// guide_kernel: the primary ray of RayGen (Shaders/RayGen.cuh:63-85: uv, seed = (x + y * width) * frame, Camera::GetRay with
// jitter and defocus), traced with the closest-hit ray query's traversal at tmin = 0, tmax = FLT_MAX (kernel_ray_query.hip, which
// is TraceRay bit for bit: same culling, far child pushed first, strict <, AnyHit alpha), then what the first trip of RayGen's
// loop makes of the hit (:99-161): the throughput after the first hit's albedo (the ALBEDO debug view), the normal turned against
// the ray (the NORMAL debug view), or on a miss the sky term the ALBEDO view shows.  Both views reach the framebuffer through
// the running sum, 0 + c (RenderKernel.cu:29): the guides are stored the same way, so a -0 component reads +0 as it does there.
// Shape: a resident grid of 256-thread workgroups, 8 per CU (the ray query's); each wave takes 8x8 pixel tiles in turn (tile
// = global wave + k * waves), one pixel per lane, so a wave's 64 rays leave the camera side by side.  Stack as the ray query's
// closest build: entry [level][thread], the bottom 8 levels in LDS (one bank per lane), the rest in the renderer's HBM array.
//
// atrous_kernel: one pass of the filter of include/drt.h drt_renderer_denoise (Dammertz et al. 2010, "Edge-avoiding a-trous
// wavelet transform for fast global illumination filtering"): 5x5 B3-spline taps 2^i apart, clamped to the image, each weighted by
// exp(-(colour, normal and albedo distances)).  One pixel per lane, 256 per workgroup.  Small steps (atrous_lds_kernel): a
// workgroup takes a 16x16 tile of the step's pixel lattice, whose taps all fall on the lattice, and stages the tile and its halo
// in LDS.  Large steps (atrous_kernel, where lattice tiles would lie mostly outside the image): 16x16 pixels, taps read through
// the caches (16 B of colour, 24 B of guide per tap).
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "device_scene.hpp"
#include "device_access.hpp"
#include "ray_query.hpp"
#include "denoise.hpp"

namespace drt {

namespace {

constexpr int kGuideLdsLevels = kRqLdsLevelsClosest;

__global__ __launch_bounds__(kRqThreads, kRqWavesPerSimd) void guide_kernel(const SceneView sc, const FrameParams fp, const GuideArgs a) {
    constexpr int K = kGuideLdsLevels;
    __shared__ uint32_t s_ref[K][kRqThreads];
    __shared__ float s_dist[K][kRqThreads];
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t gthread = blockIdx.x * kRqThreads + tid, gthreads = gridDim.x * kRqThreads;
    const uint32_t tiles_x = (fp.width + 7) / 8, tiles = tiles_x * ((fp.height + 7) / 8);
    const uint32_t waves = gthreads / 64;
    const uint32_t levels = a.stack_levels;

    for (uint32_t tile = gthread / 64; tile < tiles; tile += waves) {
        const uint32_t x = (tile % tiles_x) * 8 + (uint32_t)(lane & 7), y = (tile / tiles_x) * 8 + (uint32_t)(lane >> 3);
        if (x >= fp.width || y >= fp.height) continue;
        f2 screen_uv;                                                                  // RayGen.cuh:65-66
        screen_uv.x = ((float)x / (float)fp.width) * 2 - 1;
        screen_uv.y = ((float)y / (float)fp.height) * 2 - 1;
        uint32_t seed = x + y * fp.width;                                              // :74-75
        seed *= a.frame;
        const Ray ray = camera_get_ray(fp, screen_uv, seed);

        // ---- the closest-hit query at [0, FLT_MAX] (kernel_ray_query.hip, OCC = false) ----
        float best_t = FLT_MAX, best_u = 0.f, best_v = 0.f;                            // TraceRay.cu:18
        int best_prim = -1;
        uint32_t sp = 0;
        if (sc.root_ref != kNoNode) {
            s_ref[0][tid] = sc.root_ref;
            s_dist[0][tid] = slab_intersect(ld3(sc.root_min), ld3(sc.root_max), ray);
            sp = 1;
        }
        while (sp > 0) {
            --sp;
            uint32_t ref;
            float dist;
            if (sp < (uint32_t)K) {
                ref = s_ref[sp][tid];
                dist = s_dist[sp][tid];
            } else {
                const uint2 e = reinterpret_cast<const uint2 *>(a.stack_hbm)[(size_t)(sp - K) * gthreads + gthread];
                ref = e.x; dist = __uint_as_float(e.y);
            }
            if (!(-1.0f < dist && dist < FLT_MAX)) continue;                          // :38 interval (-1, FLT_MAX)
            if (best_prim >= 0 && best_t < dist) continue;                            // :41
            if (ref & kLeafBit) {
                const LeafRange leaf = sc.leaves[ref & ~kLeafBit];
                for (int i = leaf.start; i < leaf.start + leaf.count; i++) {           // :46-57
                    const TriTest tri = load_tri(sc.tri_hot, i);
                    float t, u, v;
                    const bool h = tri_intersect_flat(ray, tri.v0, tri.e1, tri.e2, t, u, v);
                    if (h && t < best_t && t > 0.f) {
                        if (!any_hit(sc, i, mk3(1.0f - u - v, u, v))) continue;
                        best_t = t; best_prim = i; best_u = u; best_v = v;
                    }
                }
            } else {
                const ChildPair c = load_children(sc.inner, ref);
                const float d1 = slab_intersect(c.min1, c.max1, ray);
                const float d2 = slab_intersect(c.min2, c.max2, ray);
                const bool push1 = d1 >= 0 && d1 < best_t, push2 = d2 >= 0 && d2 < best_t;       // :63-70
                const bool far1 = d1 > d2;                                                      // farther child first
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
                            s_dist[sp][tid] = d;
                        } else {
                            reinterpret_cast<uint2 *>(a.stack_hbm)[(size_t)(sp - K) * gthreads + gthread] = make_uint2(r, __float_as_uint(d));
                        }
                        ++sp;
                    }
                }
            }
        }

        // ---- the first trip of RayGen's loop, as the ALBEDO / NORMAL debug views see it ----
        const f3 zero = mk3(0, 0, 0), one = mk3(1, 1, 1);
        f3 albedo, normal = zero;
        if (best_prim < 0) {                                                           // :99-108 Miss
            const f3 sky = sky_model(ray.dir, ld3(fp.sky_color));
            albedo = zero + sky * one * fp.sky_intensity;
        } else {                                                                       // ClosestHit.cuh:4-28, RayGen.cuh:111-118
            f3 position, n;
            closest_hit_frame(ray, best_t, ld3(sc.tri_hot[best_prim].fn), position, n);
            const TriCold cold = sc.tri_cold[best_prim];
            const MatDev mat = sc.mats[cold.material];
            albedo = mat.tex < 0 ? one * ld3(mat.albedo) : one * tex_get_pixel(sc, sc.texs[mat.tex], interp_uv(cold, mk3(1.0f - best_u - best_v, best_u, best_v)));
            normal = n;
        }
        albedo = zero + albedo;                                                        // RenderKernel.cu:29 (a zeroed sum + the frame)
        normal = zero + normal;
        float4 *g = reinterpret_cast<float4 *>(a.out) + 2 * ((size_t)x + (size_t)y * fp.width);
        g[0] = make_float4(albedo.x, albedo.y, albedo.z, best_t);
        g[1] = make_float4(normal.x, normal.y, normal.z, __int_as_float(best_prim));
    }
}

constexpr int kAtrousTile = 16, kAtrousHalo = kAtrousTile + 4;

// B3 spline {1/16, 1/4, 3/8, 1/4, 1/16}: every product of two is exact in fp32
__constant__ float kB3[5] = { 0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f };

// One tap: colour and guides of q against those of p, in the order of drt.h (squared distances summed x, y, z)
DRT_DEV void atrous_tap(const AtrousPass &ps, float4 cp, f3 np, f3 ap, float4 cq, f3 nq, f3 aq, float h, float &wsum, f3 &csum) {
    const f3 dc = mk3(cp.x, cp.y, cp.z) - mk3(cq.x, cq.y, cq.z), dn = np - nq, da = ap - aq;
    const float e = dot(dc, dc) * ps.k_color + dot(dn, dn) * ps.k_normal + dot(da, da) * ps.k_albedo;
    const float w = h * expf(-e);
    wsum += w;
    csum = csum + mk3(cq.x, cq.y, cq.z) * w;
}

// Small steps: a workgroup filters a 16x16 tile of the pass's lattice -- pixels rx + (16 tx + i) s, ry + (16 ty + j) s -- whose
// 25 taps all fall on the same lattice.  The 20x20 lattice points of the tile and its halo (clamped to the image, as the taps
// are) are read once into LDS: 16 B of colour + 24 B of guide each, 16 KiB, then every tap is two LDS reads.  Blocks are handed
// to the XCDs in contiguous runs (block b runs on XCD b % 8), so that one XCD's L2 sees neighbouring residues of one region.
__global__ __launch_bounds__(kAtrousTile * kAtrousTile) void atrous_lds_kernel(const AtrousPass ps, uint32_t tiles_x, uint32_t n_blocks) {
    __shared__ float4 s_c[kAtrousHalo * kAtrousHalo];
    __shared__ float4 s_g0[kAtrousHalo * kAtrousHalo];          // normal.xyz, albedo.x
    __shared__ float2 s_g1[kAtrousHalo * kAtrousHalo];          // albedo.yz
    const uint32_t per_xcd = gridDim.x / 8, block = (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
    if (block >= n_blocks) return;                              // (whole workgroups: before any barrier)
    const int s = (int)ps.step, W = (int)ps.width, H = (int)ps.height;
    const uint32_t nx = tiles_x * (uint32_t)s;
    const uint32_t bx = block % nx, by = block / nx;
    const int rx = (int)(bx % (uint32_t)s), ry = (int)(by % (uint32_t)s);
    const int x0 = rx + (int)(bx / (uint32_t)s) * kAtrousTile * s, y0 = ry + (int)(by / (uint32_t)s) * kAtrousTile * s;     // lattice point (0, 0) of the tile
    const float *gd = reinterpret_cast<const float *>(ps.guides);
    for (int i = threadIdx.x; i < kAtrousHalo * kAtrousHalo; i += kAtrousTile * kAtrousTile) {
        const int lx = i % kAtrousHalo, ly = i / kAtrousHalo;
        const int qx = min(max(x0 + (lx - 2) * s, 0), W - 1), qy = min(max(y0 + (ly - 2) * s, 0), H - 1);
        const size_t q = (size_t)qx + (size_t)qy * (size_t)W;
        const float4 g0 = reinterpret_cast<const float4 *>(gd)[2 * q], g1 = reinterpret_cast<const float4 *>(gd)[2 * q + 1];
        s_c[i] = ps.in[q];
        s_g0[i] = make_float4(g1.x, g1.y, g1.z, g0.x);
        s_g1[i] = make_float2(g0.y, g0.z);
    }
    __syncthreads();
    const int tx = threadIdx.x % kAtrousTile, ty = threadIdx.x / kAtrousTile;
    const int x = x0 + tx * s, y = y0 + ty * s;
    if (x >= W || y >= H) return;
    const int c = (ty + 2) * kAtrousHalo + tx + 2;
    const float4 cp = s_c[c], gp = s_g0[c];
    const float2 gp1 = s_g1[c];
    const f3 np = mk3(gp.x, gp.y, gp.z), ap = mk3(gp.w, gp1.x, gp1.y);
    float wsum = 0.f;
    f3 csum = mk3(0, 0, 0);
    for (int b = 0; b < 5; b++) {
        for (int a = 0; a < 5; a++) {
            const int k = (ty + b) * kAtrousHalo + tx + a;
            const float4 g = s_g0[k];
            const float2 g1 = s_g1[k];
            atrous_tap(ps, cp, np, ap, s_c[k], mk3(g.x, g.y, g.z), mk3(g.w, g1.x, g1.y), kB3[a] * kB3[b], wsum, csum);
        }
    }
    const f3 out = csum / wsum;
    ps.out[(size_t)x + (size_t)y * (size_t)W] = make_float4(out.x, out.y, out.z, cp.w);
}

// Large steps (a lattice tile would be mostly outside the image): one pixel per lane, 16x16 pixels per workgroup, the taps read
// through the caches.
__global__ __launch_bounds__(kAtrousTile * kAtrousTile) void atrous_kernel(const AtrousPass ps) {
    const uint32_t x = blockIdx.x * kAtrousTile + threadIdx.x % kAtrousTile, y = blockIdx.y * kAtrousTile + threadIdx.x / kAtrousTile;
    if (x >= ps.width || y >= ps.height) return;
    const float *gd = reinterpret_cast<const float *>(ps.guides);
    const size_t p = (size_t)x + (size_t)y * ps.width;
    const float4 cp = ps.in[p];
    const f3 ap = ld3(gd + 8 * p), np = ld3(gd + 8 * p + 4);
    float wsum = 0.f;
    f3 csum = mk3(0, 0, 0);
    const int step = (int)ps.step;
    for (int b = 0; b < 5; b++) {
        const int qy = min(max((int)y + (b - 2) * step, 0), (int)ps.height - 1);
        for (int a = 0; a < 5; a++) {
            const int qx = min(max((int)x + (a - 2) * step, 0), (int)ps.width - 1);
            const size_t q = (size_t)qx + (size_t)qy * ps.width;
            atrous_tap(ps, cp, np, ap, ps.in[q], ld3(gd + 8 * q + 4), ld3(gd + 8 * q), kB3[a] * kB3[b], wsum, csum);
        }
    }
    const f3 out = csum / wsum;
    ps.out[p] = make_float4(out.x, out.y, out.z, cp.w);
}

}  // namespace

hipError_t launch_guides(const SceneView &sc, const FrameParams &fp, const GuideArgs &args, int num_cus, hipStream_t stream) {
    const uint32_t tiles = ((fp.width + 7) / 8) * ((fp.height + 7) / 8);
    if (tiles == 0) return hipSuccess;
    const uint32_t want = (tiles + kRqThreads / 64 - 1) / (kRqThreads / 64);
    const uint32_t blocks = std::min<uint32_t>(want, (uint32_t)ray_query_max_blocks(num_cus));
    hipLaunchKernelGGL(guide_kernel, dim3(blocks), dim3(kRqThreads), 0, stream, sc, fp, args);
    return hipGetLastError();
}

hipError_t launch_atrous(const AtrousPass &ps, FilterKernel which, hipStream_t stream) {
    if (ps.width == 0 || ps.height == 0) return hipSuccess;
    const dim3 block(kAtrousTile * kAtrousTile);
    const bool fits = ps.width >= 8 * ps.step && ps.height >= 8 * ps.step;      // at least half a lattice tile each way inside the image
    if (which == FilterKernel::automatic ? fits : which == FilterKernel::lds) {
        const uint32_t tiles_x = ((ps.width + ps.step - 1) / ps.step + kAtrousTile - 1) / kAtrousTile;
        const uint32_t tiles_y = ((ps.height + ps.step - 1) / ps.step + kAtrousTile - 1) / kAtrousTile;
        const uint32_t n = tiles_x * ps.step * tiles_y * ps.step;
        hipLaunchKernelGGL(atrous_lds_kernel, dim3((n + 7) / 8 * 8), block, 0, stream, ps, tiles_x, n);
    } else {
        const dim3 grid((ps.width + kAtrousTile - 1) / kAtrousTile, (ps.height + kAtrousTile - 1) / kAtrousTile);
        hipLaunchKernelGGL(atrous_kernel, grid, block, 0, stream, ps);
    }
    return hipGetLastError();
}

}  // namespace drt
