// kernel_temporal.hip -- temporal reprojection, moment accumulation and the variance-guided a-trous filter for gfx950
// (drt_renderer_temporal_denoise; the formulas and their order are those of include/drt.h, restated in tests/temporal_ref.py).
//
// temporal_reproject_kernel: one pixel per lane, a wave per 8x8 pixel tile (as guide_kernel), so that the four previous-frame taps
// of neighbouring lanes fall in the same cache lines.  The history is three 16-byte records per pixel (colour + N, key = normal +
// prim, moments + variance + weight sum): a tap reads its key first and the other two only when it is valid.  Memory-bound, no
// LDS, no atomics.  temporal_variance_kernel: the 7x7 spatial variance of the pixels whose history is shorter than 4 (every pixel
// on the first call, disocclusions later); a wave whose 64 pixels all have N >= 4 leaves after one load.
//
// atrous_var_lds_kernel / atrous_var_kernel: the filter of kernel_denoise.hip (restated here: that file's code objects stay as they
// are) with the colour term replaced by |l(p) - l(q)| / (sigma_luma * sqrtf(gv(p)) + 1e-4f) and the variance filtered along with
// the colour.  The variance rides in the colour record's fourth component, so the staged record stays 16 B + 24 B of guide and
// the 20x20 lattice tile stays 16 000 B of LDS; the 3x3 prefilter gv of the centre pixel is off the lattice for steps > 1 and is
// read through the caches (nine 4-byte reads of records the neighbouring blocks stage anyway).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_math.hpp"
#include "temporal.hpp"

namespace drt {

namespace {

constexpr int kTpThreads = 256;                  // 4 waves, one 8x8 pixel tile each

DRT_DEV float luminance(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }

__global__ __launch_bounds__(kTpThreads) void temporal_reproject_kernel(const ReprojectArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t tiles_x = (a.width + 7) / 8, tiles = tiles_x * ((a.height + 7) / 8);
    const uint32_t tile = blockIdx.x * (kTpThreads / 64) + threadIdx.x / 64;
    if (tile >= tiles) return;
    const uint32_t x = (tile % tiles_x) * 8 + (uint32_t)(lane & 7), y = (tile / tiles_x) * 8 + (uint32_t)(lane >> 3);
    if (x >= a.width || y >= a.height) return;
    const int W = (int)a.width, H = (int)a.height;
    const size_t p = (size_t)x + (size_t)y * a.width;
    const float4 c = a.frame[p];
    const float4 g0 = reinterpret_cast<const float4 *>(a.guides)[2 * p], g1 = reinterpret_cast<const float4 *>(a.guides)[2 * p + 1];
    const int prim = __float_as_int(g1.w);
    const f3 n = mk3(g1.x, g1.y, g1.z);
    const float l = luminance(c.x, c.y, c.z);

    float S = 0.f, sN = 0.f, sm1 = 0.f, sm2 = 0.f;
    f3 sc = mk3(0, 0, 0);
    if (a.has_prev && prim >= 0) {
        const float u = ((float)x / (float)a.width) * 2 - 1, v = ((float)y / (float)a.height) * 2 - 1;      // RayGen.cuh:65-66
        const f3 d0 = normalize(ld3(a.fwd_focus) + (u * ld3(a.horizontal)) + (v * ld3(a.vertical)));        // Camera::GetRay, no jitter, no defocus
        const f3 P = ld3(a.cam_pos) + d0 * g0.w;
        const f3 pv = P - ld3(a.pc.pos);
        const float z = dot(pv, ld3(a.pc.forward));
        if (z > 0.f) {
            const float su = (dot(pv, ld3(a.pc.right)) * a.pc.focus) / (z * a.pc.plane_w);
            const float sv = (dot(pv, ld3(a.pc.up)) * a.pc.focus) / (z * a.pc.plane_h);
            const float fx = ((su + 1.0f) * 0.5f) * (float)a.width, fy = ((sv + 1.0f) * 0.5f) * (float)a.height;
            if (fx > -1.0f && fx < (float)a.width && fy > -1.0f && fy < (float)a.height) {                  // (else every tap is outside; NaN lands here too)
                const float flx = floorf(fx), fly = floorf(fy);
                const int ix = (int)flx, iy = (int)fly;
                const float wx1 = fx - flx, wy1 = fy - fly, wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;
#pragma unroll
                for (int j = 0; j < 2; j++) {
#pragma unroll
                    for (int i = 0; i < 2; i++) {
                        const int qx = ix + i, qy = iy + j;
                        if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                        const size_t q = (size_t)qx + (size_t)qy * a.width;
                        const float4 k = a.prev.key[q];
                        if (__float_as_int(k.w) != prim) continue;
                        if (!(dot(mk3(k.x, k.y, k.z), n) >= a.normal_cos_min)) continue;
                        const float4 hc = a.prev.color[q], hm = a.prev.moments[q];
                        const float w = (i ? wx1 : wx0) * (j ? wy1 : wy0);
                        S += w;
                        sc = sc + mk3(hc.x, hc.y, hc.z) * w;
                        sN += hc.w * w;
                        sm1 += hm.x * w;
                        sm2 += hm.y * w;
                    }
                }
            }
        }
    }
    float N = 1.0f, m1 = l, m2 = l * l;
    f3 out = mk3(c.x, c.y, c.z);
    if (S >= 0.01f) {
        N = fminf(floorf(sN / S + 0.5f) + 1.0f, a.max_history);
        const float al = fmaxf(1.0f / N, a.alpha_min), om = 1.0f - al;
        out = (sc / S) * om + mk3(c.x, c.y, c.z) * al;
        m1 = (sm1 / S) * om + l * al;
        m2 = (sm2 / S) * om + (l * l) * al;
    }
    const float var = fmaxf(0.f, m2 - m1 * m1);  // N >= 4; shorter histories: temporal_variance_kernel
    a.cur.color[p] = make_float4(out.x, out.y, out.z, N);
    a.cur.key[p] = g1;
    a.cur.moments[p] = make_float4(m1, m2, var, S);
}

// Pixels with N < 4: variance = max(0, E[l^2] - E[l]^2) * (4 / N) over the 7x7 window (clamped to the image: dy outer, dx inner)
// of this call's integrated colour, pixels of the same prim only
__global__ __launch_bounds__(kTpThreads) void temporal_variance_kernel(const ReprojectArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t tiles_x = (a.width + 7) / 8, tiles = tiles_x * ((a.height + 7) / 8);
    const uint32_t tile = blockIdx.x * (kTpThreads / 64) + threadIdx.x / 64;
    if (tile >= tiles) return;
    const uint32_t x = (tile % tiles_x) * 8 + (uint32_t)(lane & 7), y = (tile / tiles_x) * 8 + (uint32_t)(lane >> 3);
    const bool inside = x < a.width && y < a.height;
    const size_t p = (size_t)x + (size_t)y * a.width;
    const float N = inside ? a.cur.color[p].w : 4.0f;
    if (!__any(N < 4.0f)) return;                // the whole wave has its temporal variance
    if (!(N < 4.0f)) return;
    const int W = (int)a.width, H = (int)a.height;
    const int prim = __float_as_int(a.cur.key[p].w);
    float s1 = 0.f, s2 = 0.f, cnt = 0.f;
    for (int dy = -3; dy <= 3; dy++) {
        const int qy = min(max((int)y + dy, 0), H - 1);
        for (int dx = -3; dx <= 3; dx++) {
            const int qx = min(max((int)x + dx, 0), W - 1);
            const size_t q = (size_t)qx + (size_t)qy * a.width;
            if (__float_as_int(a.cur.key[q].w) != prim) continue;
            const float4 cq = a.cur.color[q];
            const float lq = luminance(cq.x, cq.y, cq.z);
            s1 += lq;
            s2 += lq * lq;
            cnt += 1.0f;
        }
    }
    const float e1 = s1 / cnt, e2 = s2 / cnt;
    float4 m = a.cur.moments[p];
    m.z = fmaxf(0.f, e2 - e1 * e1) * (4.0f / N);
    a.cur.moments[p] = m;
}

__global__ __launch_bounds__(256) void temporal_copy_kernel(const float4 *in, float4 *out, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 c = in[i];
    out[i] = make_float4(c.x, c.y, c.z, 1.0f);
}

constexpr int kAtrousTile = 16, kAtrousHalo = kAtrousTile + 4;

// B3 spline {1/16, 1/4, 3/8, 1/4, 1/16}: every product of two is exact in fp32
__constant__ float kB3v[5] = { 0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f };

// The variance of pixel q as the pass reads it
DRT_DEV float var_of(const AtrousVarPass &ps, size_t q) { return ps.var_src ? ps.var_src[q].z : ps.in[q].w; }

// gv(p): the 3x3 Gaussian 1 2 1 / 2 4 2 / 1 2 1 over 16 of the variance, clamped to the image, dy outer and dx inner
DRT_DEV float prefiltered_variance(const AtrousVarPass &ps, int x, int y) {
    const int W = (int)ps.width, H = (int)ps.height;
    float gv = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = min(max(y + dy, 0), H - 1);
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = min(max(x + dx, 0), W - 1);
            const float k = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
            gv += k * var_of(ps, (size_t)qx + (size_t)qy * (size_t)W);
        }
    }
    return gv;
}

// One tap: q against p, in the order of drt.h (luminance term, then the normal and albedo distances summed x, y, z)
DRT_DEV void atrous_var_tap(const AtrousVarPass &ps, float lp, float inv_den, f3 np, f3 ap, float4 cq, f3 nq, f3 aq, float h, float &wsum,
                            f3 &csum, float &vsum) {
    const f3 dn = np - nq, da = ap - aq;
    const float lq = luminance(cq.x, cq.y, cq.z);
    const float e = fabsf(lp - lq) * inv_den + dot(dn, dn) * ps.k_normal + dot(da, da) * ps.k_albedo;
    const float w = h * expf(-e);
    wsum += w;
    csum = csum + mk3(cq.x, cq.y, cq.z) * w;
    vsum += (w * w) * cq.w;
}

// Small steps: a workgroup filters a 16x16 tile of the pass's lattice, staged with its halo in LDS (atrous_lds_kernel's scheme:
// 20x20 points of 16 B colour + variance and 24 B guide, 16 000 B; blocks handed to the XCDs in contiguous runs).
__global__ __launch_bounds__(kAtrousTile * kAtrousTile) void atrous_var_lds_kernel(const AtrousVarPass ps, uint32_t tiles_x, uint32_t n_blocks) {
    __shared__ float4 s_c[kAtrousHalo * kAtrousHalo];           // rgb, variance
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
        float4 c = ps.in[q];
        if (ps.var_src) c.w = ps.var_src[q].z;
        s_c[i] = c;
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
    const float lp = luminance(cp.x, cp.y, cp.z);
    const float inv_den = 1.0f / (ps.sigma_luma * sqrtf(prefiltered_variance(ps, x, y)) + 1e-4f);
    float wsum = 0.f, vsum = 0.f;
    f3 csum = mk3(0, 0, 0);
    for (int b = 0; b < 5; b++) {
        for (int a = 0; a < 5; a++) {
            const int k = (ty + b) * kAtrousHalo + tx + a;
            const float4 g = s_g0[k];
            const float2 g1 = s_g1[k];
            atrous_var_tap(ps, lp, inv_den, np, ap, s_c[k], mk3(g.x, g.y, g.z), mk3(g.w, g1.x, g1.y), kB3v[a] * kB3v[b], wsum, csum, vsum);
        }
    }
    const f3 out = csum / wsum;
    ps.out[(size_t)x + (size_t)y * (size_t)W] = make_float4(out.x, out.y, out.z, ps.last ? 1.0f : vsum / (wsum * wsum));
}

// Large steps (a lattice tile would be mostly outside the image): one pixel per lane, 16x16 pixels per workgroup, the taps read
// through the caches.
__global__ __launch_bounds__(kAtrousTile * kAtrousTile) void atrous_var_kernel(const AtrousVarPass ps) {
    const uint32_t x = blockIdx.x * kAtrousTile + threadIdx.x % kAtrousTile, y = blockIdx.y * kAtrousTile + threadIdx.x / kAtrousTile;
    if (x >= ps.width || y >= ps.height) return;
    const float *gd = reinterpret_cast<const float *>(ps.guides);
    const size_t p = (size_t)x + (size_t)y * ps.width;
    const float4 cp = ps.in[p];
    const f3 ap = ld3(gd + 8 * p), np = ld3(gd + 8 * p + 4);
    const float lp = luminance(cp.x, cp.y, cp.z);
    const float inv_den = 1.0f / (ps.sigma_luma * sqrtf(prefiltered_variance(ps, (int)x, (int)y)) + 1e-4f);
    float wsum = 0.f, vsum = 0.f;
    f3 csum = mk3(0, 0, 0);
    const int step = (int)ps.step;
    for (int b = 0; b < 5; b++) {
        const int qy = min(max((int)y + (b - 2) * step, 0), (int)ps.height - 1);
        for (int a = 0; a < 5; a++) {
            const int qx = min(max((int)x + (a - 2) * step, 0), (int)ps.width - 1);
            const size_t q = (size_t)qx + (size_t)qy * ps.width;
            float4 cq = ps.in[q];
            if (ps.var_src) cq.w = ps.var_src[q].z;
            atrous_var_tap(ps, lp, inv_den, np, ap, cq, ld3(gd + 8 * q + 4), ld3(gd + 8 * q), kB3v[a] * kB3v[b], wsum, csum, vsum);
        }
    }
    const f3 out = csum / wsum;
    ps.out[p] = make_float4(out.x, out.y, out.z, ps.last ? 1.0f : vsum / (wsum * wsum));
}

}  // namespace

hipError_t launch_temporal_reproject(const ReprojectArgs &args, int num_cus, hipStream_t stream) {
    (void)num_cus;
    const uint32_t tiles = ((args.width + 7) / 8) * ((args.height + 7) / 8);
    if (tiles == 0) return hipSuccess;
    const dim3 grid((tiles + kTpThreads / 64 - 1) / (kTpThreads / 64));
    hipLaunchKernelGGL(temporal_reproject_kernel, grid, dim3(kTpThreads), 0, stream, args);
    hipLaunchKernelGGL(temporal_variance_kernel, grid, dim3(kTpThreads), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_temporal_variance(const ReprojectArgs &args, hipStream_t stream) {
    const uint32_t tiles = ((args.width + 7) / 8) * ((args.height + 7) / 8);
    if (tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(temporal_variance_kernel, dim3((tiles + kTpThreads / 64 - 1) / (kTpThreads / 64)), dim3(kTpThreads), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_atrous_var(const AtrousVarPass &ps, FilterKernel which, hipStream_t stream) {
    if (ps.width == 0 || ps.height == 0) return hipSuccess;
    const dim3 block(kAtrousTile * kAtrousTile);
    const bool fits = ps.width >= 8 * ps.step && ps.height >= 8 * ps.step;      // launch_atrous's switch-over: at least half a lattice tile each way inside the image
    if (which == FilterKernel::automatic ? fits : which == FilterKernel::lds) {
        const uint32_t tiles_x = ((ps.width + ps.step - 1) / ps.step + kAtrousTile - 1) / kAtrousTile;
        const uint32_t tiles_y = ((ps.height + ps.step - 1) / ps.step + kAtrousTile - 1) / kAtrousTile;
        const uint32_t n = tiles_x * ps.step * tiles_y * ps.step;
        hipLaunchKernelGGL(atrous_var_lds_kernel, dim3((n + 7) / 8 * 8), block, 0, stream, ps, tiles_x, n);
    } else {
        const dim3 grid((ps.width + kAtrousTile - 1) / kAtrousTile, (ps.height + kAtrousTile - 1) / kAtrousTile);
        hipLaunchKernelGGL(atrous_var_kernel, grid, block, 0, stream, ps);
    }
    return hipGetLastError();
}

hipError_t launch_temporal_copy(const float4 *in, float4 *out, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(temporal_copy_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, in, out, n);
    return hipGetLastError();
}

}  // namespace drt
