// kernel_motion.hip -- the temporal reprojection for geometry that a device refit moved, and the motion-vector buffer, for gfx950
// (drt_renderer_track_motion, drt_renderer_motion_vectors; the rule and its order are those of include/drt.h, restated in
// tests/motion_ref.py).
//
// A refit keeps TriHot record k the same surface, so the point a pixel sees is carried back by its barycentric coordinates: solved
// on the current record (v0, e1, e2), applied to the snapshot's (v0', e1', e2').  previous_point() is that rule; the two kernels
// differ only in what they do with P'.
//
// motion_reproject_kernel: temporal_reproject_kernel of kernel_temporal.hip restated (that file's code objects stay as they are:
// they are what runs with tracking off or nothing armed) with P' in place of P and the tap's normal test against the previous
// face normal; the variance pass after it is kernel_temporal.hip's own (launch_temporal_variance).  motion_vectors_kernel: the
// projection of P' alone, one float4 per pixel.  Both: one pixel per lane, a wave per 8x8 pixel tile; neighbouring lanes mostly share a prim, so
// the two 48-byte records are cache hits.  No LDS, no atomics.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "motion.hpp"

namespace drt {

namespace {

constexpr int kMvThreads = 256;                  // 4 waves, one 8x8 pixel tile each

DRT_DEV float luminance(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }

DRT_DEV bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }

// The nine words v0, e1, e2 of two TriHot records, each read as three float4
DRT_DEV bool same_position_words(float4 h0, float4 h1, float4 h2, float4 s0, float4 s1, float4 s2) {
    return same_bits(h0.x, s0.x) && same_bits(h0.y, s0.y) && same_bits(h0.z, s0.z) && same_bits(h0.w, s0.w) && same_bits(h1.x, s1.x) &&
           same_bits(h1.y, s1.y) && same_bits(h1.z, s1.z) && same_bits(h1.w, s1.w) && same_bits(h2.x, s2.x);
}

// P' and the normal n' a tap's stored normal is compared with, for the pixel's point P on triangle `prim` (>= 0) with guide normal n.
// Returns false (P' = P, n' = n: the static rule) when there is no snapshot, the triangle did not move or it has no area.
DRT_DEV bool previous_point(const MotionGeometry &geo, int prim, f3 P, f3 n, f3 &Pp, f3 &np) {
    Pp = P;
    np = n;
    if (!geo.snapshot) return false;
    const size_t k = 3 * (size_t)prim;
    const float4 h0 = geo.hot[k], h1 = geo.hot[k + 1], h2 = geo.hot[k + 2];
    const float4 s0 = geo.snapshot[k], s1 = geo.snapshot[k + 1], s2 = geo.snapshot[k + 2];
    if (same_position_words(h0, h1, h2, s0, s1, s2)) return false;
    const f3 v0 = mk3(h0.x, h0.y, h0.z), e1 = mk3(h0.w, h1.x, h1.y), e2 = mk3(h1.z, h1.w, h2.x), fn = mk3(h2.y, h2.z, h2.w);
    const f3 w = P - v0;
    const float d11 = dot(e1, e1), d12 = dot(e1, e2), d22 = dot(e2, e2), w1 = dot(w, e1), w2 = dot(w, e2);
    const float den = d11 * d22 - d12 * d12;
    if (!(den > 0.f)) return false;              // zero area, NaN
    const float b1 = (d22 * w1 - d12 * w2) / den, b2 = (d11 * w2 - d12 * w1) / den;
    const f3 pv0 = mk3(s0.x, s0.y, s0.z), pe1 = mk3(s0.w, s1.x, s1.y), pe2 = mk3(s1.z, s1.w, s2.x), pfn = mk3(s2.y, s2.z, s2.w);
    Pp = (pv0 + pe1 * b1) + pe2 * b2;
    np = dot(fn, n) < 0.f ? mk3(-pfn.x, -pfn.y, -pfn.z) : pfn;
    return true;
}

__global__ __launch_bounds__(kMvThreads) void motion_reproject_kernel(const ReprojectArgs a, const MotionGeometry geo) {
    const int lane = threadIdx.x & 63;
    const uint32_t tiles_x = (a.width + 7) / 8, tiles = tiles_x * ((a.height + 7) / 8);
    const uint32_t tile = blockIdx.x * (kMvThreads / 64) + threadIdx.x / 64;
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
        const float u = ((float)x / (float)a.width) * 2 - 1, v = ((float)y / (float)a.height) * 2 - 1;
        const f3 d0 = normalize(ld3(a.fwd_focus) + (u * ld3(a.horizontal)) + (v * ld3(a.vertical)));
        const f3 P = ld3(a.cam_pos) + d0 * g0.w;
        f3 Pp, nt;
        previous_point(geo, prim, P, n, Pp, nt);
        const f3 pv = Pp - ld3(a.pc.pos);
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
                        if (!(dot(mk3(k.x, k.y, k.z), nt) >= a.normal_cos_min)) continue;
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
    a.cur.key[p] = g1;                           // the CURRENT normal and prim
    a.cur.moments[p] = make_float4(m1, m2, var, S);
}

__global__ __launch_bounds__(kMvThreads) void motion_vectors_kernel(const ReprojectArgs a, const MotionGeometry geo, float4 *out) {
    const int lane = threadIdx.x & 63;
    const uint32_t tiles_x = (a.width + 7) / 8, tiles = tiles_x * ((a.height + 7) / 8);
    const uint32_t tile = blockIdx.x * (kMvThreads / 64) + threadIdx.x / 64;
    if (tile >= tiles) return;
    const uint32_t x = (tile % tiles_x) * 8 + (uint32_t)(lane & 7), y = (tile / tiles_x) * 8 + (uint32_t)(lane >> 3);
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)x + (size_t)y * a.width;
    const float4 g0 = reinterpret_cast<const float4 *>(a.guides)[2 * p], g1 = reinterpret_cast<const float4 *>(a.guides)[2 * p + 1];
    const int prim = __float_as_int(g1.w);
    float4 mv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (prim >= 0) {
        const float u = ((float)x / (float)a.width) * 2 - 1, v = ((float)y / (float)a.height) * 2 - 1;
        const f3 d0 = normalize(ld3(a.fwd_focus) + (u * ld3(a.horizontal)) + (v * ld3(a.vertical)));
        const f3 P = ld3(a.cam_pos) + d0 * g0.w;
        f3 Pp, nt;
        const bool moved = previous_point(geo, prim, P, mk3(g1.x, g1.y, g1.z), Pp, nt);
        const f3 pv = Pp - ld3(a.pc.pos);
        const float z = dot(pv, ld3(a.pc.forward));
        if (z > 0.f) {
            const float su = (dot(pv, ld3(a.pc.right)) * a.pc.focus) / (z * a.pc.plane_w);
            const float sv = (dot(pv, ld3(a.pc.up)) * a.pc.focus) / (z * a.pc.plane_h);
            const float fx = ((su + 1.0f) * 0.5f) * (float)a.width, fy = ((sv + 1.0f) * 0.5f) * (float)a.height;
            mv = make_float4(fx - (float)x, fy - (float)y, z, moved ? 2.0f : 1.0f);
        }
    }
    out[p] = mv;
}

dim3 tile_grid(const ReprojectArgs &args) {
    const uint32_t tiles = ((args.width + 7) / 8) * ((args.height + 7) / 8);
    return dim3((tiles + kMvThreads / 64 - 1) / (kMvThreads / 64));
}

}  // namespace

hipError_t launch_motion_reproject(const ReprojectArgs &args, const MotionGeometry &geo, hipStream_t stream) {
    if (args.width == 0 || args.height == 0) return hipSuccess;
    const dim3 grid = tile_grid(args);
    hipLaunchKernelGGL(motion_reproject_kernel, grid, dim3(kMvThreads), 0, stream, args, geo);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : launch_temporal_variance(args, stream);
}

hipError_t launch_motion_vectors(const ReprojectArgs &args, const MotionGeometry &geo, float4 *out, hipStream_t stream) {
    if (args.width == 0 || args.height == 0) return hipSuccess;
    hipLaunchKernelGGL(motion_vectors_kernel, tile_grid(args), dim3(kMvThreads), 0, stream, args, geo, out);
    return hipGetLastError();
}

}  // namespace drt
