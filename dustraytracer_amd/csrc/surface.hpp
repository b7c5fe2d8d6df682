// surface.hpp -- surface lookups and area-weighted sampling (drt_renderer_surface_lookup / _surface_weights / _sample_surface,
// kernel_surface.hip).  The reference has neither; include/drt.h states both rules bit for bit, and the per-record routines below are
// those rules, one operation per header operation.  They are compiled for the device by kernel_surface.hip and, unchanged, for the host
// by the stand-alone check of DESIGN 5.29 (a plain C++ compiler: nothing here needs the HIP runtime), so they use no device-only helper.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "device_scene.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DRT_SURF_FN __host__ __device__ inline
#else
#define DRT_SURF_FN inline
#endif

namespace drt {

constexpr int kSurfThreads = 256;                 // workgroup size of every kernel here
constexpr uint32_t kSurfScanBlock = 256;          // triangles per workgroup of the scan = DRT_SURFACE_SCAN_BLOCK (one per thread)

struct alignas(16) SurfQuad { uint32_t x, y, z, w; };
struct alignas(16) SurfRecord { SurfQuad q[6]; };                       // drt_surface as its six 16-byte words
struct alignas(16) SurfRef { float t; int32_t prim; float u, v; };      // drt_hit
static_assert(sizeof(SurfRecord) == 96 && sizeof(SurfRef) == 16, "drt_surface / drt_hit layout");

struct SurfaceArgs {
    const SurfRef *refs;
    SurfRecord *out;
    uint32_t n;
    const float *own_normals;      // float[n_tris][3][3] in TREE order: the host scene's vertex normals (the renderer's copy)
    const int32_t *load_index;     // tree order -> load order (drt_scene_get_triangle_order)
    const float *normals;          // the caller's float[n_tris][3][3] in LOAD order, or nullptr
};

DRT_SURF_FN uint32_t surf_bits(float x) { uint32_t b; std::memcpy(&b, &x, 4); return b; }
DRT_SURF_FN SurfQuad surf_quad(float x, float y, float z, uint32_t w) { return SurfQuad{ surf_bits(x), surf_bits(y), surf_bits(z), w }; }

// The miss record: all zero bits except material = load_index = texture = -1
DRT_SURF_FN SurfRecord surface_miss() {
    SurfRecord r;
    for (int k = 0; k < 6; k++) r.q[k] = SurfQuad{ 0u, 0u, 0u, 0u };
    r.q[0].w = r.q[2].w = r.q[3].w = 0xFFFFFFFFu;
    return r;
}

// One texel coordinate (Texture.cu:35-36): (int)((c - floorf(c)) * size), with the one departure -- a fractional part that is not in
// [0, 1] (a NaN: the uv was a NaN or an infinity) is taken as 0, so the index stays inside the texture's padded extent
DRT_SURF_FN int surface_texel_coord(float c, int32_t size) {
    float f = c - floorf(c);
    if (!(f >= 0.0f && f <= 1.0f)) f = 0.0f;
    return (int)(f * size);
}

DRT_SURF_FN SurfRecord surface_lookup_one(const SceneView &sc, const SurfaceArgs &a, int32_t prim, float u, float v) {
    if (prim < 0 || (uint32_t)prim >= sc.n_tris) return surface_miss();
    const TriHot hot = sc.tri_hot[prim];
    const TriCold cold = sc.tri_cold[prim];
    const int32_t load = a.load_index[prim];
    const float *nrm = a.normals ? a.normals + 9 * (size_t)(uint32_t)load : a.own_normals + 9 * (size_t)(uint32_t)prim;
    const MatDev mat = sc.mats[cold.material];
    const MatExt ext = sc.mats_ext[cold.material];
    const float w = 1.0f - u - v;                                                  // Intersection.cu's
    float pos[3], shd[3];
    for (int k = 0; k < 3; k++) {
        pos[k] = (hot.v0[k] + u * hot.e1[k]) + v * hot.e2[k];
        shd[k] = (w * nrm[k] + u * nrm[3 + k]) + v * nrm[6 + k];
    }
    const float uvx = (w * cold.uv[0][0] + u * cold.uv[1][0]) + v * cold.uv[2][0];   // interp_uv (RayGen.cuh:116)
    const float uvy = (w * cold.uv[0][1] + u * cold.uv[1][1]) + v * cold.uv[2][1];
    float alb[3] = { mat.albedo[0], mat.albedo[1], mat.albedo[2] };
    float alpha = 1.0f;
    if (mat.tex >= 0) {
        const TexDev tex = sc.texs[mat.tex];
        const int x = surface_texel_coord(uvx, tex.width), y = surface_texel_coord(uvy, tex.height);
        const uint32_t i = (uint32_t)(y * tex.width + x);
        float r = 0, g = 0, b = 255;                                               // Texture.cu:33-58
        if (tex.comps == 3 || tex.comps == 4) {
            const uint8_t *p = sc.texels + tex.offset + (size_t)i * (uint32_t)tex.comps;
            r = p[0]; g = p[1]; b = p[2];
        }
        r = r / (float)255; g = g / (float)255; b = b / (float)255;
        alb[0] = r * r; alb[1] = g * g; alb[2] = b * b;
        if (!(tex.comps < 4)) alpha = sc.texels[tex.offset + (size_t)i * 4u + 3u] / (float)255;   // Texture.cu:60-75
    }
    SurfRecord o;
    o.q[0] = surf_quad(pos[0], pos[1], pos[2], (uint32_t)cold.material);
    o.q[1] = SurfQuad{ surf_bits(hot.fn[0]), surf_bits(hot.fn[1]), surf_bits(hot.fn[2]), surf_bits(alpha) };
    o.q[2] = surf_quad(shd[0], shd[1], shd[2], (uint32_t)load);
    o.q[3] = surf_quad(alb[0], alb[1], alb[2], (uint32_t)(mat.tex >= 0 ? mat.tex : -1));
    o.q[4] = SurfQuad{ surf_bits(uvx), surf_bits(uvy), surf_bits(ext.roughness), (ext.metallic ? 1u : 0u) | (ext.transmission ? 2u : 0u) };
    o.q[5] = SurfQuad{ surf_bits(ext.emissive[0]), surf_bits(ext.emissive[1]), surf_bits(ext.emissive[2]), surf_bits(ext.refractive_index) };
    return o;
}

// ---- weights ----
// a = |cross(e1, e2)| (twice the area), a non-finite one counts as 0
DRT_SURF_FN float surface_area2(const TriHot &h) {
    const float cx = h.e1[1] * h.e2[2] - h.e1[2] * h.e2[1];
    const float cy = h.e1[2] * h.e2[0] - h.e1[0] * h.e2[2];
    const float cz = h.e1[0] * h.e2[1] - h.e1[1] * h.e2[0];
    const float a = sqrtf((cx * cx + cy * cy) + cz * cz);
    return a <= FLT_MAX ? a : 0.0f;                           // (a NaN fails the test too)
}
// frexp's exponent of a positive finite float from its bits: amax = m 2^e with m in [0.5, 1), subnormals included
DRT_SURF_FN int surface_exponent(uint32_t amax_bits) {
    const int field = (int)(amax_bits >> 23);
    if (field) return field - 126;
    return (31 - __builtin_clz(amax_bits)) - 148;             // the highest set bit p of the mantissa: 2^(p - 149) <= amax
}
// q = (uint64_t)ldexp((double)a, 35 - e), truncated: the scaling is a product with a power of two, exact in double (35 - e lies in
// [-93, 183]).  a <= amax < 2^e, so q < 2^35
DRT_SURF_FN uint64_t surface_weight(float a, int e) {
    const uint64_t pow_bits = (uint64_t)(35 - e + 1023) << 52;
    double scale;
    std::memcpy(&scale, &pow_bits, 8);
    return (uint64_t)((double)a * scale);
}

// ---- samples ----
DRT_SURF_FN uint32_t surf_pcg(uint32_t input) {               // the reference's pcg_hash, Random.cu:6-11
    const uint32_t state = input * 747796405u + 2891336453u;
    const uint32_t word = ((state >> ((state >> 28u) + 4u)) ^ state) * 277803737u;
    return (word >> 22u) ^ word;
}
DRT_SURF_FN uint64_t surf_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}
// Sample i of the stream `seed` (seed_hash = pcg(seed)) from the inclusive table cdf[n_tris]; n_tris == 0 or a total of 0: the miss
// record {0, -1, 0, 0}
DRT_SURF_FN SurfRef surface_sample_one(uint32_t seed_hash, uint32_t i, const uint64_t *cdf, uint32_t n_tris) {
    const uint64_t total = n_tris ? cdf[n_tris - 1] : 0;
    if (total == 0) return SurfRef{ 0.0f, -1, 0.0f, 0.0f };
    const uint32_t s = surf_pcg(i ^ seed_hash);
    const uint32_t h1 = surf_pcg(s), h2 = surf_pcg(h1), h3 = surf_pcg(h2), h4 = surf_pcg(h3);
    const uint64_t target = surf_mulhi((uint64_t)h1 << 32 | h2, total);           // < total
    uint32_t lo = 0, hi = n_tris - 1;                                              // the smallest k with cdf[k] > target
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (cdf[mid] > target) hi = mid; else lo = mid + 1;
    }
    uint32_t a = h3 >> 8, b = h4 >> 8;
    if (a + b > (1u << 24)) { a = (1u << 24) - a; b = (1u << 24) - b; }
    return SurfRef{ 0.0f, (int32_t)lo, (float)a * 0x1p-24f, (float)b * 0x1p-24f };
}

#if defined(__HIPCC__)
struct SurfaceScanArgs {
    const TriHot *hot;
    uint32_t n_tris;
    uint32_t *amax_bits;           // one word, zeroed on the stream before the first kernel
    uint64_t *block_totals;        // ceil(n_tris / kSurfScanBlock) words
    uint64_t *cdf;                 // n_tris words
};
hipError_t launch_surface_lookup(const SceneView &sc, const SurfaceArgs &args, int num_cus, hipStream_t stream);
hipError_t launch_surface_weights(const SurfaceScanArgs &args, hipStream_t stream);       // n_tris > 0
hipError_t launch_surface_sample(const uint64_t *cdf, uint32_t n_tris, uint32_t seed, uint32_t first, SurfRef *out, uint32_t n,
                                 int num_cus, hipStream_t stream);
#endif

}  // namespace drt
