// ambient.hpp -- ambient occlusion: cosine-weighted visibility at surface points (drt_renderer_ambient_occlusion,
// kernel_ambient.hip).  The reference has no such query; include/drt.h states the rule bit for bit, and the routines below are that
// rule, one operation per header operation: the tile arithmetic (which point and which sample a lane of a 64-lane tile holds) and the
// ray rule (the ray of sample j of point i, and what an open sample adds to the record).  They are compiled for the device by
// kernel_ambient.hip and, unchanged, for the host by the stand-alone check of DESIGN 5.30 (a plain C++ compiler: nothing here needs the
// HIP runtime).  One seam: 1 / sqrtf(x) is the plain correctly rounded pair on the host and device_math.hpp's exact fast forms on the
// device, which equal the plain operators for every float (tests/test_gpu_parity.py, all 2^32 bit patterns).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "device_math.hpp"
#include "device_scene.hpp"
#include "ray_query.hpp"
#define DRT_AO_FN __host__ __device__ inline
#else
#define DRT_AO_FN inline
#endif

namespace drt {

constexpr uint32_t kAoMaxSamples = 4096;          // |bent[k]| <= 4096 * 65536 = 2^28
constexpr int kAoMaxTries = 1024;                 // device_math.hpp's kMaxTries: the cycle guard of the rejection loop
constexpr int kAoHeadStride = 16;                 // 64-bit claim heads, 128 bytes apart (kRqShards of them)

struct alignas(16) AoPoint { float p[3]; float max_dist; float n[3]; float bias; };   // drt_ao_point
struct alignas(16) AoResult { int32_t open; int32_t bent[3]; };                      // drt_ao_result
static_assert(sizeof(AoPoint) == 32 && sizeof(AoResult) == 16, "drt_ao_point / drt_ao_result layout");

// ---- tiles: the work unit is 64 lanes ----
//   S >= 64                   samples [64 t, min(64 t + 64, S)) of one point: ceil(S / 64) tiles per point
//   S in {1, 2, 4, 8, 16, 32} 64 / S consecutive points, S lanes each ("packed")
//   any other S < 64          one point, lanes S .. 63 idle
struct AoTiling {
    uint32_t samples;        // S
    uint32_t seg;            // lanes per point in a tile: S (packed), else 64
    uint32_t per_point;      // tiles per point (S >= 64), else 1
    uint32_t per_tile;       // points per tile (packed), else 1
};
DRT_AO_FN AoTiling ao_tiling(uint32_t samples) {
    AoTiling t;
    t.samples = samples;
    const bool packed = samples < 64u && (samples & (samples - 1u)) == 0u;
    t.seg = packed ? samples : 64u;
    t.per_point = samples >= 64u ? (samples + 63u) / 64u : 1u;
    t.per_tile = packed ? 64u / samples : 1u;
    return t;
}
// the number of tiles of n points, in 64 bits (n = 2^32 - 1 with S = 4096: 2^38 - 64)
DRT_AO_FN uint64_t ao_tile_count(const AoTiling &t, uint32_t n) {
    if (t.per_tile > 1u) return ((uint64_t)n + t.per_tile - 1u) / t.per_tile;
    return (uint64_t)n * t.per_point;
}
// Lane `lane` of tile `tile`: its point and its sample.  false: the lane is idle (a sample beyond S, or a point beyond n in the last
// packed tile)
DRT_AO_FN bool ao_tile_lane(const AoTiling &t, uint64_t tile, uint32_t lane, uint32_t n, uint32_t &point, uint32_t &sample) {
    uint64_t i;
    if (t.per_tile > 1u) { i = tile * t.per_tile + lane / t.seg; sample = lane % t.seg; }
    else if (t.per_point > 1u) { i = tile / t.per_point; sample = (uint32_t)(tile % t.per_point) * 64u + lane; }
    else { i = tile; sample = lane; }
    point = (uint32_t)i;
    return i < (uint64_t)n && sample < t.samples;
}
// shard s of `shards` covers tiles [count s / shards, count (s + 1) / shards): count < 2^38, so the product stays in 64 bits
DRT_AO_FN uint64_t ao_shard_begin(uint64_t count, uint32_t s, uint32_t shards) { return count * s / shards; }

// ---- the ray rule ----
DRT_AO_FN uint32_t ao_pcg(uint32_t input) {               // the reference's pcg_hash, Random.cu:6-11
    const uint32_t state = input * 747796405u + 2891336453u;
    const uint32_t word = ((state >> ((state >> 28u) + 4u)) ^ state) * 277803737u;
    return (word >> 22u) ^ word;
}
DRT_AO_FN float ao_dot(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }   // helper_math.cuh:1264
DRT_AO_FN float ao_inv_sqrt(float x) {                    // 1.0f / sqrtf(x), both correctly rounded (helper_math.cuh:78-81)
#if defined(__HIP_DEVICE_COMPILE__)
    return exact_rcp(exact_sqrt(x));
#else
    return 1.0f / sqrtf(x);
#endif
}
DRT_AO_FN void ao_normalize(float v[3]) {                 // helper_math.cuh:1325
    const float inv_len = ao_inv_sqrt(ao_dot(v, v));
    v[0] = v[0] * inv_len; v[1] = v[1] * inv_len; v[2] = v[2] * inv_len;
}
// randomUnitSphereVec3 (Random.cu:50-58) with the renderer's cycle guard: candidates (float)seed / 2^32 * 2 - 1 per component (x, then
// y, then z), normalised, until len * len < 1 with len = sqrtf(dot(p, p)) or kAoMaxTries candidates were drawn.  fl(fl(sqrt(d))^2) < 1
// <=> d < 1 for every float d (tests/test_oracle_kat.py::test_sphere_accept_shortcut), and the two scalings of the candidate are exact,
// so this is device_math.hpp's random_unit_sphere_vec3, which oracle.kat_unitsphere pins.
DRT_AO_FN void ao_unit_sphere(uint32_t &seed, float p[3]) {
    for (int tries = 1;; tries++) {
        for (int k = 0; k < 3; k++) { seed = ao_pcg(seed); p[k] = (float)seed * 0x1p-31f - 1.0f; }
        ao_normalize(p);
        if (ao_dot(p, p) < 1.0f || tries >= kAoMaxTries) return;
    }
}
// seed_hash = pcg(seed).  The ray of sample j of point index i (= first + the point's position in the call)
DRT_AO_FN void ao_ray(const AoPoint &pt, uint32_t seed_hash, uint32_t i, uint32_t j, float o[3], float d[3]) {
    const uint32_t h = ao_pcg(i ^ seed_hash);
    uint32_t state = ao_pcg(j ^ h);
    float fuzz[3];
    ao_unit_sphere(state, fuzz);
    for (int k = 0; k < 3; k++) d[k] = pt.n[k] + fuzz[k];
    ao_normalize(d);
    for (int k = 0; k < 3; k++) o[k] = pt.p[k] + pt.n[k] * pt.bias;
}
// What an open sample adds to bent[k]: (int32_t)(d[k] * 65536.0f), truncated; a product that is a NaN or not below 2^31 in magnitude
// (the cast is undefined there; only a NaN or a zero n + fuzz gets that far) adds 0
DRT_AO_FN int32_t ao_bent_term(float dk) {
    const float c = dk * 65536.0f;
    return fabsf(c) < 2147483648.0f ? (int32_t)c : 0;
}
// a point with !(max_dist >= 0) is skipped: no rays, the record {-1, 0, 0, 0}
DRT_AO_FN bool ao_live(float max_dist) { return max_dist >= 0.0f; }

#if defined(__HIPCC__)
struct AmbientArgs {
    const AoPoint *pts;
    AoResult *out;
    uint32_t n;                  // < 2^31
    uint32_t samples, seed_hash, first;
    uint32_t stack_levels;       // tree depth (<= 64)
    unsigned long long *heads;   // kRqShards heads, kAoHeadStride words apart, zeroed
    uint32_t *stack_hbm;         // the occlusion ray query's: ray_query_stack_bytes(num_cus, levels, true)
};
// the records of skipped points, and zeros for the others where the tracing kernel adds to them (S > 64)
hipError_t launch_ambient_init(const AmbientArgs &args, hipStream_t stream);
// stats != nullptr: the counting build, which adds {trips of the waves' traversal loops, lanes that took a step in them} to stats[0..1]
hipError_t launch_ambient(const SceneView &scene, const AmbientArgs &args, int num_cus, unsigned long long *stats, hipStream_t stream);
#endif

}  // namespace drt
