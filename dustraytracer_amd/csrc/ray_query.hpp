// ray_query.hpp -- launch seam of kernel_ray_query.hip (batched closest-hit / occlusion queries, include/drt.h
// drt_renderer_trace_rays / drt_renderer_occluded).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device_scene.hpp"

namespace drt {

constexpr int kRqThreads = 256;                 // 4 waves per workgroup
constexpr int kRqWavesPerSimd = 8;              // 8 workgroups per CU: <= 64 VGPRs, <= 20 KiB LDS per workgroup
constexpr int kRqLdsLevelsClosest = 8;          // stack levels kept in LDS: 8 x 256 x (4 B ref + 4 B entry distance) = 16 KiB
constexpr int kRqLdsLevelsOccluded = 16;        // 16 x 256 x 4 B ref = 16 KiB
constexpr int kRqShards = 16;                   // ray-claim heads, kRqShardStride words (128 B) apart
constexpr int kRqShardStride = 32;
constexpr int kRqHeadWords = kRqShards * kRqShardStride;
constexpr int kRqMaxLevels = 64;                // the reference's stack (BVHTraversal.cuh:17)

// the five fields every batched query's *Args carries (query_frame.hpp: the claim and the stack that read them).  It is defined
// here, with the constants, because RayQueryArgs below embeds it and query_frame.hpp includes this header.
struct QueryFrame {
    uint32_t n;                  // queries, < 2^31
    uint32_t stack_levels;       // tree depth (<= 64): the stack never holds more entries
    uint32_t refill_min;         // a wave claims new queries once this many of its lanes are idle (1..64)
    unsigned int *heads;         // kRqHeadWords zeroed words
    uint32_t *stack_hbm;         // levels beyond the LDS ones: [(level - K) * grid threads + thread], 8 B {ref, key} / 4 B ref entries
};

struct RayQueryArgs {
    const void *rays;            // drt_ray[n] (32 B, 16-B aligned)
    void *out;                   // drt_hit[n] (closest) or uint8_t[n] (occluded)
    QueryFrame frame;            // stack entries: 8 B (closest) / 4 B (occluded)
};

inline int ray_query_max_blocks(int num_cus) { return std::max(1, num_cus) * (kRqWavesPerSimd * 4 * 64 / kRqThreads); }
// bytes of HBM stack a launch over a tree of `levels` levels needs (0 when the LDS levels suffice)
inline size_t ray_query_stack_bytes(int num_cus, int levels, bool occluded) {
    const int k = occluded ? kRqLdsLevelsOccluded : kRqLdsLevelsClosest;
    if (levels <= k) return 0;
    return (size_t)(levels - k) * (size_t)ray_query_max_blocks(num_cus) * kRqThreads * (occluded ? 4u : 8u);
}

hipError_t launch_ray_query(const SceneView &scene, bool occluded, const RayQueryArgs &args, int num_cus, hipStream_t stream,
                            const char **kernel_name);

}  // namespace drt
