// list_hits.hpp -- launch seam of kernel_list_hits.hip (ordered hit lists of rays: include/drt.h drt_renderer_list_hits).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_scene.hpp"
#include "ray_query.hpp"

namespace drt {

// The grid, the claim heads and the HBM stack are the occlusion ray query's (ray_query.hpp), as crossings.hpp's are: kRqThreads-thread
// workgroups, kRqWavesPerSimd waves per SIMD, kRqShards heads, kRqLdsLevelsOccluded reference-only stack levels in LDS and the rest in
// ray_query_stack_bytes(num_cus, levels, true) bytes of HBM.
struct ListHitsArgs {
    const void *rays;            // drt_ray[n] (32 B, 16-B aligned)
    const uint32_t *offsets;     // n + 1 words: ray i owns hits[offsets[i] .. offsets[i + 1]), clamped to hits_capacity
    void *hits;                  // drt_hit[hits_capacity] (16 B, 16-B aligned); may be null when hits_capacity == 0
    uint32_t *counts;            // n words or null: every listed triangle of the ray, stored or not
    uint32_t hits_capacity;
    QueryFrame frame;            // n, tree depth, refill threshold, claim heads, HBM stack: 4 B stack entries
};

hipError_t launch_list_hits(const SceneView &scene, const ListHitsArgs &args, int num_cus, hipStream_t stream);

}  // namespace drt
