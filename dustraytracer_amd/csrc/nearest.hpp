// nearest.hpp -- launch seam of kernel_nearest.hip (batched closest-point-on-mesh queries, include/drt.h drt_renderer_nearest).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_scene.hpp"
#include "ray_query.hpp"

namespace drt {

// The grid, the claim heads and the HBM stack are the closest-hit ray query's (ray_query.hpp): kRqThreads-thread workgroups,
// kRqWavesPerSimd waves per SIMD, kRqShards heads, kRqLdsLevelsClosest stack levels {ref, box2} in LDS and the rest in
// ray_query_stack_bytes(num_cus, levels, false) bytes of HBM.
struct NearestArgs {
    const void *points;          // drt_point[n] (16 B, 16-B aligned)
    void *out;                   // drt_nearest[n] (32 B, 16-B aligned)
    QueryFrame frame;            // n, tree depth, refill threshold, claim heads, HBM stack: 8 B stack entries
};

hipError_t launch_nearest(const SceneView &scene, const NearestArgs &args, int num_cus, hipStream_t stream);

}  // namespace drt
