// sphere_cast.hpp -- launch seam of kernel_sphere_cast.hip (batched sphere casts, include/drt.h drt_renderer_sphere_cast).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_scene.hpp"
#include "ray_query.hpp"

namespace drt {

// The grid, the claim heads and the HBM stack are the closest-hit ray query's (ray_query.hpp): kRqThreads-thread workgroups,
// kRqWavesPerSimd waves per SIMD, kRqShards heads, kRqLdsLevelsClosest stack levels {ref, enter} in LDS and the rest in
// ray_query_stack_bytes(num_cus, levels, false) bytes of HBM.

struct SphereCastArgs {
    const void *rays;            // drt_ray[n] (32 B, 16-B aligned)
    const float *radii;          // float[n]
    void *out;                   // drt_sweep_hit[n] (32 B, 16-B aligned)
    QueryFrame frame;            // n, tree depth, refill threshold, claim heads, HBM stack: 8 B stack entries
};

hipError_t launch_sphere_cast(const SceneView &scene, const SphereCastArgs &args, int num_cus, hipStream_t stream);

}  // namespace drt
