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
    uint32_t n;                  // < 2^31
    uint32_t stack_levels;       // tree depth (<= 64): the stack never holds more entries
    uint32_t refill_min;         // a wave claims new casts once this many of its lanes are idle (1..64)
    unsigned int *heads;         // kRqHeadWords zeroed words
    uint32_t *stack_hbm;         // levels beyond the LDS ones: [(level - K) * grid threads + thread], 8 B entries
};

hipError_t launch_sphere_cast(const SceneView &scene, const SphereCastArgs &args, int num_cus, hipStream_t stream);

}  // namespace drt
