// denoise.hpp -- launch seam of kernel_denoise.hip: first-hit guide buffers (drt_renderer_render_guides) and the edge-avoiding
// a-trous filter (drt_renderer_denoise).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_scene.hpp"

namespace drt {

// One drt_guide (include/drt.h) per pixel: albedo[3], t, normal[3], prim -- 32 B, two 16-byte stores
struct GuideArgs {
    void *out;                   // drt_guide[width * height], 16-B aligned, pixel x + y * width (row 0 = bottom)
    uint32_t frame;              // frame index >= 1: seed = (x + y * width) * frame
    uint32_t stack_levels;       // tree depth (<= 64)
    uint32_t *stack_hbm;         // levels beyond the LDS ones, as the closest-hit ray query lays them out (ray_query_stack_bytes)
};

// The guide pass: the renderer's primary ray of every pixel (width, height and the camera from `frame`), the ray query's
// closest-hit traversal, and what the ALBEDO / NORMAL debug views make of the first hit.  The grid is the ray query's resident
// grid at most, so its HBM stack (ray_query_stack_bytes(num_cus, levels, false)) serves here too.
hipError_t launch_guides(const SceneView &scene, const FrameParams &frame, const GuideArgs &args, int num_cus, hipStream_t stream);

// One a-trous pass, step 2^pass: out = the filtered colour of `in` (float4[width * height]), alpha copied from `in`.
// k_color = 2^pass / sigma_color^2, k_normal = 1 / sigma_normal^2, k_albedo = 1 / sigma_albedo^2.
struct AtrousPass {
    const float4 *in;
    float4 *out;
    const void *guides;          // drt_guide[width * height]
    uint32_t width, height, step;
    float k_color, k_normal, k_albedo;
};
// Which of the two filter kernels a pass runs: the rule of launch_atrous (lattice tiles in LDS when width >= 8 * step and height >=
// 8 * step, cache-read taps otherwise), or one of them whatever the size (DRT_FILTER_KERNEL=lds|taps: both kernels clamp every tap,
// so both are valid at every size and step; for the tests, which compare the two bit for bit)
enum class FilterKernel : int32_t { automatic = 0, lds, taps };
hipError_t launch_atrous(const AtrousPass &pass, FilterKernel which, hipStream_t stream);

}  // namespace drt
