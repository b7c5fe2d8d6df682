// upscale.hpp -- launch seam of kernel_upscale.hip: joint-bilateral upsampling of a low-resolution colour image, steered by the
// first-hit guides of both resolutions (drt_renderer_upscale, include/drt.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace drt {

struct UpscaleArgs {
    const float4 *color;         // the source colour, float4[width * height] (row 0 = bottom)
    const void *guides_lo;       // drt_guide[width * height]: frame 1's guides at the source size
    const void *guides_hi;       // drt_guide[out_width * out_height]: frame 1's guides at the output size
    float4 *out;                 // float4[out_width * out_height]
    uint32_t width, height, out_width, out_height;      // out_width >= width >= 1, out_height >= height >= 1
    int32_t demodulate;          // 0 / 1: interpolate colour / colour divided by the first hit's albedo
    float k_normal, k_albedo;    // 1 / sigma_normal^2, 1 / sigma_albedo^2
    float sigma_depth, albedo_floor;
};
// One launch on `stream`: one output pixel per lane.
hipError_t launch_upscale(const UpscaleArgs &args, hipStream_t stream);

}  // namespace drt
