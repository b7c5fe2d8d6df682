// temporal.hpp -- launch seam of kernel_temporal.hip: temporal reprojection, moment accumulation and the variance-guided a-trous
// filter of drt_renderer_temporal_denoise (include/drt.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "denoise.hpp"

namespace drt {

// One half of the ping-pong history: three 16-byte records per pixel x + y * width (row 0 = bottom)
struct TemporalHistory {
    float4 *color;               // integrated colour rgb, history length N (a float >= 1)
    float4 *key;                 // the first hit's normal xyz, prim (int bits; -1 on a miss)
    float4 *moments;             // m1, m2, variance, sum of the valid taps' weights
};

// The previous call's camera as a pinhole: what the host keeps between calls
struct PrevCamera {
    float pos[3], forward[3], right[3], up[3];
    float focus, plane_w, plane_h;
};

struct ReprojectArgs {
    const float4 *frame;         // the framebuffer, float4[width * height]
    const void *guides;          // drt_guide[width * height] of this call's camera, frame 1
    TemporalHistory prev, cur;   // read / written; prev is not read when has_prev == 0
    uint32_t width, height;
    int32_t has_prev;
    float cam_pos[3], fwd_focus[3], horizontal[3], vertical[3];     // this call's camera (FrameParams' constants)
    PrevCamera pc;
    float max_history, alpha_min, normal_cos_min;
};
// Stage (b): reprojection, accumulation and the temporal variance (temporal_reproject_kernel), then the spatial variance of the
// pixels whose history is shorter than 4 (temporal_variance_kernel) -- two launches on `stream`.
hipError_t launch_temporal_reproject(const ReprojectArgs &args, int num_cus, hipStream_t stream);
// The second of those launches alone, for a caller that has written args.cur with a reprojection of its own (kernel_motion.hip)
hipError_t launch_temporal_variance(const ReprojectArgs &args, hipStream_t stream);

// One variance-guided a-trous pass, step 2^pass.  in = (rgb, variance) per pixel; when `var_src` is given the variance comes
// from its .z instead (pass 0 reads the history's colour and moments records as they are).  out = (rgb, variance'), or
// (rgb, 1) when `last`.
struct AtrousVarPass {
    const float4 *in;
    const float4 *var_src;
    float4 *out;
    const void *guides;
    uint32_t width, height, step;
    int32_t last;
    float sigma_luma, k_normal, k_albedo;
};
hipError_t launch_atrous_var(const AtrousVarPass &pass, FilterKernel which, hipStream_t stream);

// out = (in.rgb, 1): the result of zero passes
hipError_t launch_temporal_copy(const float4 *in, float4 *out, uint32_t n, hipStream_t stream);

}  // namespace drt
