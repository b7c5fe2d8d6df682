// adaptive.hpp -- launch seam of kernel_adaptive.hip: adaptive sampling (drt_renderer_render_adaptive, include/drt.h).  Per call:
// weights from the per-pixel state, counts from the weights, an exclusive scan of the counts, the ragged ray list of a pixel
// range, (the radiance kernel traces it: radiance.hpp), and the fold of the samples back into the state and the image.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "radiance.hpp"

namespace drt {

constexpr uint32_t kAdaptiveCap = 16777215u;      // the weight of a pixel whose variance is unknown or not finite (2^24 - 1)
constexpr int kScanThreads = 256;                 // the scan's workgroup ...
constexpr int kScanItems = 4;                     // ... and counts per lane:
constexpr uint32_t kScanBlock = kScanThreads * kScanItems;      // 1024 counts per block

// What the plan's stages leave for the host (one 24-byte read-back per call); zeroed on the stream in front of the weights
struct AdaptiveTotals {
    unsigned long long Q;        // sum of the weights
    uint32_t active;             // pixels with q > 0
    uint32_t total;              // sum of the counts: the samples of this call
    uint32_t max_count;
    uint32_t _pad;
};

struct AdaptivePlanArgs {
    const float4 *state0, *state1;       // (sum rgb, n bits), (m1, m2, -, -) per pixel; both NULL: `q` is given (drt_debug_adaptive_plan)
    uint32_t *q;                         // uint32[pixels]: the weights (written by the weights stage unless given)
    uint32_t *counts;                    // uint32[pixels]
    uint32_t *offsets;                   // uint32[pixels]: the exclusive prefix sum of counts
    uint32_t *block_sums;                // uint32[ceil(pixels / kScanBlock)]
    AdaptiveTotals *totals;
    uint32_t pixels;                     // 1 .. 2^31
    uint32_t min_spp, max_spp, extra;    // extra = budget - min_spp * pixels
    int32_t thresholded;                 // target_error > 0: a converged pixel gets 0 samples instead of min_spp
    float target_error, luma_floor;
};
// Stages 1-3 on `stream`: four launches (weights + reduction, counts + block sums, the scan of the block sums, offsets).
hipError_t launch_adaptive_plan(const AdaptivePlanArgs &args, hipStream_t stream);

struct AdaptiveRangeArgs {
    float4 *state0, *state1;             // per pixel, read and written by the fold
    const uint32_t *q, *counts, *offsets;
    void *rays;                          // drt_path_ray[n_rays] of the range, 16-B aligned
    const float4 *samples;               // float4[n_rays]: the radiance of rays[]
    float4 *rgba;                        // the framebuffer, float4[width * height]
    uint32_t width, height;
    uint32_t pixel_first, pixel_end;     // the range [first, end)
    uint32_t ray_base, n_rays;           // offsets[pixel_first], and the samples of the range
    CamConst cam;
};
// Stage 4: ray j of the range is sample k = ray_base + j - offsets[p] + 1 of the pixel p that owns it, in frame n(p) + k.
hipError_t launch_adaptive_rays(const AdaptiveRangeArgs &args, hipStream_t stream);
// Stage 6: the samples of every pixel of the range folded into its state in sample order, and its image value written.
hipError_t launch_adaptive_fold(const AdaptiveRangeArgs &args, hipStream_t stream);

}  // namespace drt
