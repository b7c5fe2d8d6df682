// drt_capi_adaptive.cpp -- the C ABI of include/drt.h, third part: adaptive sampling (drt_renderer_render_adaptive and its
// read-back, kernel_adaptive.hip).  The samples themselves are traced by the radiance kernel, as drt_renderer_radiance runs it.
#include "renderer_state.hpp"

#include <cmath>

using namespace drt;

namespace {

// What both entry points check of the parameters (nullptr = fine); *budget = the samples of the call (0 in = 4 per pixel)
const char *adaptive_arguments(const drt_adaptive_params *p, uint64_t pixels, uint32_t *budget) {
    if (p->max_spp < 1 || p->min_spp > p->max_spp) return "min_spp <= max_spp and max_spp >= 1 expected";
    if (!std::isfinite(p->target_error) || !(p->target_error >= 0.f)) return "target_error must be finite and >= 0";
    if (!std::isfinite(p->luma_floor) || !(p->luma_floor > 0.f)) return "luma_floor must be finite and > 0";
    if (p->budget >= (1u << 31)) return "budget too large (less than 2^31 samples per call)";
    if (pixels == 0) return "no frame size";
    if (pixels > (1ull << 31)) return "too many pixels (at most 2^31)";
    const uint64_t b = p->budget ? p->budget : 4 * pixels;
    if (b >= (1ull << 31)) return "budget too large (less than 2^31 samples per call)";
    if (b < (uint64_t)p->min_spp * pixels) return "budget smaller than min_spp samples for every pixel";
    *budget = (uint32_t)b;
    return nullptr;
}

AdaptivePlanArgs plan_args(const drt_adaptive_params *p, uint32_t pixels, uint32_t budget, bool thresholded) {
    AdaptivePlanArgs a;
    std::memset(&a, 0, sizeof a);
    a.pixels = pixels;
    a.min_spp = p->min_spp; a.max_spp = p->max_spp;
    a.extra = budget - p->min_spp * pixels;
    a.thresholded = thresholded;
    a.target_error = p->target_error; a.luma_floor = p->luma_floor;
    return a;
}

int alloc_adaptive_state(drt_renderer *r, size_t px) {
    if (r->ad_state[0].ptr) return DRT_OK;
    hipError_t e = alloc_group(px, r->ad_q, r->ad_counts, r->ad_offsets);
    if (e == hipSuccess) e = r->ad_block_sums.alloc((px + kScanBlock - 1) / kScanBlock);
    if (e == hipSuccess) e = r->ad_totals.alloc(1);
    if (e == hipSuccess) e = r->ad_state[1].alloc_zeroed(px);
    if (e == hipSuccess) e = r->ad_state[0].alloc_zeroed(px);       // (the last one: its pointer says that the state is whole)
    if (e != hipSuccess) r->free_adaptive();
    HIP_TRY(e);
    return DRT_OK;
}

}  // namespace

extern "C" {

void drt_default_adaptive_params(drt_adaptive_params *out) {
    if (!out) return;
    out->budget = 0;
    out->min_spp = 1; out->max_spp = 64;
    out->target_error = 0.f; out->luma_floor = 0.01f;
}

int drt_renderer_render_adaptive(drt_renderer *r, const drt_camera *cam, const drt_scene *scene, const drt_adaptive_params *p,
                                 drt_adaptive_info *info) {
    if (info) std::memset(info, 0, sizeof *info);
    if (!r || !cam || !scene || !p) return fail(DRT_ERR_INVALID, "null argument");
    if (int rc = stage_open(r, "adaptive sampling needs")) return rc;
    if (r->settings.render_mode == 1) return fail(DRT_ERR_UNSUPPORTED, "debug views are the frame loop's: adaptive sampling needs render_mode 0");
    const size_t px = (size_t)r->width * r->height;
    uint32_t budget = 0;
    if (const char *why = adaptive_arguments(p, px, &budget)) return fail(DRT_ERR_INVALID, why);
    if (int rc = upload_scene(r, scene)) return rc;          // (nothing is allocated for a scene the tracing refuses)
    if (int rc = alloc_adaptive_state(r, px)) return rc;
    hipStream_t s = r->stream;

    // stages 1-3: the plan
    AdaptivePlanArgs pa = plan_args(p, (uint32_t)px, budget, p->target_error > 0.f);
    pa.state0 = r->ad_state[0].ptr; pa.state1 = r->ad_state[1].ptr;
    pa.q = r->ad_q.ptr; pa.counts = r->ad_counts.ptr; pa.offsets = r->ad_offsets.ptr; pa.block_sums = r->ad_block_sums.ptr;
    pa.totals = r->ad_totals.ptr;
    if (int rc = stage_begin(r)) return rc;
    HIP_TRY(hipMemsetAsync(r->ad_totals.ptr, 0, sizeof(AdaptiveTotals), s));
    HIP_TRY(launch_adaptive_plan(pa, s));
    AdaptiveTotals tot;
    HIP_TRY(hipMemcpyAsync(&tot, r->ad_totals.ptr, sizeof tot, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (tot.total > budget) return fail(DRT_ERR_DEVICE, "adaptive plan: the counts sum to more than the budget");

    // the pixel ranges of stages 4-6: 48 bytes per sample (ray + result) within the sample budget, at least one pixel each
    const size_t per_range = std::max<size_t>(1, r->sample_budget / (sizeof(drt_path_ray) + sizeof(float4)));
    std::vector<uint32_t> bounds{ 0u }, stops{ 0u };     // the pixel where a range starts and the samples in front of it; then px, total
    size_t largest = tot.total;
    if (tot.total > per_range) {
        std::vector<uint32_t> off(px);
        HIP_TRY(hipMemcpy(off.data(), r->ad_offsets.ptr, px * sizeof(uint32_t), hipMemcpyDeviceToHost));
        largest = 0;
        for (uint32_t first = 0; first < px;) {
            // the last end whose samples in front of it, off[end] (off[px] = total), are within per_range of off[first]; past first
            const uint64_t limit = (uint64_t)off[first] + per_range;
            const uint32_t e = (uint32_t)(std::upper_bound(off.begin() + first, off.end(), limit, [](uint64_t v, uint32_t o) { return v < o; }) - off.begin());
            uint32_t end = (e == px && tot.total <= limit) ? (uint32_t)px : e - 1;
            end = std::max(end, first + 1);               // (a pixel whose own samples exceed the budget is a range of its own)
            const uint32_t stop = end < px ? off[end] : tot.total;
            largest = std::max<size_t>(largest, stop - off[first]);
            bounds.push_back(end); stops.push_back(stop);
            first = end;
        }
    } else {
        bounds.push_back((uint32_t)px); stops.push_back(tot.total);
    }
    if (largest > r->ad_rays.count || !r->ad_rays.ptr) {
        HIP_TRY(alloc_group(largest, r->ad_rays, r->ad_samples));
    }

    AdaptiveRangeArgs ra;
    std::memset(&ra, 0, sizeof ra);
    ra.state0 = r->ad_state[0].ptr; ra.state1 = r->ad_state[1].ptr;
    ra.q = r->ad_q.ptr; ra.counts = r->ad_counts.ptr; ra.offsets = r->ad_offsets.ptr;
    ra.rays = r->ad_rays.ptr; ra.samples = r->ad_samples.ptr;
    ra.rgba = reinterpret_cast<float4 *>(r->cur_rgba());
    ra.width = r->width; ra.height = r->height;
    ra.cam = camera_const(cam, (float)r->width, (float)r->height);
    FrameParams fp;
    std::memset(&fp, 0, sizeof fp);
    fill_frame_params(r, nullptr, fp);
    for (size_t k = 0; k + 1 < bounds.size(); k++) {
        ra.pixel_first = bounds[k]; ra.pixel_end = bounds[k + 1];
        ra.ray_base = stops[k]; ra.n_rays = stops[k + 1] - stops[k];
        if (ra.n_rays > r->ad_rays.count) return fail(DRT_ERR_DEVICE, "adaptive plan: a range outgrew its buffers");
        if (ra.n_rays) {
            // stages 4-5: the ray list, then the radiance kernel with the ray queries' heads and stack, in their order
            if (int rc = query_order(r, s)) return rc;
            if (int rc = traversal_scratch(r, s, false, true)) return rc;
            HIP_TRY(launch_adaptive_rays(ra, s));
            RadianceArgs a;
            a.rays = r->ad_rays.ptr; a.out = r->ad_samples.ptr; a.frame = query_frame(r, ra.n_rays);
            a.accumulate = 0;
            HIP_TRY(launch_radiance(r->view, fp, r->scene_has_alpha, a, r->num_cus, s));
            if (int rc = query_recorded(r, s)) return rc;
        }
        HIP_TRY(launch_adaptive_fold(ra, s));             // stage 6 (also for a range without samples: the last q and count, the image)
    }
    float ms = 0.f;
    if (int rc = stage_end(r, &ms)) return rc;
    if (info) { info->samples = tot.total; info->active_pixels = tot.active; info->max_count = tot.max_count; info->ms = ms; }
    return DRT_OK;
}

int drt_renderer_adaptive_reset(drt_renderer *r) {
    if (!r) return fail(DRT_ERR_INVALID, "null argument");
    if (r->pending) return fail(DRT_ERR_INVALID, "an asynchronous render batch is pending: drt_renderer_wait first");
    if (r->ad_state[0].ptr) {
        HIP_TRY(hipSetDevice(r->device));
        HIP_TRY(hipStreamSynchronize(r->stream));
    }
    r->free_adaptive();
    return DRT_OK;
}

void *drt_renderer_device_adaptive(drt_renderer *r, int32_t which) {
    return r && (which == 0 || which == 1) ? (void *)r->ad_state[which].ptr : nullptr;
}

int drt_renderer_read_adaptive(drt_renderer *r, int32_t which, void *dst, size_t dst_bytes) {
    if (!r || !dst) return fail(DRT_ERR_INVALID, "null argument");
    if (which < 0 || which > 1) return fail(DRT_ERR_INVALID, "which must be 0 (sum, n) or 1 (m1, m2, last q, last count)");
    if (!r->ad_state[0].ptr) return fail(DRT_ERR_INVALID, "no adaptive state yet: drt_renderer_render_adaptive first");
    const size_t need = r->ad_state[which].bytes();
    if (dst_bytes < need) return fail(DRT_ERR_INVALID, "destination too small");
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipStreamSynchronize(r->stream));
    HIP_TRY(hipMemcpy(dst, r->ad_state[which].ptr, need, hipMemcpyDeviceToHost));
    return DRT_OK;
}

int drt_debug_adaptive_plan(int32_t device, const uint32_t *q, uint32_t pixels, const drt_adaptive_params *p, int32_t thresholded,
                            uint32_t *counts, uint32_t *offsets, uint64_t *Q_out) {
    if (!q || !p || !counts || !offsets) return fail(DRT_ERR_INVALID, "null argument");
    uint32_t budget = 0;
    if (const char *why = adaptive_arguments(p, pixels, &budget)) return fail(DRT_ERR_INVALID, why);
    HIP_TRY(hipSetDevice(device));
    DeviceArray<uint32_t> d_q, d_counts, d_offsets, d_sums;
    DeviceArray<AdaptiveTotals> d_tot;
    HIP_TRY(alloc_group(pixels, d_q, d_counts, d_offsets));
    HIP_TRY(d_sums.alloc((pixels + kScanBlock - 1) / kScanBlock));
    HIP_TRY(d_tot.alloc_zeroed(1));
    HIP_TRY(hipMemcpy(d_q.ptr, q, (size_t)pixels * sizeof(uint32_t), hipMemcpyHostToDevice));
    AdaptivePlanArgs a = plan_args(p, pixels, budget, thresholded != 0);
    a.q = d_q.ptr; a.counts = d_counts.ptr; a.offsets = d_offsets.ptr; a.block_sums = d_sums.ptr; a.totals = d_tot.ptr;
    HIP_TRY(launch_adaptive_plan(a, nullptr));
    AdaptiveTotals tot;
    HIP_TRY(hipMemcpy(&tot, d_tot.ptr, sizeof tot, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(counts, d_counts.ptr, (size_t)pixels * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(offsets, d_offsets.ptr, (size_t)pixels * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (Q_out) *Q_out = tot.Q;
    return DRT_OK;
}

int drt_debug_adaptive_weights(int32_t device, const float *state0, const float *state1, uint32_t pixels, const drt_adaptive_params *p,
                               uint32_t *q, uint64_t *Q_out, uint32_t *active_out) {
    if (!state0 || !state1 || !p || !q) return fail(DRT_ERR_INVALID, "null argument");
    uint32_t budget = 0;
    if (const char *why = adaptive_arguments(p, pixels, &budget)) return fail(DRT_ERR_INVALID, why);
    HIP_TRY(hipSetDevice(device));
    DeviceArray<float4> d_s0, d_s1;
    DeviceArray<uint32_t> d_q, d_counts, d_offsets, d_sums;
    DeviceArray<AdaptiveTotals> d_tot;
    HIP_TRY(alloc_group(pixels, d_s0, d_s1));
    HIP_TRY(alloc_group(pixels, d_q, d_counts, d_offsets));
    HIP_TRY(d_sums.alloc((pixels + kScanBlock - 1) / kScanBlock));
    HIP_TRY(d_tot.alloc_zeroed(1));
    HIP_TRY(hipMemcpy(d_s0.ptr, state0, (size_t)pixels * sizeof(float4), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_s1.ptr, state1, (size_t)pixels * sizeof(float4), hipMemcpyHostToDevice));
    AdaptivePlanArgs a = plan_args(p, pixels, budget, p->target_error > 0.f);      // (as drt_renderer_render_adaptive sets them)
    a.state0 = d_s0.ptr; a.state1 = d_s1.ptr;
    a.q = d_q.ptr; a.counts = d_counts.ptr; a.offsets = d_offsets.ptr; a.block_sums = d_sums.ptr; a.totals = d_tot.ptr;
    HIP_TRY(launch_adaptive_plan(a, nullptr));
    AdaptiveTotals tot;
    HIP_TRY(hipMemcpy(&tot, d_tot.ptr, sizeof tot, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(q, d_q.ptr, (size_t)pixels * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (Q_out) *Q_out = tot.Q;
    if (active_out) *active_out = tot.active;
    return DRT_OK;
}

}  // extern "C"
