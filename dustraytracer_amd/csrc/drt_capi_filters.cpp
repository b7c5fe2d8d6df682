// drt_capi_filters.cpp -- the C ABI of include/drt.h, second part: the guide pass and the stages that work on a finished frame
// (a-trous denoiser, temporal filter, motion vectors, upscaler) with their read-back.  The renderer itself is in drt_capi.cpp.
#include "renderer_state.hpp"

#include <cmath>

#include "motion.hpp"
#include "upscale.hpp"

using namespace drt;

// The timed span of a stage on the renderer's stream: stage_begin opens it, stage_end closes it, waits and stores the time
int drt::stage_begin(drt_renderer *r) {
    HIP_TRY(r->ev_dn_start.create());
    HIP_TRY(r->ev_dn_stop.create());
    HIP_TRY(hipEventRecord(r->ev_dn_start, r->stream));
    return DRT_OK;
}
int drt::stage_end(drt_renderer *r, float *delta_ms) {
    HIP_TRY(hipEventRecord(r->ev_dn_stop, r->stream));
    HIP_TRY(hipEventSynchronize(r->ev_dn_stop));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, r->ev_dn_start, r->ev_dn_stop));
    if (delta_ms) *delta_ms = ms;
    return DRT_OK;
}

// The stages' buffer groups, allocated by the first call after a resize.  Each is there whole or not at all: a failure releases
// the group, so the next call allocates again instead of finding the first pointer set and launching on the others.
static int alloc_filter_targets(drt_renderer *r, size_t px) {
    if (r->dn_guides.ptr) return DRT_OK;
    HIP_TRY(alloc_group(px, r->dn_guides, r->dn_buf[0], r->dn_buf[1]));
    return DRT_OK;
}
static int alloc_temporal_history(drt_renderer *r, size_t px) {
    auto &h = r->tp_hist;
    if (h[0][0].ptr) return DRT_OK;
    r->tp_cur = -1;
    HIP_TRY(alloc_group(px, h[0][0], h[0][1], h[0][2], h[1][0], h[1][1], h[1][2]));
    return DRT_OK;
}
static int alloc_upscale_targets(drt_renderer *r, size_t px, size_t out_px) {
    r->free_upscale();
    hipError_t e = r->us_guides.alloc(px + out_px);
    if (e == hipSuccess) e = r->us_out.alloc(out_px);
    if (e != hipSuccess) r->free_upscale();
    HIP_TRY(e);
    return DRT_OK;
}

static void set_camera(ReprojectArgs &a, const CamConst &cc) {
    std::memcpy(a.cam_pos, cc.cam_pos, 12); std::memcpy(a.fwd_focus, cc.fwd_focus, 12);
    std::memcpy(a.horizontal, cc.horizontal, 12); std::memcpy(a.vertical, cc.vertical, 12);
}

extern "C" {

// ------------------------------------------------------------------ guide buffers and the a-trous denoiser (kernel_denoise.hip)
// The guide pass on stream `s`, ordered with the ray queries (it shares their HBM stack); the caller has checked the arguments.
// width, height: the size of the image the guides are for, 0 = the renderer's frame (`guides` holds that many records).
static int enqueue_guides(drt_renderer *r, const drt_camera *cam, const drt_scene *scene, uint32_t frame_index, void *guides, hipStream_t s,
                          uint32_t width = 0, uint32_t height = 0) {
    if (int rc = whole_frame(r, "guides and the denoiser need")) return rc;
    if (int rc = upload_scene(r, scene)) return rc;
    if (int rc = query_order(r, s)) return rc;
    if (int rc = traversal_scratch(r, s, false, false)) return rc;
    FrameParams fp;
    std::memset(&fp, 0, sizeof fp);
    fill_frame_params(r, cam, fp, width, height);
    GuideArgs a;
    a.out = guides;
    a.frame = frame_index;
    a.stack_levels = query_stack_levels(r);
    a.stack_hbm = r->rq_stack.ptr;
    HIP_TRY(launch_guides(r->view, fp, a, r->num_cus, s));
    return query_recorded(r, s);
}

int drt_renderer_render_guides(drt_renderer *r, const drt_camera *cam, const drt_scene *scene, uint32_t frame_index,
                               drt_guide *guides, void *hip_stream) {
    if (!r || !cam || !scene || !guides) return fail(DRT_ERR_INVALID, "null argument");
    if (frame_index == 0) return fail(DRT_ERR_INVALID, "frame indices start at 1");
    if (((uintptr_t)guides & 15u) != 0) return fail(DRT_ERR_INVALID, "guides must be 16-byte aligned");
    if (int rc = stage_open(r, nullptr)) return rc;             // (enqueue_guides refuses a sharded renderer)
    if (!on_renderer_device(r, guides)) return fail(DRT_ERR_INVALID, "guides must be device memory on the renderer's device");
    return enqueue_guides(r, cam, scene, frame_index, guides, hip_stream ? (hipStream_t)hip_stream : r->stream);
}

void drt_default_denoise_params(drt_denoise_params *out) {
    if (!out) return;
    out->iterations = 5;
    out->sigma_color = 0.5f; out->sigma_normal = 0.1f; out->sigma_albedo = 0.1f;
}

int drt_renderer_denoise(drt_renderer *r, const drt_camera *cam, const drt_scene *scene, const drt_denoise_params *p, float *delta_ms) {
    if (delta_ms) *delta_ms = 0.f;
    if (!r || !cam || !scene || !p) return fail(DRT_ERR_INVALID, "null argument");
    if (p->iterations < 0 || p->iterations > 10) return fail(DRT_ERR_INVALID, "iterations must lie in [0, 10]");
    for (float sigma : { p->sigma_color, p->sigma_normal, p->sigma_albedo })
        if (!std::isfinite(sigma) || !(sigma > 0.f)) return fail(DRT_ERR_INVALID, "every sigma must be finite and > 0");
    if (int rc = stage_open(r, "the denoiser needs")) return rc;
    const size_t px = (size_t)r->width * r->height;
    if (int rc = alloc_filter_targets(r, px)) return rc;
    r->denoised = -1;
    if (int rc = stage_begin(r)) return rc;
    if (int rc = enqueue_guides(r, cam, scene, 1, r->dn_guides.ptr, r->stream)) return rc;
    const float4 *in = reinterpret_cast<const float4 *>(r->cur_rgba());
    int out = 0;
    if (p->iterations == 0) {
        HIP_TRY(hipMemcpyAsync(r->dn_buf[0].ptr, in, px * sizeof(float4), hipMemcpyDeviceToDevice, r->stream));
    } else {
        const float inv_sc2 = 1.0f / (p->sigma_color * p->sigma_color);
        for (int i = 0; i < p->iterations; i++, out ^= 1) {
            AtrousPass ps;
            ps.in = i == 0 ? in : r->dn_buf[out ^ 1].ptr;
            ps.out = r->dn_buf[out].ptr;
            ps.guides = r->dn_guides.ptr;
            ps.width = r->width; ps.height = r->height; ps.step = 1u << i;
            ps.k_color = (float)(1 << i) * inv_sc2;
            ps.k_normal = 1.0f / (p->sigma_normal * p->sigma_normal);
            ps.k_albedo = 1.0f / (p->sigma_albedo * p->sigma_albedo);
            HIP_TRY(launch_atrous(ps, r->filter_kernel, r->stream));
        }
        out ^= 1;
    }
    if (int rc = stage_end(r, delta_ms)) return rc;
    r->denoised = out;
    return DRT_OK;
}

// ------------------------------------------------------------------ temporal reprojection and the variance-guided filter (kernel_temporal.hip)
void drt_default_temporal_params(drt_temporal_params *out) {
    if (!out) return;
    out->iterations = 5;
    out->max_history = 32;
    out->alpha_min = 0.f;
    out->normal_cos_min = 0.9f;
    out->sigma_luma = 4.f; out->sigma_normal = 0.1f; out->sigma_albedo = 0.1f;
}

// The camera as the next call's reprojection sees it: Camera.cu:82's basis and image plane, without jitter and defocus
static PrevCamera pinhole_of(const drt_camera *cam, float width, float height) {
    PrevCamera pc;
    const float fov_factor = tanf((cam->vfov_rad / 2) / 2.0f);
    pc.plane_h = 2.0f * fov_factor * cam->focus_dist;
    pc.plane_w = pc.plane_h * (width / height);
    pc.focus = cam->focus_dist;
    const V3 f = normalize(V3{ cam->forward[0], cam->forward[1], cam->forward[2] });
    const V3 right = normalize(cross(f, V3{ 0, 1, 0 })), up = cross(right, f);
    auto put = [](float *dst, V3 v) { dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; };
    std::memcpy(pc.pos, cam->position, 12);
    put(pc.forward, f); put(pc.right, right); put(pc.up, up);
    return pc;
}

// The current records and the armed snapshot as the kernels of kernel_motion.hip read them (snapshot NULL = nothing armed: every
// pixel static)
static MotionGeometry motion_geometry(const drt_renderer *r) {
    MotionGeometry geo;
    geo.hot = reinterpret_cast<const float4 *>(r->d_hot.ptr);
    geo.snapshot = nullptr;
    if (r->mv_armed && r->mv_snap.count == r->d_hot.count && r->d_hot.count != 0) geo.snapshot = reinterpret_cast<const float4 *>(r->mv_snap.ptr);
    return geo;
}

int drt_renderer_temporal_denoise(drt_renderer *r, const drt_camera *cam, const drt_scene *scene, const drt_temporal_params *p, float *delta_ms) {
    if (delta_ms) *delta_ms = 0.f;
    if (!r || !cam || !scene || !p) return fail(DRT_ERR_INVALID, "null argument");
    if (p->iterations < 0 || p->iterations > 10) return fail(DRT_ERR_INVALID, "iterations must lie in [0, 10]");
    if (p->max_history < 1) return fail(DRT_ERR_INVALID, "max_history must be at least 1");
    if (!(p->alpha_min >= 0.f && p->alpha_min <= 1.f)) return fail(DRT_ERR_INVALID, "alpha_min must lie in [0, 1]");
    if (!std::isfinite(p->normal_cos_min)) return fail(DRT_ERR_INVALID, "normal_cos_min must be finite");
    for (float sigma : { p->sigma_luma, p->sigma_normal, p->sigma_albedo })
        if (!std::isfinite(sigma) || !(sigma > 0.f)) return fail(DRT_ERR_INVALID, "every sigma must be finite and > 0");
    if (int rc = stage_open(r, "the temporal filter needs")) return rc;
    const size_t px = (size_t)r->width * r->height;
    if (int rc = alloc_filter_targets(r, px)) return rc;
    if (int rc = alloc_temporal_history(r, px)) return rc;
    r->denoised = -1;
    if (int rc = stage_begin(r)) return rc;
    if (int rc = enqueue_guides(r, cam, scene, 1, r->dn_guides.ptr, r->stream)) return rc;

    const int half = r->tp_cur < 0 ? 0 : r->tp_cur ^ 1;
    const CamConst cc = camera_const(cam, (float)r->width, (float)r->height);
    ReprojectArgs a;
    std::memset(&a, 0, sizeof a);
    a.frame = reinterpret_cast<const float4 *>(r->cur_rgba());
    a.guides = r->dn_guides.ptr;
    a.cur = TemporalHistory{ r->tp_hist[half][0].ptr, r->tp_hist[half][1].ptr, r->tp_hist[half][2].ptr };
    a.prev = TemporalHistory{ r->tp_hist[half ^ 1][0].ptr, r->tp_hist[half ^ 1][1].ptr, r->tp_hist[half ^ 1][2].ptr };
    a.width = r->width; a.height = r->height;
    a.has_prev = r->tp_cur >= 0;
    set_camera(a, cc);
    if (a.has_prev) a.pc = r->tp_cam;
    a.max_history = (float)p->max_history; a.alpha_min = p->alpha_min; a.normal_cos_min = p->normal_cos_min;
    r->tp_cur = -1;                            // (a failure below leaves no history)
    if (r->mv_armed) {                         // geometry moved since the last call: P' and n' of the moved rule (kernel_motion.hip)
        HIP_TRY(launch_motion_reproject(a, motion_geometry(r), r->stream));
        r->mv_armed = false;                   // the geometry as it is now is the previous geometry of the next call
    } else {
        HIP_TRY(launch_temporal_reproject(a, r->num_cus, r->stream));
    }

    int out = 0;
    if (p->iterations == 0) {
        HIP_TRY(launch_temporal_copy(a.cur.color, r->dn_buf[0].ptr, (uint32_t)px, r->stream));
    } else {
        for (int i = 0; i < p->iterations; i++, out ^= 1) {
            AtrousVarPass ps;
            ps.in = i == 0 ? a.cur.color : r->dn_buf[out ^ 1].ptr;
            ps.var_src = i == 0 ? a.cur.moments : nullptr;
            ps.out = r->dn_buf[out].ptr;
            ps.guides = r->dn_guides.ptr;
            ps.width = r->width; ps.height = r->height; ps.step = 1u << i;
            ps.last = i == p->iterations - 1;
            ps.sigma_luma = p->sigma_luma;
            ps.k_normal = 1.0f / (p->sigma_normal * p->sigma_normal);
            ps.k_albedo = 1.0f / (p->sigma_albedo * p->sigma_albedo);
            HIP_TRY(launch_atrous_var(ps, r->filter_kernel, r->stream));
        }
        out ^= 1;
    }
    if (int rc = stage_end(r, delta_ms)) return rc;
    r->tp_cam = pinhole_of(cam, (float)r->width, (float)r->height);
    r->tp_cur = half;
    r->denoised = out;
    return DRT_OK;
}

int drt_renderer_temporal_reset(drt_renderer *r) {
    if (!r) return fail(DRT_ERR_INVALID, "null argument");
    if (r->pending) return fail(DRT_ERR_INVALID, "an asynchronous render batch is pending: drt_renderer_wait first");
    if (r->tp_hist[0][0].ptr) {
        HIP_TRY(hipSetDevice(r->device));
        HIP_TRY(hipStreamSynchronize(r->stream));
    }
    r->free_temporal();
    return DRT_OK;
}

void *drt_renderer_device_temporal(drt_renderer *r, int32_t which) {
    return r && r->tp_cur >= 0 && (which == 0 || which == 1) ? (void *)r->tp_hist[r->tp_cur][which == 0 ? 0 : 2].ptr : nullptr;
}

// ------------------------------------------------------------------ motion tracking and motion vectors (kernel_motion.hip)
int drt_renderer_track_motion(drt_renderer *r, int32_t enable) {
    if (!r) return fail(DRT_ERR_INVALID, "null argument");
    r->mv_track = enable != 0;
    if (!r->mv_track) {
        if (r->mv_snap.ptr) {
            HIP_TRY(hipSetDevice(r->device));
            HIP_TRY(hipDeviceSynchronize());     // (a motion-vector pass on a caller's stream may still read them)
        }
        r->mv_snap.release();
        r->mv_armed = false;
    }
    return DRT_OK;
}

int drt_renderer_motion_advance(drt_renderer *r) {
    if (!r) return fail(DRT_ERR_INVALID, "null argument");
    r->mv_armed = false;
    return DRT_OK;
}

int drt_renderer_motion_vectors(drt_renderer *r, const drt_camera *cam, const drt_camera *prev_cam, const drt_scene *scene, float *out,
                                void *hip_stream) {
    if (!r || !cam || !scene || !out) return fail(DRT_ERR_INVALID, "null argument");
    if (((uintptr_t)out & 15u) != 0) return fail(DRT_ERR_INVALID, "out must be 16-byte aligned");
    if (!prev_cam && r->tp_cur < 0) return fail(DRT_ERR_INVALID, "no previous camera: pass prev_cam or call drt_renderer_temporal_denoise first");
    if (int rc = stage_open(r, nullptr)) return rc;             // (a sharded renderer is refused after the pointer)
    if (!on_renderer_device(r, out)) return fail(DRT_ERR_INVALID, "out must be device memory on the renderer's device");
    if (int rc = whole_frame(r, "motion vectors need")) return rc;
    if (int rc = upload_scene(r, scene)) return rc;       // (nothing is allocated for a scene the guide pass refuses)
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : r->stream;
    if (!r->mv_guides.ptr) HIP_TRY(r->mv_guides.alloc((size_t)r->width * r->height));
    if (int rc = enqueue_guides(r, cam, scene, 1, r->mv_guides.ptr, s)) return rc;
    const CamConst cc = camera_const(cam, (float)r->width, (float)r->height);
    ReprojectArgs a;
    std::memset(&a, 0, sizeof a);
    a.guides = r->mv_guides.ptr;
    a.width = r->width; a.height = r->height;
    a.has_prev = 1;
    set_camera(a, cc);
    a.pc = prev_cam ? pinhole_of(prev_cam, (float)r->width, (float)r->height) : r->tp_cam;
    HIP_TRY(launch_motion_vectors(a, motion_geometry(r), reinterpret_cast<float4 *>(out), s));
    return query_recorded(r, s);                 // (the next guide pass, on whatever stream, overwrites mv_guides only after this one)
}

// ------------------------------------------------------------------ guide-driven upscaling (kernel_upscale.hip)
void drt_default_upscale_params(drt_upscale_params *out) {
    if (!out) return;
    out->source = 0;
    out->demodulate = 0;                         // (include/drt.h: demodulation lost against the oracle on both test scenes)
    out->sigma_normal = 0.1f; out->sigma_depth = 0.05f; out->sigma_albedo = 0.1f;
    out->albedo_floor = 0.01f;
}

// What both entry points check of the parameters and the two sizes (nullptr = fine)
static const char *upscale_arguments(const drt_upscale_params *p, uint32_t W, uint32_t H, uint32_t Wo, uint32_t Ho) {
    if (p->source < 0 || p->source > 1) return "source must be 0 (the framebuffer) or 1 (the denoised target)";
    if (p->demodulate < 0 || p->demodulate > 1) return "demodulate must be 0 or 1";
    for (float v : { p->sigma_normal, p->sigma_depth, p->sigma_albedo, p->albedo_floor })
        if (!std::isfinite(v) || !(v > 0.f)) return "every sigma and the albedo floor must be finite and > 0";
    if (W == 0 || H == 0) return "no frame size";
    if (Wo < W || Ho < H) return "the output must be at least as large as the frame in both axes";
    if ((uint64_t)Wo * Ho > (1ull << 31)) return "output too large (at most 2^31 pixels)";
    return nullptr;
}

static UpscaleArgs upscale_args(const drt_upscale_params *p, uint32_t W, uint32_t H, uint32_t Wo, uint32_t Ho) {
    UpscaleArgs a;
    std::memset(&a, 0, sizeof a);
    a.width = W; a.height = H; a.out_width = Wo; a.out_height = Ho;
    a.demodulate = p->demodulate;
    a.k_normal = 1.0f / (p->sigma_normal * p->sigma_normal);
    a.k_albedo = 1.0f / (p->sigma_albedo * p->sigma_albedo);
    a.sigma_depth = p->sigma_depth;
    a.albedo_floor = p->albedo_floor;
    return a;
}

int drt_renderer_upscale(drt_renderer *r, const drt_camera *cam, const drt_scene *scene, uint32_t out_width, uint32_t out_height,
                         const drt_upscale_params *p, float *delta_ms) {
    if (delta_ms) *delta_ms = 0.f;
    if (!r || !cam || !scene || !p) return fail(DRT_ERR_INVALID, "null argument");
    if (int rc = stage_open(r, "upscaling needs")) return rc;
    if (const char *why = upscale_arguments(p, r->width, r->height, out_width, out_height)) return fail(DRT_ERR_INVALID, why);
    if (p->source == 1 && r->denoised < 0) return fail(DRT_ERR_INVALID, "source 1 is the denoised target: drt_renderer_denoise or drt_renderer_temporal_denoise first");
    const size_t px = (size_t)r->width * r->height, out_px = (size_t)out_width * out_height;
    if (r->us_width != out_width || r->us_height != out_height) {
        if (int rc = alloc_upscale_targets(r, px, out_px)) return rc;
    }
    r->us_width = r->us_height = 0;              // (a failure below leaves no result)
    drt_guide *lo = r->us_guides.ptr, *hi = lo + px;
    int rc = stage_begin(r);
    if (rc == DRT_OK) rc = enqueue_guides(r, cam, scene, 1, lo, r->stream);
    if (rc == DRT_OK) rc = enqueue_guides(r, cam, scene, 1, hi, r->stream, out_width, out_height);
    if (rc != DRT_OK) { r->free_upscale(); return rc; }
    UpscaleArgs a = upscale_args(p, r->width, r->height, out_width, out_height);
    a.color = p->source == 1 ? r->dn_buf[r->denoised].ptr : reinterpret_cast<const float4 *>(r->cur_rgba());
    a.guides_lo = lo; a.guides_hi = hi;
    a.out = r->us_out.ptr;
    HIP_TRY(launch_upscale(a, r->stream));
    if ((rc = stage_end(r, delta_ms)) != DRT_OK) return rc;
    r->us_width = out_width; r->us_height = out_height;
    return DRT_OK;
}

void *drt_renderer_device_upscaled(drt_renderer *r) { return r && r->us_width ? (void *)r->us_out.ptr : nullptr; }

int drt_renderer_read_upscaled_rgba32f(drt_renderer *r, float *dst, size_t dst_floats) {
    if (!r || !dst) return fail(DRT_ERR_INVALID, "null argument");
    if (r->us_width == 0) return fail(DRT_ERR_INVALID, "no upscaled image yet: drt_renderer_upscale first");
    const size_t need = (size_t)r->us_width * r->us_height * 4;
    if (dst_floats < need) return fail(DRT_ERR_INVALID, "destination too small");
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipStreamSynchronize(r->stream));
    HIP_TRY(hipMemcpy(dst, r->us_out.ptr, need * sizeof(float), hipMemcpyDeviceToHost));
    return DRT_OK;
}

int drt_debug_upscale(int32_t device, const float *colour, const drt_guide *guides_lo, const drt_guide *guides_hi, uint32_t width, uint32_t height,
                      uint32_t out_width, uint32_t out_height, const drt_upscale_params *p, float *out) {
    if (!colour || !guides_lo || !guides_hi || !p || !out) return fail(DRT_ERR_INVALID, "null argument");
    if (const char *why = upscale_arguments(p, width, height, out_width, out_height)) return fail(DRT_ERR_INVALID, why);
    HIP_TRY(hipSetDevice(device));
    const size_t px = (size_t)width * height, out_px = (size_t)out_width * out_height;
    const size_t off_lo = px * sizeof(float4), off_hi = off_lo + px * sizeof(drt_guide), off_out = off_hi + out_px * sizeof(drt_guide);
    DeviceArray<char> buf;                       // colour, guides_lo, guides_hi, out: every part a multiple of 16 bytes
    HIP_TRY(buf.alloc(off_out + out_px * sizeof(float4)));
    char *const d = buf.ptr;
    HIP_TRY(hipMemcpy(d, colour, off_lo, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d + off_lo, guides_lo, px * sizeof(drt_guide), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d + off_hi, guides_hi, out_px * sizeof(drt_guide), hipMemcpyHostToDevice));
    UpscaleArgs a = upscale_args(p, width, height, out_width, out_height);
    a.color = reinterpret_cast<const float4 *>(d);
    a.guides_lo = d + off_lo; a.guides_hi = d + off_hi;
    a.out = reinterpret_cast<float4 *>(d + off_out);
    HIP_TRY(launch_upscale(a, nullptr));
    HIP_TRY(hipMemcpy(out, d + off_out, out_px * sizeof(float4), hipMemcpyDeviceToHost));
    return DRT_OK;
}

void *drt_renderer_device_denoised(drt_renderer *r) { return r && r->denoised >= 0 ? (void *)r->dn_buf[r->denoised].ptr : nullptr; }

int drt_renderer_read_denoised_rgba32f(drt_renderer *r, float *dst, size_t dst_floats) {
    if (r && r->denoised < 0) return fail(DRT_ERR_INVALID, "no denoised image yet: drt_renderer_denoise first");
    return read_back(r, r ? (const float *)r->dn_buf[r->denoised].ptr : nullptr, 4, dst, dst_floats);
}

int drt_renderer_read_temporal(drt_renderer *r, int32_t which, float *dst, size_t dst_floats) {
    if (!r || !dst) return fail(DRT_ERR_INVALID, "null argument");
    if (which < 0 || which > 1) return fail(DRT_ERR_INVALID, "which must be 0 (colour, N) or 1 (moments, variance, weight)");
    if (r->tp_cur < 0) return fail(DRT_ERR_INVALID, "no temporal history yet: drt_renderer_temporal_denoise first");
    return read_back(r, (const float *)r->tp_hist[r->tp_cur][which == 0 ? 0 : 2].ptr, 4, dst, dst_floats);
}

}  // extern "C"
