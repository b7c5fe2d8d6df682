// drt_capi_winding.cpp -- the generalised-winding-number entry points of include/drt.h (drt_renderer_winding_numbers / _winding_inside /
// _winding_signed_distance, kernel_winding.hip): every argument check before any device work (the handles, beta, n == 0, the pointers,
// the alignment, n < 2^31, a pending batch), then device memory, the scene upload, the queries' stream ordering and the occlusion
// query's HBM stack, the node moments if an upload or a refit has made them stale, and the launch.
#include "renderer_state.hpp"

#include <cmath>

#include "winding.hpp"

using namespace drt;

namespace {

int bad_beta(float beta) { return fail(DRT_ERR_INVALID, "beta " + std::to_string(beta) + ": a number >= 0 (or +inf) expected"); }

// The moments of the uploaded tree, on stream s: made by the first call after an upload or a refit, kept until the next one.
int winding_moments(drt_renderer *r, const drt_scene *scene, hipStream_t s) {
    if (r->wn_valid) return DRT_OK;
    if (int rc = refit_metadata(r, scene)) return rc;
    const size_t n_nodes = (size_t)r->view.n_inner + r->view.n_leaves;
    if (r->wn_moments.count != n_nodes) {
        HIP_TRY(alloc_group(n_nodes, r->wn_moments, r->wn_sums));
        HIP_TRY(hipMemsetAsync(r->wn_moments.ptr, 0, r->wn_moments.bytes(), s));       // (a node the root does not reach reads zeros)
    }
    WindingMomentArgs m;
    m.leaves = r->rf_leaves.ptr; m.n_leaves = (uint32_t)r->rf_leaves.count;
    m.levels = r->rf_levels.ptr;
    m.moments = r->wn_moments.ptr; m.sums = r->wn_sums.ptr;
    HIP_TRY(launch_winding_moments(r->view, m, r->rf_heights, s));
    r->wn_valid = true;
    return DRT_OK;
}

// out: what `kind` says, aligned to out_align bytes
int winding_impl(drt_renderer *r, const drt_scene *scene, const drt_point *points, void *out, size_t out_align, uint32_t n, float beta,
                 float threshold, void *hip_stream, WindingOut kind) {
    if (!r || !scene) return fail(DRT_ERR_INVALID, "null argument");
    if (!(beta >= 0.0f)) return bad_beta(beta);
    if (n == 0) return DRT_OK;
    if (!points || !out) return fail(DRT_ERR_INVALID, "null point or result pointer");
    if (((uintptr_t)points & 15u) != 0 || ((uintptr_t)out & (out_align - 1)) != 0)
        return fail(DRT_ERR_INVALID, "points must be 16-byte aligned, results " + std::to_string(out_align) + "-byte aligned");
    hipStream_t s;              // (query_open's upload refuses a tree deeper than 64 levels, as the traversing queries do)
    if (int rc = query_open(r, scene, n, {points, out}, "points", "points and results", hip_stream, true, &s)) return rc;
    if (int rc = winding_moments(r, scene, s)) return rc;
    WindingArgs a;
    a.points = points; a.out = out; a.frame = query_frame(r, n);
    a.beta2 = beta * beta;
    a.threshold = threshold;
    a.moments = r->wn_moments.ptr;
    HIP_TRY(launch_winding(r->view, kind, a, r->num_cus, s));
    return query_recorded(r, s);
}

}  // namespace

extern "C" {

int drt_renderer_winding_numbers(drt_renderer *r, const drt_scene *scene, const drt_point *points, uint32_t n, float beta, float *out,
                                 void *hip_stream) {
    return winding_impl(r, scene, points, out, 4, n, beta, 0.5f, hip_stream, WindingOut::number);
}

int drt_renderer_winding_inside(drt_renderer *r, const drt_scene *scene, const drt_point *points, uint32_t n, float beta, float threshold,
                                uint8_t *out, void *hip_stream) {
    return winding_impl(r, scene, points, out, 1, n, beta, threshold, hip_stream, WindingOut::inside);
}

// The nearest kernel writes the records, then the winding kernel replaces their `side` words: two launches on one stream.
int drt_renderer_winding_signed_distance(drt_renderer *r, const drt_scene *scene, const drt_point *points, uint32_t n, float beta,
                                         float threshold, drt_nearest *out, void *hip_stream) {
    if (!r || !scene) return fail(DRT_ERR_INVALID, "null argument");
    if (!(beta >= 0.0f)) return bad_beta(beta);
    if (int rc = drt_renderer_nearest(r, scene, points, out, n, hip_stream)) return rc;
    return winding_impl(r, scene, points, out, 16, n, beta, threshold, hip_stream, WindingOut::side);
}

// The node moments of the renderer's copy of `scene` as the winding calls use them, made now if they are stale: n_inner + n_leaves
// records of 32 bytes, the interior nodes at their record index (the host scene's interior nodes in node order), then the leaves in
// node order.  out == NULL: only *count is written.
int drt_debug_winding_moments(drt_renderer *r, const drt_scene *scene, float *out, size_t out_floats, uint32_t *count) {
    if (!r || !scene || !count) return fail(DRT_ERR_INVALID, "null argument");
    if (r->pending) return fail(DRT_ERR_INVALID, "an asynchronous render batch is pending: drt_renderer_wait first");
    HIP_TRY(hipSetDevice(r->device));
    (void)hipGetLastError();
    if (int rc = upload_scene(r, scene)) return rc;
    const size_t n_nodes = (size_t)r->view.n_inner + r->view.n_leaves;
    *count = (uint32_t)n_nodes;
    if (!out) return DRT_OK;
    if (out_floats < 8 * n_nodes) return fail(DRT_ERR_INVALID, "destination too small");
    if (int rc = query_order(r, r->stream)) return rc;
    if (int rc = winding_moments(r, scene, r->stream)) return rc;
    if (int rc = query_recorded(r, r->stream)) return rc;
    HIP_TRY(hipStreamSynchronize(r->stream));
    if (n_nodes) HIP_TRY(hipMemcpy(out, r->wn_moments.ptr, n_nodes * sizeof(WindingMoment), hipMemcpyDeviceToHost));
    return DRT_OK;
}

}  // extern "C"
