// drt_capi_ambient.cpp -- the ambient-occlusion entry point of include/drt.h (drt_renderer_ambient_occlusion, kernel_ambient.hip):
// every argument check before any device work (the handles, the parameters, n == 0, the pointers, the alignment, n < 2^31, first + n,
// a scene without a BVH, a pending batch), then device memory, the scene upload, the occlusion query's stream ordering and HBM stack,
// the 64-bit claim heads this feature owns, the pass that writes the skipped points' records, and the launch.
#include "renderer_state.hpp"

#include "ambient.hpp"

using namespace drt;

extern "C" {

int drt_renderer_ambient_occlusion(drt_renderer *r, const drt_scene *scene, const drt_ao_point *pts, uint32_t n, const drt_ao_params *params,
                                   drt_ao_result *out, void *hip_stream) {
    if (!r || !scene || !params) return fail(DRT_ERR_INVALID, "null argument");
    if (params->samples == 0 || params->samples > kAoMaxSamples)
        return fail(DRT_ERR_INVALID, "samples " + std::to_string(params->samples) + ": 1 .. 4096 expected");
    if (params->flags != 0) return fail(DRT_ERR_INVALID, "flags " + std::to_string(params->flags) + ": 0 expected");
    if (n == 0) return DRT_OK;
    if (!pts || !out) return fail(DRT_ERR_INVALID, "null point or result pointer");
    if (((uintptr_t)pts & 15u) != 0 || ((uintptr_t)out & 15u) != 0) return fail(DRT_ERR_INVALID, "points and results must be 16-byte aligned");
    if (n > 0x7fffffffu) return fail(DRT_ERR_INVALID, "at most 2^31 - 1 points per call");
    if ((uint64_t)params->first + n > ((uint64_t)1 << 32)) return fail(DRT_ERR_INVALID, "first + n must not exceed 2^32");
    if (scene->host.nodes.empty()) return fail(DRT_ERR_INVALID, "scene has no BVH: build one first");
    if (r->pending) return fail(DRT_ERR_INVALID, "an asynchronous render batch is pending: drt_renderer_wait first");
    HIP_TRY(hipSetDevice(r->device));
    (void)hipGetLastError();                   // (see render_batch_impl: only this call's own errors count)
    if (!on_renderer_device(r, pts) || !on_renderer_device(r, out))
        return fail(DRT_ERR_INVALID, "points and results must be device memory on the renderer's device");
    if (int rc = upload_scene(r, scene)) return rc;             // (refuses a tree deeper than 64 levels, as the traversing queries do)
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : r->stream;
    if (int rc = query_order(r, s)) return rc;
    if (int rc = traversal_scratch(r, s, true, false)) return rc;
    if (!r->ao_heads.ptr) HIP_TRY(r->ao_heads.alloc((size_t)kRqShards * kAoHeadStride));
    HIP_TRY(hipMemsetAsync(r->ao_heads.ptr, 0, r->ao_heads.bytes(), s));
    AmbientArgs a;
    a.pts = reinterpret_cast<const AoPoint *>(pts); a.out = reinterpret_cast<AoResult *>(out); a.n = n;
    a.samples = params->samples; a.seed_hash = ao_pcg(params->seed); a.first = params->first;
    a.stack_levels = query_stack_levels(r);
    a.heads = r->ao_heads.ptr;
    a.stack_hbm = r->rq_stack.ptr;
    HIP_TRY(launch_ambient_init(a, s));
    HIP_TRY(launch_ambient(r->view, a, r->num_cus, r->ao_stats_on ? r->ao_stats.ptr : nullptr, s));
    return query_recorded(r, s);
}

// The counting build of the tracing kernel (DESIGN 5.30's lane utilisation).  enable != 0: the calls that follow run it and add to two
// counters, zeroed here; enable == 0: they run the plain build again.  out != NULL: the counters so far, after the queries in flight:
// {trips of the waves' traversal loops, lanes that took a step in them}; utilisation = out[1] / (64 out[0]).
int drt_debug_ambient_stats(drt_renderer *r, int32_t enable, uint64_t out[2]) {
    if (!r) return fail(DRT_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(r->device));
    if (r->query_recorded) HIP_TRY(hipEventSynchronize(r->ev_query));
    if (out) {
        out[0] = out[1] = 0;
        if (r->ao_stats.ptr) HIP_TRY(hipMemcpy(out, r->ao_stats.ptr, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    if (enable) HIP_TRY(r->ao_stats.alloc_zeroed(2));
    r->ao_stats_on = enable != 0;
    return DRT_OK;
}

}  // extern "C"
