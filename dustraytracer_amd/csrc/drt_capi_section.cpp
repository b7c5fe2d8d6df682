// drt_capi_section.cpp -- the plane-section entry point of include/drt.h (drt_renderer_plane_sections, kernel_section.hip): the box
// query's argument checks in its order, the scene upload, the wave-per-plane kernel's worklist scratch and the launch.
#include "renderer_state.hpp"

#include "section.hpp"

using namespace drt;

extern "C" {

// drt_renderer_overlap_boxes' checks in its order, word for word (out for prims, 16-byte aligned as the planes are: the kernel
// writes a record as two 16-byte words).  The claim heads are the ray queries'; the worklists are this query's own scratch.
int drt_renderer_plane_sections(drt_renderer *r, const drt_scene *scene, const drt_plane *planes, const uint32_t *offsets, drt_section *out,
                                uint32_t out_capacity, uint32_t *counts, uint32_t n, int32_t mode, void *hip_stream) {
    if (!r || !scene) return fail(DRT_ERR_INVALID, "null argument");
    if (mode != DRT_SECTION_LIST && mode != DRT_SECTION_ANY)
        return fail(DRT_ERR_INVALID, "mode " + std::to_string(mode) + ": 0 (list) or 1 (any) expected");
    if (n == 0) return DRT_OK;
    const bool any = mode == DRT_SECTION_ANY;
    if (!planes || (!any && !offsets)) return fail(DRT_ERR_INVALID, "null plane or offset pointer");
    if (any) {
        if (out || out_capacity != 0) return fail(DRT_ERR_INVALID, "mode any writes no list: out must be null and out_capacity 0");
        if (!counts) return fail(DRT_ERR_INVALID, "mode any: counts is null: nothing to write");
        offsets = nullptr;                     // (not read)
    } else {
        if (!out && !counts) return fail(DRT_ERR_INVALID, "out and counts are both null: nothing to write");
        if ((out == nullptr) != (out_capacity == 0)) return fail(DRT_ERR_INVALID, "out must be null if and only if out_capacity is 0");
    }
    if (((uintptr_t)planes & 15u) != 0 || ((uintptr_t)out & 15u) != 0 || ((uintptr_t)offsets & 3u) != 0 || ((uintptr_t)counts & 3u) != 0)
        return fail(DRT_ERR_INVALID, "planes and out must be 16-byte aligned, offsets and counts 4-byte aligned");
    if (n > 0x7fffffffu) return fail(DRT_ERR_INVALID, "at most 2^31 - 1 planes per call");
    if (r->pending) return fail(DRT_ERR_INVALID, "an asynchronous render batch is pending: drt_renderer_wait first");
    HIP_TRY(hipSetDevice(r->device));
    (void)hipGetLastError();                   // (see render_batch_impl: only this call's own errors count)
    if (!on_renderer_device(r, planes) || (offsets && !on_renderer_device(r, offsets)) || (out && !on_renderer_device(r, out)) ||
        (counts && !on_renderer_device(r, counts)))
        return fail(DRT_ERR_INVALID, "planes, offsets, out and counts must be device memory on the renderer's device");
    if (int rc = upload_scene(r, scene)) return rc;
    if (!r->leaves_ascending)
        return fail(DRT_ERR_UNSUPPORTED, "plane sections need a tree whose leaves, child 1 first, hold ascending triangle ranges (the "
                                         "builder's trees do); this scene's do not, and its lists would not be sorted");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : r->stream;
    if (int rc = query_order(r, s)) return rc;
    // scratch: the claim heads, zeroed on the stream, and two worklists per wave, grown only once the query in flight is over
    SectionArgs a;
    a.waves = section_waves(n, r->num_cus, r->view.n_leaves, r->section_waves);
    a.list_words = std::max<uint32_t>(r->view.n_leaves, 1u);
    const size_t words = (size_t)a.waves * 2 * a.list_words;
    if (!r->rq_heads.ptr) HIP_TRY(r->rq_heads.alloc(kRqHeadWords));
    if (words > r->section_work.count) {
        if (r->query_recorded) HIP_TRY(hipEventSynchronize(r->ev_query));
        HIP_TRY(r->section_work.alloc(words));
    }
    HIP_TRY(hipMemsetAsync(r->rq_heads.ptr, 0, r->rq_heads.bytes(), s));
    a.planes = planes; a.offsets = offsets; a.out = out; a.counts = counts;
    a.out_capacity = out_capacity; a.n = n;
    a.heads = r->rq_heads.ptr;
    a.work = r->section_work.ptr;
    HIP_TRY(launch_section(r->view, any, a, s));
    return query_recorded(r, s);
}

}  // extern "C"
