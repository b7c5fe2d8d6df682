// drt_capi_intersect.cpp -- the intersection-segment entry point of include/drt.h (drt_renderer_intersect_triangles,
// kernel_intersect.hip): plane sections' argument checks in its order without a mode, the scene upload, the triangle overlap entry's
// stream ordering and scratch, and the launch.
#include "renderer_state.hpp"

#include "intersect.hpp"

using namespace drt;

extern "C" {

// drt_renderer_plane_sections' checks in mode LIST, in its order (tris for planes; out 16-byte aligned: the kernel writes a record as
// two 16-byte words).  The occlusion query's HBM stack (ref entries).  The opening is written out, not query_open: the check of
// leaves_ascending stands between the upload and the scratch.
int drt_renderer_intersect_triangles(drt_renderer *r, const drt_scene *scene, const drt_tri *tris, const uint32_t *offsets, drt_isect *out,
                                     uint32_t out_capacity, uint32_t *counts, uint32_t n, void *hip_stream) {
    if (!r || !scene) return fail(DRT_ERR_INVALID, "null argument");
    if (n == 0) return DRT_OK;
    if (!tris || !offsets) return fail(DRT_ERR_INVALID, "null triangle or offset pointer");
    if (!out && !counts) return fail(DRT_ERR_INVALID, "out and counts are both null: nothing to write");
    if ((out == nullptr) != (out_capacity == 0)) return fail(DRT_ERR_INVALID, "out must be null if and only if out_capacity is 0");
    if (((uintptr_t)tris & 15u) != 0 || ((uintptr_t)out & 15u) != 0 || ((uintptr_t)offsets & 3u) != 0 || ((uintptr_t)counts & 3u) != 0)
        return fail(DRT_ERR_INVALID, "tris and out must be 16-byte aligned, offsets and counts 4-byte aligned");
    if (n > 0x7fffffffu) return fail(DRT_ERR_INVALID, "at most 2^31 - 1 triangles per call");
    if (r->pending) return fail(DRT_ERR_INVALID, "an asynchronous render batch is pending: drt_renderer_wait first");
    HIP_TRY(hipSetDevice(r->device));
    (void)hipGetLastError();                   // (see render_batch_impl: only this call's own errors count)
    if (!on_renderer_device(r, tris) || !on_renderer_device(r, offsets) || (out && !on_renderer_device(r, out)) ||
        (counts && !on_renderer_device(r, counts)))
        return fail(DRT_ERR_INVALID, "tris, offsets, out and counts must be device memory on the renderer's device");
    if (int rc = upload_scene(r, scene)) return rc;
    if (!r->leaves_ascending)
        return fail(DRT_ERR_UNSUPPORTED, "intersection segments need a tree whose leaves, child 1 first, hold ascending triangle ranges (the "
                                         "builder's trees do); this scene's do not, and its lists would not be sorted");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : r->stream;
    if (int rc = query_order(r, s)) return rc;
    if (int rc = traversal_scratch(r, s, true, true)) return rc;
    IntersectArgs a;
    a.tris = tris; a.offsets = offsets; a.out = out; a.counts = counts;
    a.out_capacity = out_capacity; a.frame = query_frame(r, n);
    HIP_TRY(launch_intersect(r->view, a, r->num_cus, s));
    return query_recorded(r, s);
}

}  // extern "C"
