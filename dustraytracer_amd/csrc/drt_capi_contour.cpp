// drt_capi_contour.cpp -- the section-contour entry points of include/drt.h: drt_scene_edge_adjacency (the host table) and
// drt_renderer_chain_sections (kernel_contour.hip): the plane-section query's argument checks in its order, the scene upload, the
// device copy of the adjacency beside it, the scratch and the launches.  And the intersection-curve entry points, which are the same
// two things for the records of drt_renderer_intersect_triangles: drt_tri_edge_adjacency (the host table of a query mesh) and
// drt_renderer_chain_intersections (kernel_curve.hip).
#include "renderer_state.hpp"

#include "contour.hpp"
#include "edge_adjacency.hpp"

using namespace drt;

extern "C" {

int drt_scene_edge_adjacency(const drt_scene *scene, int32_t *out, uint32_t capacity) {
    if (!scene) return fail(DRT_ERR_INVALID, "null scene");
    const size_t words = 3 * scene->host.triangles.size();
    if (capacity < words) return fail(DRT_ERR_INVALID, "destination too small: 3 values per triangle");
    if (!out && words) return fail(DRT_ERR_INVALID, "null destination");
    try {
        const std::vector<int32_t> adj = scene->host.edge_adjacency();
        if (words) std::memcpy(out, adj.data(), words * sizeof(int32_t));
        return DRT_OK;
    } catch (const std::invalid_argument &e) { return fail(DRT_ERR_INVALID, e.what());
    } catch (const std::exception &e) { return fail(DRT_ERR_INVALID, e.what()); }
}

int drt_tri_edge_adjacency(const drt_tri *tris, uint32_t n, int32_t *out, uint32_t capacity) {
    const size_t words = 3 * (size_t)n;
    if (capacity < words) return fail(DRT_ERR_INVALID, "destination too small: 3 values per triangle");
    if (words && (!tris || !out)) return fail(DRT_ERR_INVALID, "null triangles or destination");
    try {
        const std::vector<int32_t> adj = edge_adjacency_of(tris, sizeof(drt_tri), 3 * sizeof(float), n);
        if (words) std::memcpy(out, adj.data(), words * sizeof(int32_t));
        return DRT_OK;
    } catch (const std::exception &e) { return fail(DRT_ERR_INVALID, e.what()); }
}

namespace {

// drt_renderer_plane_sections' checks in its order (segs for planes, splits for offsets, slots for out, chains for counts; there is no
// mode; query_adj, where there is one, goes with splits).  The adjacency is made (scene_adjacency) with the first call after a scene upload and
// dropped with that upload.  curves: chains holds three words, not two per range, and kernel_curve.hip links.
int chain_impl(drt_renderer *r, const drt_scene *scene, const void *segs, const uint32_t *splits, const int32_t *query_adj, bool curves,
               drt_chain_slot *slots, uint32_t *chains, uint32_t n, uint32_t total, void *hip_stream) {
    if (!r || !scene) return fail(DRT_ERR_INVALID, "null argument");
    if (n == 0 || total == 0) return DRT_OK;
    if (!segs || !splits || !slots || (curves && !query_adj))
        return fail(DRT_ERR_INVALID, curves ? "null segment, split, query adjacency or slot pointer" : "null segment, split or slot pointer");
    if (((uintptr_t)segs & 15u) != 0 || ((uintptr_t)slots & 15u) != 0 || ((uintptr_t)splits & 3u) != 0 || ((uintptr_t)chains & 3u) != 0 ||
        ((uintptr_t)query_adj & 3u) != 0)
        return fail(DRT_ERR_INVALID, curves ? "segs and slots must be 16-byte aligned, splits, query_adj and counts 4-byte aligned"
                                            : "segs and slots must be 16-byte aligned, splits and chains 4-byte aligned");
    if (n > 0x7fffffffu) return fail(DRT_ERR_INVALID, curves ? "at most 2^31 - 1 queries per call" : "at most 2^31 - 1 planes per call");
    if (total > 0x7fffffffu) return fail(DRT_ERR_INVALID, "at most 2^31 - 1 records per call");
    if (r->pending) return fail(DRT_ERR_INVALID, "an asynchronous render batch is pending: drt_renderer_wait first");
    HIP_TRY(hipSetDevice(r->device));
    (void)hipGetLastError();                   // (see render_batch_impl: only this call's own errors count)
    if (!on_renderer_device(r, segs) || !on_renderer_device(r, splits) || !on_renderer_device(r, slots) || (chains && !on_renderer_device(r, chains)) ||
        (curves && !on_renderer_device(r, query_adj)))
        return fail(DRT_ERR_INVALID, curves ? "segs, splits, query_adj, slots and counts must be device memory on the renderer's device"
                                            : "segs, splits, slots and chains must be device memory on the renderer's device");
    if (int rc = upload_scene(r, scene)) return rc;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : r->stream;
    if (int rc = query_order(r, s)) return rc;
    if (int rc = scene_adjacency(r, scene, s)) return rc;      // the host scene's table: a device refit keeps the order and what is shared
    // scratch: grown only once the query in flight is over
    const size_t words = contour_scratch_words(total);
    if (words > r->contour_work.count) {
        if (r->query_recorded) HIP_TRY(hipEventSynchronize(r->ev_query));
        HIP_TRY(r->contour_work.alloc(words));
    }
    ContourArgs a;
    a.segs = segs; a.splits = splits; a.slots = slots; a.chains = chains;
    a.adj = r->d_adj.ptr;
    a.query_adj = query_adj;
    a.n = n; a.total = total; a.n_tris = r->view.n_tris;
    contour_carve(a, r->contour_work.ptr);
    HIP_TRY(curves ? launch_curves(a, s) : launch_contour(a, s));
    return query_recorded(r, s);
}

}  // namespace

int drt_renderer_chain_sections(drt_renderer *r, const drt_scene *scene, const drt_section *segs, const uint32_t *splits, drt_chain_slot *slots,
                                uint32_t *chains, uint32_t n, uint32_t total, void *hip_stream) {
    return chain_impl(r, scene, segs, splits, nullptr, false, slots, chains, n, total, hip_stream);
}

int drt_renderer_chain_intersections(drt_renderer *r, const drt_scene *scene, const drt_isect *segs, const uint32_t *splits,
                                     const int32_t *query_adj, drt_chain_slot *slots, uint32_t *counts, uint32_t n, uint32_t total,
                                     void *hip_stream) {
    return chain_impl(r, scene, segs, splits, query_adj, true, slots, counts, n, total, hip_stream);
}

}  // extern "C"
