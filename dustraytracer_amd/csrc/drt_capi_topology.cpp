// drt_capi_topology.cpp -- the mesh-topology entry points of include/drt.h (kernel_topology.hip): drt_renderer_shell_labels,
// drt_renderer_boundary_loops, drt_renderer_shell_terms and drt_renderer_topology_steps.  The argument checks are
// drt_renderer_chain_sections' in its order; what depends on the adjacency alone is made once per scene upload and kept beside d_adj.
#include "renderer_state.hpp"

#include "topology.hpp"

#include <initializer_list>

using namespace drt;

namespace {

// The checks every entry point shares once its own pointers are known to be non-null and aligned: no pending batch, the renderer's
// device, device memory (null entries are skipped), the scene's upload, the order with the query in flight
int topo_open(drt_renderer *r, const drt_scene *scene, std::initializer_list<const void *> device_ptrs, void *hip_stream, hipStream_t *s) {
    if (r->pending) return fail(DRT_ERR_INVALID, "an asynchronous render batch is pending: drt_renderer_wait first");
    HIP_TRY(hipSetDevice(r->device));
    (void)hipGetLastError();                   // (see render_batch_impl: only this call's own errors count)
    for (const void *p : device_ptrs)
        if (p && !on_renderer_device(r, p)) return fail(DRT_ERR_INVALID, "the arrays must be device memory on the renderer's device");
    if (int rc = upload_scene(r, scene)) return rc;
    *s = hip_stream ? (hipStream_t)hip_stream : r->stream;
    return query_order(r, *s);
}

// scratch: grown only once the query in flight is over
int topo_scratch(drt_renderer *r, size_t words) {
    if (words <= r->topo_work.count) return DRT_OK;
    if (r->query_recorded) HIP_TRY(hipEventSynchronize(r->ev_query));
    HIP_TRY(r->topo_work.alloc(words));
    return DRT_OK;
}

// What depends on the adjacency alone, for a scene with triangles: the table on the device (scene_adjacency, as drt_renderer_chain_sections makes it),
// the labels, the counts and the boundary list.  Waits for `s` while it labels: the host looks at the step's mode between groups of
// steps.  A device refit keeps all of it; free_scene drops it.
int ensure_topology(drt_renderer *r, const drt_scene *scene, hipStream_t s) {
    if (int rc = scene_adjacency(r, scene, s)) return rc;
    if (r->topo_built) return DRT_OK;
    const uint32_t n = r->view.n_tris;
    if (n > 0x7fffffffu / 3u) return fail(DRT_ERR_INVALID, "fewer than 2^31 half-edges expected");
    HIP_TRY(r->topo_labels.alloc(n));
    HIP_TRY(r->topo_counts.alloc(3));
    const uint32_t n_blocks = topo_scan_blocks(3u * n);
    if (int rc = topo_scratch(r, std::max(topo_label_words(n), (size_t)n_blocks * 3))) return rc;
    TopoLabelArgs la;
    la.adj = r->d_adj.ptr; la.n_tris = n; la.label = r->topo_labels.ptr;
    topo_label_carve(la, r->topo_work.ptr);
    HIP_TRY(launch_topo_label_init(la, s));
    const uint32_t cap = topo_max_steps(n);
    uint32_t launched = 0, last = kTopoHook;
    while (launched < cap && last != kTopoDone) {
        const uint32_t count = std::min<uint32_t>(kTopoStepGroup, cap - launched);
        HIP_TRY(launch_topo_label_steps(la, launched, count, s));
        launched += count;
        HIP_TRY(hipMemcpyAsync(&last, la.mode + launched - 1, sizeof last, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (last != kTopoDone) return fail(DRT_ERR_DEVICE, "the shell labelling did not settle within its bound on steps");
    std::vector<uint32_t> modes(launched);
    HIP_TRY(hipMemcpyAsync(modes.data(), la.mode, launched * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    // the parents are spent: the block sums of the counts take their place
    TopoCountArgs ca;
    ca.adj = r->d_adj.ptr; ca.label = r->topo_labels.ptr; ca.n_tris = n;
    ca.counts = r->topo_counts.ptr; ca.block_sums = r->topo_work.ptr; ca.boundary = nullptr;
    HIP_TRY(launch_topo_counts(ca, s));
    HIP_TRY(hipMemcpyAsync(r->topo_counts_host, ca.counts, sizeof r->topo_counts_host, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    r->topo_steps[0] = launched;
    r->topo_steps[1] = (uint32_t)std::count_if(modes.begin(), modes.end(), [](uint32_t m) { return m != kTopoDone; });
    r->topo_steps[2] = (uint32_t)std::count(modes.begin(), modes.end(), (uint32_t)kTopoHook);
    const uint32_t n_boundary = r->topo_counts_host[1];
    HIP_TRY(r->topo_boundary.alloc(n_boundary));
    if (n_boundary) {
        ca.boundary = r->topo_boundary.ptr;
        HIP_TRY(launch_topo_compact(ca, n_boundary, s));
    }
    r->topo_built = true;
    return DRT_OK;
}

}  // namespace

extern "C" {

int drt_renderer_shell_labels(drt_renderer *r, const drt_scene *scene, int32_t *labels, uint32_t *counts, void *hip_stream) {
    if (!r || !scene) return fail(DRT_ERR_INVALID, "null argument");
    if (!labels) return fail(DRT_ERR_INVALID, "null label pointer");
    if (((uintptr_t)labels & 3u) != 0 || ((uintptr_t)counts & 3u) != 0) return fail(DRT_ERR_INVALID, "labels and counts must be 4-byte aligned");
    hipStream_t s;
    if (int rc = topo_open(r, scene, { labels, counts }, hip_stream, &s)) return rc;
    const uint32_t n = r->view.n_tris;
    if (n == 0) {
        if (counts) HIP_TRY(hipMemsetAsync(counts, 0, 3 * sizeof(uint32_t), s));
        return query_recorded(r, s);
    }
    if (int rc = ensure_topology(r, scene, s)) return rc;
    HIP_TRY(hipMemcpyAsync(labels, r->topo_labels.ptr, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (counts) HIP_TRY(hipMemcpyAsync(counts, r->topo_counts.ptr, 3 * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    return query_recorded(r, s);
}

int drt_renderer_boundary_loops(drt_renderer *r, const drt_scene *scene, drt_loop_slot *slots, uint32_t capacity, uint32_t *counts, void *hip_stream) {
    if (!r || !scene) return fail(DRT_ERR_INVALID, "null argument");
    if (!counts) return fail(DRT_ERR_INVALID, "null count pointer");
    if ((slots == nullptr) != (capacity == 0)) return fail(DRT_ERR_INVALID, "slots must be null iff capacity is 0");
    if (((uintptr_t)slots & 15u) != 0 || ((uintptr_t)counts & 3u) != 0) return fail(DRT_ERR_INVALID, "slots must be 16-byte aligned, counts 4-byte aligned");
    if (capacity > 0x7fffffffu) return fail(DRT_ERR_INVALID, "at most 2^31 - 1 slots per call");
    hipStream_t s;
    if (int rc = topo_open(r, scene, { slots, counts }, hip_stream, &s)) return rc;
    const uint32_t n = r->view.n_tris;
    if (n > 0)
        if (int rc = ensure_topology(r, scene, s)) return rc;
    const uint32_t n_rec = n > 0 ? r->topo_counts_host[1] : 0u;
    if (n_rec == 0) {
        HIP_TRY(hipMemsetAsync(counts, 0, 3 * sizeof(uint32_t), s));
        return query_recorded(r, s);
    }
    if (int rc = topo_scratch(r, topo_loop_words(n_rec))) return rc;
    TopoLoopArgs a;
    a.adj = r->d_adj.ptr; a.boundary = r->topo_boundary.ptr;
    a.n_tris = n; a.n_rec = n_rec;
    a.slots = slots; a.capacity = capacity; a.counts = counts;
    topo_loop_carve(a, r->topo_work.ptr);
    HIP_TRY(launch_topo_loops(a, s));
    return query_recorded(r, s);
}

int drt_renderer_shell_terms(drt_renderer *r, const drt_scene *scene, double *terms, void *hip_stream) {
    if (!r || !scene) return fail(DRT_ERR_INVALID, "null argument");
    if (!terms) return fail(DRT_ERR_INVALID, "null term pointer");
    if (((uintptr_t)terms & 15u) != 0) return fail(DRT_ERR_INVALID, "terms must be 16-byte aligned");
    hipStream_t s;
    if (int rc = topo_open(r, scene, { terms }, hip_stream, &s)) return rc;
    if (r->view.n_tris == 0) return query_recorded(r, s);
    HIP_TRY(launch_topo_terms(r->view.tri_hot, r->view.n_tris, terms, s));
    return query_recorded(r, s);
}

int drt_renderer_edge_adjacency(drt_renderer *r, const drt_scene *scene, int32_t *adj, void *hip_stream) {
    if (!r || !scene) return fail(DRT_ERR_INVALID, "null argument");
    if (!adj) return fail(DRT_ERR_INVALID, "null adjacency pointer");
    if (((uintptr_t)adj & 3u) != 0) return fail(DRT_ERR_INVALID, "adj must be 4-byte aligned");
    hipStream_t s;
    if (int rc = topo_open(r, scene, { adj }, hip_stream, &s)) return rc;
    const uint32_t n = r->view.n_tris;
    if (n == 0) return query_recorded(r, s);
    if (int rc = ensure_topology(r, scene, s)) return rc;
    HIP_TRY(hipMemcpyAsync(adj, r->d_adj.ptr, (size_t)n * 3 * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return query_recorded(r, s);
}

int drt_renderer_topology_steps(const drt_renderer *r, uint32_t *out) {
    if (!r || !out) return fail(DRT_ERR_INVALID, "null argument");
    std::memcpy(out, r->topo_steps, sizeof r->topo_steps);
    return DRT_OK;
}

}  // extern "C"
