// drt_capi_adjacency.cpp -- the device edge-adjacency entry points of include/drt.h (drt_renderer_tri_adjacency,
// drt_renderer_face_adjacency, drt_renderer_boundary_vertices, drt_renderer_adjacency_route; kernel_adjacency.hip): every argument
// check before any device work, in drt_renderer_weld's order and style, then the renderer's scratch, grown on demand, and the
// launches.  And scene_adjacency, which makes the uploaded scene's table for the contour, curve and topology calls with the same
// kernel.  The calls share scratch with the welding calls, so they order themselves as the queries do (query_order / query_recorded).
#include "renderer_state.hpp"

#include "adjacency.hpp"

using namespace drt;

namespace {

template <class T>
int grow(drt_renderer *r, drt_renderer::DeviceArray<T> &a, size_t n) {
    if (a.ptr && a.count >= n) return DRT_OK;
    if (r->query_recorded) HIP_TRY(hipEventSynchronize(r->ev_query));          // nothing in flight reads the old block
    HIP_TRY(a.alloc(n));                                                         // out of memory: DRT_ERR_DEVICE, and the next call tries again
    return DRT_OK;
}

bool misaligned4(const void *p) { return ((uintptr_t)p & 3u) != 0; }

// the scratch of adjacency.hpp for a.half_edges > 0 (a.edge says whether the scan's block totals are needed), then the launches
int run_adjacency(drt_renderer *r, AdjacencyKey key, AdjacencyArgs &a, hipStream_t s) {
    const uint64_t slots = weld_table_slots(a.half_edges);
    a.mask = (uint32_t)(slots - 1);
    if (int rc = grow(r, r->wd_table, slots)) return rc;
    if (int rc = grow(r, r->wd_rep, a.half_edges)) return rc;
    if (int rc = grow(r, r->wd_acc, ((size_t)a.half_edges + 1) / 2)) return rc;     // `other`: 4 bytes each in the 8-byte words
    if (a.edge) if (int rc = grow(r, r->wd_blocks, weld_blocks(a.half_edges))) return rc;
    a.table = r->wd_table.ptr; a.rep = r->wd_rep.ptr; a.other = reinterpret_cast<uint32_t *>(r->wd_acc.ptr);
    a.block_totals = a.edge ? r->wd_blocks.ptr : nullptr;
    HIP_TRY(launch_adjacency(key, a, s));
    return DRT_OK;
}

// the two adjacency calls behind their own checks of `first`: the outputs' checks, the device, the order, the launches
int adjacency_impl(drt_renderer *r, AdjacencyKey key, const void *first, uint32_t tri_stride, uint32_t vertex_stride, const char *first_name,
                   uint32_t n, int32_t *adj, int32_t *edge, int32_t *half_edge, uint32_t capacity, uint32_t *edge_count, void *hip_stream) {
    if ((uint64_t)n * 3 > 0x7fffffffu) return fail(DRT_ERR_INVALID, std::to_string(n) + " triangles: 3 N < 2^31 expected");
    if (n == 0) return DRT_OK;                                                   // nothing is touched
    if (!first || !adj) return fail(DRT_ERR_INVALID, std::string("null ") + first_name + " or adj");
    if ((edge == nullptr) != (edge_count == nullptr)) return fail(DRT_ERR_INVALID, "edge and edge_count must be null together");
    if (!edge && (half_edge || capacity)) return fail(DRT_ERR_INVALID, "half_edge and capacity without edge");
    if ((half_edge == nullptr) != (capacity == 0)) return fail(DRT_ERR_INVALID, "half_edge must be null if and only if capacity is 0");
    if (misaligned4(first) || misaligned4(adj) || misaligned4(edge) || misaligned4(half_edge) || misaligned4(edge_count))
        return fail(DRT_ERR_INVALID, std::string(first_name) + ", adj, edge, half_edge and edge_count must be 4-byte aligned");
    if (r->pending) return fail(DRT_ERR_INVALID, "an asynchronous render batch is pending: drt_renderer_wait first");
    HIP_TRY(hipSetDevice(r->device));
    (void)hipGetLastError();                   // (see render_batch_impl: only this call's own errors count)
    if (!on_renderer_device(r, first) || !on_renderer_device(r, adj) || (edge && !on_renderer_device(r, edge)) ||
        (half_edge && !on_renderer_device(r, half_edge)) || (edge_count && !on_renderer_device(r, edge_count)))
        return fail(DRT_ERR_INVALID, std::string(first_name) + ", adj, edge, half_edge and edge_count must be device memory on the renderer's device");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : r->stream;
    if (int rc = query_order(r, s)) return rc;
    AdjacencyArgs a;
    a.first = static_cast<const unsigned char *>(first); a.tri_stride = tri_stride; a.vertex_stride = vertex_stride; a.half_edges = 3 * n;
    a.adj = adj; a.edge = edge; a.half_edge = half_edge; a.capacity = capacity; a.edge_count = edge_count;
    if (int rc = run_adjacency(r, key, a, s)) return rc;
    return query_recorded(r, s);
}

}  // namespace

// The uploaded scene's table into d_adj, once per upload (free_scene drops it): on the device from the HOST scene's positions in tree
// order -- the device's TriHot holds v0, e1, e2, and a device refit changes them -- or, with DRT_ADJACENCY=host, by the host's sort.
// The same bytes either way (drt_scene_edge_adjacency is the reference).  `s` is the stream the calling entry point resolved and has
// ordered with the query in flight.
int drt::scene_adjacency(drt_renderer *r, const drt_scene *scene, hipStream_t s) {
    if (r->adj_built) return DRT_OK;
    const std::vector<drt_triangle> &tris = scene->host.triangles;
    const size_t n = tris.size();
    if (scene->host.nodes.empty()) return fail(DRT_ERR_INVALID, "scene has no BVH: the adjacency is in tree order, build one first");
    if (n > 0x7fffffffu / 3u) return fail(DRT_ERR_INVALID, "fewer than 2^31 half-edges expected");
    if (r->adjacency_host || n == 0) {
        std::vector<int32_t> adj;
        try { adj = scene->host.edge_adjacency(); } catch (const std::exception &e) { return fail(DRT_ERR_INVALID, e.what()); }
        HIP_TRY(r->d_adj.upload(adj));
        r->adjacency_route = kAdjRouteHost;
    } else {
        std::vector<float> packed(9 * n);                                        // 36 bytes per triangle, copied bit for bit
        for (size_t t = 0; t < n; t++)
            for (int k = 0; k < 3; k++) std::memcpy(&packed[9 * t + 3 * k], tris[t].vertex[k].position, 12);
        drt_renderer::DeviceArray<float> positions;                              // the temporary: freed when this returns
        HIP_TRY(positions.alloc(packed.size()));
        HIP_TRY(r->d_adj.alloc(3 * n));
        HIP_TRY(hipMemcpyAsync(positions.ptr, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice, s));
        AdjacencyArgs a;
        a.first = reinterpret_cast<const unsigned char *>(positions.ptr); a.tri_stride = 36; a.vertex_stride = 12; a.half_edges = (uint32_t)(3 * n);
        a.adj = r->d_adj.ptr; a.edge = nullptr; a.half_edge = nullptr; a.capacity = 0; a.edge_count = nullptr;
        if (int rc = run_adjacency(r, AdjacencyKey::position, a, s)) return rc;
        HIP_TRY(hipStreamSynchronize(s));                                        // the launches are over: `packed` and `positions` may go
        r->adjacency_route = kAdjRouteDevice;
    }
    r->adj_built = true;
    return DRT_OK;
}

extern "C" {

int drt_renderer_tri_adjacency(drt_renderer *r, const void *tris, uint32_t n, uint32_t stride, int32_t *adj, int32_t *edge, int32_t *half_edge,
                               uint32_t capacity, uint32_t *edge_count, void *hip_stream) {
    if (!r) return fail(DRT_ERR_INVALID, "null argument");
    if (stride != 36 && stride != 48) return fail(DRT_ERR_INVALID, "stride " + std::to_string(stride) + ": 36 ([N][3][3] floats) or 48 (drt_tri) expected");
    return adjacency_impl(r, AdjacencyKey::position, tris, stride, 12, "tris", n, adj, edge, half_edge, capacity, edge_count, hip_stream);
}

int drt_renderer_face_adjacency(drt_renderer *r, const int32_t *faces, uint32_t n, int32_t *adj, int32_t *edge, int32_t *half_edge,
                                uint32_t capacity, uint32_t *edge_count, void *hip_stream) {
    if (!r) return fail(DRT_ERR_INVALID, "null argument");
    return adjacency_impl(r, AdjacencyKey::index, faces, 12, 4, "faces", n, adj, edge, half_edge, capacity, edge_count, hip_stream);
}

int drt_renderer_boundary_vertices(drt_renderer *r, const int32_t *faces, const int32_t *adj, uint32_t n_tris, uint32_t n_vertices,
                                   uint32_t flags, uint8_t *out, void *hip_stream) {
    if (!r) return fail(DRT_ERR_INVALID, "null argument");
    if (flags & ~1u) return fail(DRT_ERR_INVALID, "flags " + std::to_string(flags) + ": 0 or DRT_BOUNDARY_BAD_EDGES (1) expected");
    if ((uint64_t)n_tris * 3 > 0x7fffffffu) return fail(DRT_ERR_INVALID, std::to_string(n_tris) + " triangles: 3 N < 2^31 expected");
    if (n_vertices > 0x7fffffffu) return fail(DRT_ERR_INVALID, std::to_string(n_vertices) + " vertices: fewer than 2^31 expected");
    if (n_vertices == 0) return DRT_OK;
    if (!out) return fail(DRT_ERR_INVALID, "null out");
    if (n_tris && (!faces || !adj)) return fail(DRT_ERR_INVALID, "null faces or adj");
    if (misaligned4(faces) || misaligned4(adj)) return fail(DRT_ERR_INVALID, "faces and adj must be 4-byte aligned");
    if (r->pending) return fail(DRT_ERR_INVALID, "an asynchronous render batch is pending: drt_renderer_wait first");
    HIP_TRY(hipSetDevice(r->device));
    (void)hipGetLastError();
    if ((n_tris && (!on_renderer_device(r, faces) || !on_renderer_device(r, adj))) || !on_renderer_device(r, out))
        return fail(DRT_ERR_INVALID, "faces, adj and out must be device memory on the renderer's device");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : r->stream;
    if (int rc = query_order(r, s)) return rc;
    HIP_TRY(hipMemsetAsync(out, 0, n_vertices, s));
    BoundaryArgs a;
    a.faces = faces; a.adj = adj; a.n_tris = n_tris; a.n_vertices = n_vertices; a.flags = flags; a.out = out;
    HIP_TRY(launch_boundary_vertices(a, s));
    return query_recorded(r, s);
}

int drt_renderer_adjacency_route(const drt_renderer *r) { return r ? r->adjacency_route : 0; }

}  // extern "C"
