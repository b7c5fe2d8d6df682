// drt_capi_subdivide.cpp -- the subdivision entry point of include/drt.h (drt_renderer_subdivide; kernel_subdivide.hip): every argument
// check before any device work, in drt_renderer_simplify's order and style, then the renderer's scratch, grown on demand, and the
// launches: the adjacency of the faces by index with the edges numbered (adjacency.hpp), with Loop the coordinate maximum (weld.hpp),
// then the children, the edges and the finish (subdivide.hpp).  The call reads no scene and no tree; it shares scratch with the
// welding calls, so it orders itself as the queries do (query_order / query_recorded: one event).
#include "renderer_state.hpp"

#include <algorithm>

#include "adjacency.hpp"
#include "subdivide.hpp"

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

// [p, p + bytes) meets [q, q + qbytes)
bool overlaps(const void *p, uint64_t bytes, const void *q, uint64_t qbytes) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return p && q && bytes && qbytes && a < b + qbytes && b < a + bytes;
}

}  // namespace

extern "C" {

int drt_renderer_subdivide(drt_renderer *r, const float *vertices, uint32_t n_vertices, const int32_t *faces, uint32_t n_tris, int32_t scheme,
                           float *out_vertices, int32_t *parents, uint32_t vertex_capacity, int32_t *out_faces, uint32_t *vertex_count,
                           void *hip_stream) {
    if (!r || !vertex_count) return fail(DRT_ERR_INVALID, "null argument");
    if (scheme != DRT_SUBDIVIDE_MIDPOINT && scheme != DRT_SUBDIVIDE_LOOP)
        return fail(DRT_ERR_INVALID, "scheme " + std::to_string(scheme) + ": DRT_SUBDIVIDE_MIDPOINT (0) or DRT_SUBDIVIDE_LOOP (1) expected");
    if ((uint64_t)n_tris * 3 > 0x7fffffffu) return fail(DRT_ERR_INVALID, std::to_string(n_tris) + " triangles: 3 N < 2^31 expected");
    if ((uint64_t)n_vertices + (uint64_t)n_tris * 3 > 0x7fffffffu)
        return fail(DRT_ERR_INVALID, std::to_string(n_vertices) + " vertices, " + std::to_string(n_tris) + " triangles: V + 3 N < 2^31 expected");
    if ((uint64_t)n_tris * 12 > 0x7fffffffu) return fail(DRT_ERR_INVALID, std::to_string(n_tris) + " triangles: 12 N < 2^31 expected");
    // (n_tris == 0 stores V, copies the stored vertices and is otherwise a no-op: the checks below apply to what it touches)
    if (n_vertices && !vertices) return fail(DRT_ERR_INVALID, "null vertices");
    if (n_tris && (!faces || !out_faces)) return fail(DRT_ERR_INVALID, "null faces or out_faces");
    if ((out_vertices == nullptr) != (vertex_capacity == 0)) return fail(DRT_ERR_INVALID, "out_vertices must be null if and only if vertex_capacity is 0");
    if (parents && !out_vertices) return fail(DRT_ERR_INVALID, "parents without out_vertices: a capacity is needed");
    if (misaligned4(vertices) || misaligned4(faces) || misaligned4(out_vertices) || misaligned4(parents) || misaligned4(out_faces) ||
        misaligned4(vertex_count))
        return fail(DRT_ERR_INVALID, "vertices, faces, out_vertices, parents, out_faces and vertex_count must be 4-byte aligned");
    {
        const uint64_t vb = 12ull * n_vertices, fb = 12ull * n_tris;
        const struct { const void *p; uint64_t bytes; } outs[] = {{out_vertices, 12ull * vertex_capacity}, {parents, 8ull * vertex_capacity},
                                                                  {out_faces, 48ull * n_tris}, {vertex_count, 4}};
        for (const auto &o : outs)
            if (overlaps(o.p, o.bytes, vertices, vb) || overlaps(o.p, o.bytes, faces, fb))
                return fail(DRT_ERR_INVALID, "an output may not alias vertices or faces");
    }
    if (r->pending) return fail(DRT_ERR_INVALID, "an asynchronous render batch is pending: drt_renderer_wait first");
    HIP_TRY(hipSetDevice(r->device));
    (void)hipGetLastError();                   // (see render_batch_impl: only this call's own errors count)
    if (!on_renderer_device(r, vertex_count) || (n_vertices && !on_renderer_device(r, vertices)) ||
        (n_tris && (!on_renderer_device(r, faces) || !on_renderer_device(r, out_faces))) ||
        (out_vertices && !on_renderer_device(r, out_vertices)) || (parents && !on_renderer_device(r, parents)))
        return fail(DRT_ERR_INVALID, "vertices, faces, out_vertices, parents, out_faces and vertex_count must be device memory on the renderer's device");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : r->stream;
    if (int rc = query_order(r, s)) return rc;
    const bool loop = scheme == DRT_SUBDIVIDE_LOOP;
    const bool sums = loop && n_tris && n_vertices && vertex_capacity;          // the even vertices are stored first: any capacity needs them
    SubdivideArgs a;
    a.vertices = vertices; a.faces = faces; a.n_vertices = n_vertices; a.n_tris = n_tris;
    a.adj = nullptr; a.edge = nullptr; a.half_edge = nullptr; a.edge_count = nullptr;
    a.acc_int = nullptr; a.acc_cr = nullptr; a.n_int = nullptr; a.n_cr = nullptr; a.max_bits = nullptr;
    a.out_vertices = out_vertices; a.parents = parents; a.capacity = vertex_capacity; a.out_faces = out_faces; a.vertex_count = vertex_count;
    if (n_tris) {
        AdjacencyArgs adj;
        adj.first = reinterpret_cast<const unsigned char *>(faces); adj.tri_stride = 12; adj.vertex_stride = 4; adj.half_edges = 3 * n_tris;
        const uint64_t slots = weld_table_slots(adj.half_edges);
        const size_t other_words = ((size_t)adj.half_edges + 1) / 2;            // `other`: 4 bytes each in the 8-byte words of wd_acc
        // every block is grown before the first launch: wd_acc holds `other` during the adjacency and the interior sums after it
        if (int rc = grow(r, r->wd_table, slots)) return rc;
        if (int rc = grow(r, r->wd_rep, adj.half_edges)) return rc;
        if (int rc = grow(r, r->wd_blocks, weld_blocks(adj.half_edges))) return rc;
        if (int rc = grow(r, r->wd_acc, std::max(other_words, sums ? 3 * (size_t)n_vertices : (size_t)0))) return rc;
        if (int rc = grow(r, r->sd_adj, adj.half_edges)) return rc;
        if (int rc = grow(r, r->sd_edge, adj.half_edges)) return rc;
        if (int rc = grow(r, r->sd_half_edge, adj.half_edges)) return rc;
        if (int rc = grow(r, r->sd_cnt, 2 + (sums ? 2 * (size_t)n_vertices : (size_t)0))) return rc;
        if (sums) {
            if (int rc = grow(r, r->sd_acc, 3 * (size_t)n_vertices)) return rc;
            if (int rc = grow(r, r->wd_max, 2)) return rc;
        }
        adj.table = r->wd_table.ptr; adj.mask = (uint32_t)(slots - 1); adj.rep = r->wd_rep.ptr;
        adj.other = reinterpret_cast<uint32_t *>(r->wd_acc.ptr); adj.block_totals = r->wd_blocks.ptr;
        adj.adj = r->sd_adj.ptr; adj.edge = r->sd_edge.ptr; adj.half_edge = r->sd_half_edge.ptr; adj.capacity = adj.half_edges;
        adj.edge_count = r->sd_cnt.ptr;
        HIP_TRY(launch_adjacency(AdjacencyKey::index, adj, s));
        a.adj = adj.adj; a.edge = adj.edge; a.half_edge = adj.half_edge; a.edge_count = adj.edge_count;
        if (sums) {
            // behind the adjacency's last launch in stream order: `other` is dead, its words become the interior sums
            HIP_TRY(hipMemsetAsync(r->wd_acc.ptr, 0, 3 * (size_t)n_vertices * sizeof(unsigned long long), s));
            HIP_TRY(hipMemsetAsync(r->sd_acc.ptr, 0, 3 * (size_t)n_vertices * sizeof(unsigned long long), s));
            HIP_TRY(hipMemsetAsync(r->sd_cnt.ptr + 2, 0, 2 * (size_t)n_vertices * sizeof(uint32_t), s));
            HIP_TRY(hipMemsetAsync(r->wd_max.ptr, 0, 2 * sizeof(uint32_t), s));
            SmoothArgs m;                                                        // the seam reads src, n_vertices and max_bits only
            m.src = vertices; m.dst = nullptr; m.faces = faces; m.fixed = nullptr; m.n_vertices = n_vertices; m.n_tris = n_tris;
            m.acc = nullptr; m.cnt = nullptr; m.max_bits = r->wd_max.ptr; m.step = 0; m.factor = 0.0f;
            HIP_TRY(launch_smooth_maximum(m, r->num_cus, s));                    // M, the largest finite |coordinate|, into word 0
            a.acc_int = reinterpret_cast<long long *>(r->wd_acc.ptr); a.acc_cr = reinterpret_cast<long long *>(r->sd_acc.ptr);
            a.n_int = r->sd_cnt.ptr + 2; a.n_cr = r->sd_cnt.ptr + 2 + n_vertices; a.max_bits = r->wd_max.ptr;
        }
    }
    // without the sums (midpoint, or nothing stored) the kernels take the midpoint forms, which read none of them
    HIP_TRY(launch_subdivide(sums ? SubdivideScheme::loop : SubdivideScheme::midpoint, a, r->num_cus, s));
    return query_recorded(r, s);
}

}  // extern "C"
