// drt_capi_simplify.cpp -- the simplification entry point of include/drt.h (drt_renderer_simplify; kernel_simplify.hip): every argument
// check before any device work, in drt_renderer_weld's order and style, then the renderer's scratch, grown on demand, and the
// launches.  The call reads no scene and no tree; it shares scratch with the welding calls, so it orders itself as the queries do
// (query_order / query_recorded: one event).
#include "renderer_state.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "simplify.hpp"

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

int drt_renderer_simplify(drt_renderer *r, const float *vertices, uint32_t n_vertices, const int32_t *faces, uint32_t n_tris,
                          const drt_grid *grid, int32_t placement, int32_t *cluster, float *out_vertices, int32_t *first,
                          uint32_t vertex_capacity, int32_t *out_faces, int32_t *source, uint32_t tri_capacity, uint32_t *counts,
                          void *hip_stream) {
    if (!r || !grid || !counts) return fail(DRT_ERR_INVALID, "null argument");
    if (n_vertices && (!vertices || !cluster)) return fail(DRT_ERR_INVALID, "null vertices or cluster");
    if (n_tris && !faces) return fail(DRT_ERR_INVALID, "null faces");
    if ((out_vertices == nullptr) != (vertex_capacity == 0) || (first == nullptr) != (vertex_capacity == 0))
        return fail(DRT_ERR_INVALID, "out_vertices and first must be null if and only if vertex_capacity is 0");
    if ((out_faces == nullptr) != (tri_capacity == 0) || (source == nullptr) != (tri_capacity == 0))
        return fail(DRT_ERR_INVALID, "out_faces and source must be null if and only if tri_capacity is 0");
    if (placement != DRT_SIMPLIFY_MEAN && placement != DRT_SIMPLIFY_QUADRIC)
        return fail(DRT_ERR_INVALID, "placement " + std::to_string(placement) + ": DRT_SIMPLIFY_MEAN (0) or DRT_SIMPLIFY_QUADRIC (1) expected");
    uint64_t cells = 1;
    for (int k = 0; k < 3; k++) {
        if (!std::isfinite(grid->lo[k])) return fail(DRT_ERR_INVALID, "grid lo[" + std::to_string(k) + "]: a finite value expected");
        if (!std::isfinite(grid->cell[k]) || !(grid->cell[k] > 0.0f))
            return fail(DRT_ERR_INVALID, "grid cell[" + std::to_string(k) + "] = " + std::to_string(grid->cell[k]) + ": a finite value greater than 0 expected");
    }
    for (int k = 0; k < 3; k++) {
        if (grid->dims[k] < 1u) return fail(DRT_ERR_INVALID, "grid dims[" + std::to_string(k) + "] = 0: at least 1 cell per axis expected");
        if (grid->dims[k] > 0x7fffffffu) return fail(DRT_ERR_INVALID, "grid dims: fewer than 2^31 cells expected");
        cells *= grid->dims[k];
        if (cells > 0x7fffffffu) return fail(DRT_ERR_INVALID, "grid dims: fewer than 2^31 cells expected");
    }
    if (n_vertices > 0x7fffffffu) return fail(DRT_ERR_INVALID, std::to_string(n_vertices) + " vertices: fewer than 2^31 expected");
    if ((uint64_t)n_tris * 3 > 0x7fffffffu) return fail(DRT_ERR_INVALID, std::to_string(n_tris) + " triangles: 3 N < 2^31 expected");
    const bool empty = n_vertices == 0;                                          // a no-op that stores C = M = 0: only counts is looked at
    if (misaligned4(counts) || (!empty && (misaligned4(vertices) || misaligned4(faces) || misaligned4(cluster) || misaligned4(out_vertices) ||
                                           misaligned4(first) || misaligned4(out_faces) || misaligned4(source))))
        return fail(DRT_ERR_INVALID, "vertices, faces, cluster, out_vertices, first, out_faces, source and counts must be 4-byte aligned");
    if (!empty) {
        const uint64_t vb = 12ull * n_vertices, fb = 12ull * n_tris;
        const struct { const void *p; uint64_t bytes; } outs[] = {{cluster, 4ull * n_vertices}, {out_vertices, 12ull * vertex_capacity},
                                                                  {first, 4ull * vertex_capacity}, {out_faces, 12ull * tri_capacity},
                                                                  {source, 4ull * tri_capacity}, {counts, 8}};
        for (const auto &o : outs)
            if (overlaps(o.p, o.bytes, vertices, vb) || overlaps(o.p, o.bytes, faces, fb))
                return fail(DRT_ERR_INVALID, "an output may not alias vertices or faces");
    }
    if (r->pending) return fail(DRT_ERR_INVALID, "an asynchronous render batch is pending: drt_renderer_wait first");
    HIP_TRY(hipSetDevice(r->device));
    (void)hipGetLastError();                   // (see render_batch_impl: only this call's own errors count)
    if (!on_renderer_device(r, counts) ||
        (!empty && (!on_renderer_device(r, vertices) || (n_tris && !on_renderer_device(r, faces)) || !on_renderer_device(r, cluster) ||
                    (vertex_capacity && (!on_renderer_device(r, out_vertices) || !on_renderer_device(r, first))) ||
                    (tri_capacity && (!on_renderer_device(r, out_faces) || !on_renderer_device(r, source))))))
        return fail(DRT_ERR_INVALID, "vertices, faces, cluster, out_vertices, first, out_faces, source and counts must be device memory on the renderer's device");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : r->stream;
    if (int rc = query_order(r, s)) return rc;
    if (empty) {
        HIP_TRY(hipMemsetAsync(counts, 0, 2 * sizeof(uint32_t), s));
        return query_recorded(r, s);
    }
    const bool quadric = placement == DRT_SIMPLIFY_QUADRIC;
    const uint64_t slots = simplify_table_slots(n_vertices);
    const size_t sum_words = vertex_capacity ? (size_t)(quadric ? kSimplifyWords : kSimplifyMeanWords) * n_vertices : 0;
    // the table, the representatives, the block totals, the word of the maximum and the 64-bit sums are the welding calls' scratch
    if (int rc = grow(r, r->wd_table, slots)) return rc;
    if (int rc = grow(r, r->wd_rep, n_vertices)) return rc;
    if (int rc = grow(r, r->wd_blocks, simplify_blocks(std::max(n_vertices, n_tris)))) return rc;
    if (int rc = grow(r, r->wd_max, 2)) return rc;
    if (int rc = grow(r, r->sp_key, n_vertices)) return rc;
    if (int rc = grow(r, r->sp_cnt, n_vertices)) return rc;
    if (sum_words) if (int rc = grow(r, r->wd_acc, sum_words)) return rc;
    SimplifyArgs a;
    a.vertices = vertices; a.faces = faces; a.n_vertices = n_vertices; a.n_tris = n_tris;
    for (int k = 0; k < 3; k++) { a.grid.lo[k] = grid->lo[k]; a.grid.cell[k] = grid->cell[k]; a.grid.dims[k] = grid->dims[k]; }
    a.key = r->sp_key.ptr; a.table = r->wd_table.ptr; a.mask = (uint32_t)(slots - 1); a.rep = r->wd_rep.ptr;
    a.block_totals = r->wd_blocks.ptr; a.cnt = r->sp_cnt.ptr; a.sums = reinterpret_cast<long long *>(r->wd_acc.ptr);
    a.max_bits = r->wd_max.ptr;
    // DRT_SIMPLIFY_SUMS=plain: one atomic per term, for tools/simplify_bench.py to measure against; the results are the same bytes
    const char *sums_env = std::getenv("DRT_SIMPLIFY_SUMS");
    a.combine_runs = !(sums_env && std::strcmp(sums_env, "plain") == 0);
    a.cluster = cluster; a.out_vertices = out_vertices; a.first = first; a.vertex_capacity = vertex_capacity;
    a.out_faces = out_faces; a.source = source; a.tri_capacity = tri_capacity; a.counts = counts;
    if (sum_words) {
        HIP_TRY(hipMemsetAsync(r->sp_cnt.ptr, 0, (size_t)n_vertices * sizeof(uint32_t), s));
        HIP_TRY(hipMemsetAsync(r->wd_acc.ptr, 0, sum_words * sizeof(unsigned long long), s));
        HIP_TRY(hipMemsetAsync(r->wd_max.ptr, 0, 2 * sizeof(uint32_t), s));
    }
    HIP_TRY(launch_simplify(quadric ? SimplifyPlacement::quadric : SimplifyPlacement::mean, a, r->num_cus, s));
    return query_recorded(r, s);
}

}  // extern "C"
