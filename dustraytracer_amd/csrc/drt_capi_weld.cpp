// drt_capi_weld.cpp -- the welding entry points of include/drt.h (drt_renderer_weld, drt_renderer_vertex_normals,
// drt_renderer_smooth_vertices; kernel_weld.hip): every argument check before any device work, in drt_renderer_isosurface's order and
// style, then the renderer's scratch, grown on demand, and the launches.  The calls read no scene and no tree; they share scratch with
// each other, so they order themselves as the queries do (query_order / query_recorded: one event).
#include "renderer_state.hpp"

#include <cmath>

#include "weld.hpp"

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

// the checks the two indexed-mesh calls share, behind their own; `out` is the float [V][3] result
int check_indexed(const float *vertices, uint32_t n_vertices, const int32_t *faces, uint32_t n_tris, const float *out) {
    if (!vertices || !out) return fail(DRT_ERR_INVALID, "null vertices or out");
    if (n_tris && !faces) return fail(DRT_ERR_INVALID, "null faces");
    if (misaligned4(vertices) || misaligned4(faces) || misaligned4(out)) return fail(DRT_ERR_INVALID, "vertices, faces and out must be 4-byte aligned");
    if ((uint64_t)n_tris * 3 > 0x7fffffffu) return fail(DRT_ERR_INVALID, std::to_string(n_tris) + " triangles: 3 N < 2^31 expected");
    if (n_vertices > 0x7fffffffu) return fail(DRT_ERR_INVALID, std::to_string(n_vertices) + " vertices: fewer than 2^31 expected");
    return DRT_OK;
}

}  // namespace

extern "C" {

int drt_renderer_weld(drt_renderer *r, const void *tris, uint32_t n, uint32_t stride, int32_t *faces, int32_t *first, float *vertices,
                      uint32_t capacity, uint32_t *vertex_count, void *hip_stream) {
    if (!r || !vertex_count) return fail(DRT_ERR_INVALID, "null argument");
    if (stride != 36 && stride != 48) return fail(DRT_ERR_INVALID, "stride " + std::to_string(stride) + ": 36 ([N][3][3] floats) or 48 (drt_tri) expected");
    if ((uint64_t)n * 3 > 0x7fffffffu) return fail(DRT_ERR_INVALID, std::to_string(n) + " triangles: 3 N < 2^31 expected");
    if (n && (!tris || !faces)) return fail(DRT_ERR_INVALID, "null tris or faces");
    if ((first == nullptr) != (capacity == 0)) return fail(DRT_ERR_INVALID, "first must be null if and only if capacity is 0");
    if (vertices && !first) return fail(DRT_ERR_INVALID, "vertices without first: a capacity is needed");
    if (misaligned4(tris) || misaligned4(faces) || misaligned4(first) || misaligned4(vertices) || misaligned4(vertex_count))
        return fail(DRT_ERR_INVALID, "tris, faces, first, vertices and vertex_count must be 4-byte aligned");
    if (r->pending) return fail(DRT_ERR_INVALID, "an asynchronous render batch is pending: drt_renderer_wait first");
    HIP_TRY(hipSetDevice(r->device));
    (void)hipGetLastError();                   // (see render_batch_impl: only this call's own errors count)
    if ((n && (!on_renderer_device(r, tris) || !on_renderer_device(r, faces))) || (first && !on_renderer_device(r, first)) ||
        (vertices && !on_renderer_device(r, vertices)) || !on_renderer_device(r, vertex_count))
        return fail(DRT_ERR_INVALID, "tris, faces, first, vertices and vertex_count must be device memory on the renderer's device");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : r->stream;
    if (int rc = query_order(r, s)) return rc;
    WeldArgs a;
    a.tris = static_cast<const unsigned char *>(tris); a.stride = stride; a.corners = 3 * n;
    a.faces = faces; a.first = first; a.vertices = vertices; a.capacity = capacity; a.vertex_count = vertex_count;
    const uint64_t slots = weld_table_slots(a.corners);
    a.mask = (uint32_t)(slots - 1);
    a.table = nullptr; a.rep = nullptr; a.block_totals = nullptr;
    if (n) {
        if (int rc = grow(r, r->wd_table, slots)) return rc;
        if (int rc = grow(r, r->wd_rep, a.corners)) return rc;
        if (int rc = grow(r, r->wd_blocks, weld_blocks(a.corners))) return rc;
        a.table = r->wd_table.ptr; a.rep = r->wd_rep.ptr; a.block_totals = r->wd_blocks.ptr;
    }
    HIP_TRY(launch_weld(a, s));
    return query_recorded(r, s);
}

int drt_renderer_vertex_normals(drt_renderer *r, const float *vertices, uint32_t n_vertices, const int32_t *faces, uint32_t n_tris,
                                int32_t weight, float *out, void *hip_stream) {
    if (!r) return fail(DRT_ERR_INVALID, "null argument");
    if (weight != DRT_NORMALS_ANGLE && weight != DRT_NORMALS_AREA)
        return fail(DRT_ERR_INVALID, "weight " + std::to_string(weight) + ": DRT_NORMALS_ANGLE (0) or DRT_NORMALS_AREA (1) expected");
    if (n_vertices == 0) return DRT_OK;
    if (int rc = check_indexed(vertices, n_vertices, faces, n_tris, out)) return rc;
    if (r->pending) return fail(DRT_ERR_INVALID, "an asynchronous render batch is pending: drt_renderer_wait first");
    HIP_TRY(hipSetDevice(r->device));
    (void)hipGetLastError();
    if (!on_renderer_device(r, vertices) || (n_tris && !on_renderer_device(r, faces)) || !on_renderer_device(r, out))
        return fail(DRT_ERR_INVALID, "vertices, faces and out must be device memory on the renderer's device");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : r->stream;
    if (int rc = query_order(r, s)) return rc;
    if (int rc = grow(r, r->wd_acc, 3 * (size_t)n_vertices)) return rc;
    if (int rc = grow(r, r->wd_max, 2)) return rc;
    HIP_TRY(hipMemsetAsync(r->wd_acc.ptr, 0, 3 * (size_t)n_vertices * sizeof(unsigned long long), s));
    HIP_TRY(hipMemsetAsync(r->wd_max.ptr, 0, 2 * sizeof(uint32_t), s));
    NormalsArgs a;
    a.vertices = vertices; a.faces = faces; a.n_vertices = n_vertices; a.n_tris = n_tris;
    a.acc = reinterpret_cast<long long *>(r->wd_acc.ptr); a.max_bits = r->wd_max.ptr; a.out = out;
    HIP_TRY(launch_vertex_normals(weight == DRT_NORMALS_AREA ? NormalWeight::area : NormalWeight::angle, a, r->num_cus, s));
    return query_recorded(r, s);
}

int drt_renderer_smooth_vertices(drt_renderer *r, const float *vertices, uint32_t n_vertices, const int32_t *faces, uint32_t n_tris,
                                 const float *factors, uint32_t n_factors, const uint8_t *fixed, float *out, void *hip_stream) {
    if (!r) return fail(DRT_ERR_INVALID, "null argument");
    if (n_factors && !factors) return fail(DRT_ERR_INVALID, "null factors");
    for (uint32_t i = 0; i < n_factors; i++)
        if (!(std::fabs(factors[i]) <= 1.0f))
            return fail(DRT_ERR_INVALID, "factors[" + std::to_string(i) + "] = " + std::to_string(factors[i]) + ": |f| <= 1 expected");
    if (n_vertices == 0) return DRT_OK;
    if (int rc = check_indexed(vertices, n_vertices, faces, n_tris, out)) return rc;
    const uintptr_t in0 = (uintptr_t)vertices, out0 = (uintptr_t)out, bytes = 12 * (uintptr_t)n_vertices;
    if (in0 < out0 + bytes && out0 < in0 + bytes) return fail(DRT_ERR_INVALID, "out may not alias vertices");
    if (r->pending) return fail(DRT_ERR_INVALID, "an asynchronous render batch is pending: drt_renderer_wait first");
    HIP_TRY(hipSetDevice(r->device));
    (void)hipGetLastError();
    if (!on_renderer_device(r, vertices) || (n_tris && !on_renderer_device(r, faces)) || (fixed && !on_renderer_device(r, fixed)) ||
        !on_renderer_device(r, out))
        return fail(DRT_ERR_INVALID, "vertices, faces, fixed and out must be device memory on the renderer's device");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : r->stream;
    if (int rc = query_order(r, s)) return rc;
    if (n_factors == 0) {                                                        // no step: the input's bits
        HIP_TRY(hipMemcpyAsync(out, vertices, bytes, hipMemcpyDeviceToDevice, s));
        return query_recorded(r, s);
    }
    const size_t acc_words = 3 * (size_t)n_vertices, all_words = acc_words + ((size_t)n_vertices + 1) / 2;    // the counts: 4 bytes each
    if (int rc = grow(r, r->wd_acc, all_words)) return rc;
    if (int rc = grow(r, r->wd_max, 2)) return rc;
    if (n_factors >= 2) if (int rc = grow(r, r->wd_pos[0], 3 * (size_t)n_vertices)) return rc;
    if (n_factors >= 3) if (int rc = grow(r, r->wd_pos[1], 3 * (size_t)n_vertices)) return rc;
    SmoothArgs a;
    a.faces = faces; a.fixed = fixed; a.n_vertices = n_vertices; a.n_tris = n_tris;
    a.acc = reinterpret_cast<long long *>(r->wd_acc.ptr);
    a.cnt = reinterpret_cast<uint32_t *>(r->wd_acc.ptr + acc_words);
    a.max_bits = r->wd_max.ptr;
    a.src = vertices; a.dst = nullptr; a.step = 0; a.factor = 0.0f;
    HIP_TRY(hipMemsetAsync(r->wd_max.ptr, 0, 2 * sizeof(uint32_t), s));
    HIP_TRY(launch_smooth_maximum(a, r->num_cus, s));
    for (uint32_t step = 0; step < n_factors; step++) {
        a.step = step; a.factor = factors[step];
        a.dst = step + 1 == n_factors ? out : r->wd_pos[step & 1u].ptr;          // (a step never writes the buffer it reads)
        HIP_TRY(hipMemsetAsync(r->wd_acc.ptr, 0, all_words * sizeof(unsigned long long), s));
        HIP_TRY(launch_smooth_step(a, r->num_cus, s));
        a.src = a.dst;
    }
    return query_recorded(r, s);
}

}  // extern "C"
