// drt_capi_surface.cpp -- the surface entry points of include/drt.h (drt_renderer_surface_lookup, drt_renderer_surface_weights,
// drt_renderer_sample_surface; kernel_surface.hip): drt_renderer_trace_rays' argument checks in its order (the handles, n == 0, the
// pointers, the alignment, n < 2^31, a pending batch, device memory), the scene upload, the queries' stream ordering, the buffers this
// feature owns, and the launches.  Nothing here traverses the BVH, so there is no traversal scratch and no depth limit.
#include "renderer_state.hpp"

#include "surface.hpp"

using namespace drt;

namespace {

int open_call(drt_renderer *r) {
    if (r->pending) return fail(DRT_ERR_INVALID, "an asynchronous render batch is pending: drt_renderer_wait first");
    HIP_TRY(hipSetDevice(r->device));
    (void)hipGetLastError();                   // (see render_batch_impl: only this call's own errors count)
    return DRT_OK;
}

// device memory of the renderer's device that holds `bytes` bytes from p on (as far as the runtime can tell)
bool device_range(const drt_renderer *r, const void *p, size_t bytes) {
    if (!on_renderer_device(r, p)) return false;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return true; }
    return (const char *)p >= (const char *)base && bytes <= size - (size_t)((const char *)p - (const char *)base);
}

// The scene copy as for rendering.  upload_scene refuses a tree deeper than the traversal stacks AFTER it has made the copy; nothing
// here traverses, so that refusal alone does not stop a lookup (a scene without a BVH, a bad index, a device error still do).
int scene_copy(drt_renderer *r, const drt_scene *scene) {
    const int rc = upload_scene(r, scene);
    if (rc == DRT_ERR_UNSUPPORTED && r->uploaded_scene == scene && r->uploaded_revision == scene->host.revision) return DRT_OK;
    return rc;
}

// The host scene's vertex normals in tree order and the load-order table: made by the first lookup after an upload (free_scene drops
// them with the scene copy, so they are of the scene that is on the device)
int surface_tables(drt_renderer *r, const drt_scene *scene) {
    if (r->sf_built) return DRT_OK;
    const std::vector<drt_triangle> &tris = scene->host.triangles;
    std::vector<float> nrm(9 * tris.size());
    for (size_t i = 0; i < tris.size(); i++)
        for (int k = 0; k < 3; k++) std::memcpy(&nrm[9 * i + 3 * (size_t)k], tris[i].vertex[k].normal, 12);
    std::vector<int32_t> order = scene->host.load_index;
    order.resize(tris.size(), 0);
    for (size_t i = 0; i < order.size(); i++)                         // (the kernel indexes the caller's normals with it)
        if (order[i] < 0 || (size_t)order[i] >= tris.size()) return fail(DRT_ERR_INVALID, "the scene's load-order table is not a permutation");
    HIP_TRY(r->sf_normals.upload(nrm));
    HIP_TRY(r->sf_order.upload(order));
    r->sf_built = true;
    return DRT_OK;
}

// a scratch array of at least n words: it grows only once the query in flight, which may read the old one, is over
template <class T>
int grow(drt_renderer *r, drt_renderer::DeviceArray<T> &a, size_t n) {
    if (a.ptr && a.count >= n) return DRT_OK;
    if (r->query_recorded) HIP_TRY(hipEventSynchronize(r->ev_query));
    HIP_TRY(a.alloc(n));
    return DRT_OK;
}

// the table of the uploaded scene into `cdf` (n_tris words) on stream s
int enqueue_weights(drt_renderer *r, uint64_t *cdf, hipStream_t s) {
    const uint32_t n_tris = r->view.n_tris;
    if (n_tris == 0) return DRT_OK;
    if (int rc = grow(r, r->sf_blocks, (n_tris + kSurfScanBlock - 1) / kSurfScanBlock)) return rc;
    if (int rc = grow(r, r->sf_amax, 1)) return rc;
    SurfaceScanArgs a;
    a.hot = r->view.tri_hot; a.n_tris = n_tris;
    a.amax_bits = r->sf_amax.ptr;
    a.block_totals = reinterpret_cast<uint64_t *>(r->sf_blocks.ptr);
    a.cdf = cdf;
    HIP_TRY(launch_surface_weights(a, s));
    return DRT_OK;
}

}  // namespace

extern "C" {

int drt_renderer_surface_lookup(drt_renderer *r, const drt_scene *scene, const drt_hit *refs, const float *normals, drt_surface *out,
                                uint32_t n, void *hip_stream) {
    if (!r || !scene) return fail(DRT_ERR_INVALID, "null argument");
    if (n == 0) return DRT_OK;
    if (!refs || !out) return fail(DRT_ERR_INVALID, "null reference or result pointer");
    if (((uintptr_t)refs & 15u) != 0 || ((uintptr_t)out & 15u) != 0) return fail(DRT_ERR_INVALID, "refs and results must be 16-byte aligned");
    if (((uintptr_t)normals & 3u) != 0) return fail(DRT_ERR_INVALID, "normals must be 4-byte aligned");
    if (n > 0x7fffffffu) return fail(DRT_ERR_INVALID, "at most 2^31 - 1 references per call");
    if (int rc = open_call(r)) return rc;
    if (!on_renderer_device(r, refs) || !on_renderer_device(r, out))
        return fail(DRT_ERR_INVALID, "refs and results must be device memory on the renderer's device");
    if (normals && !device_range(r, normals, 9 * sizeof(float) * scene->host.triangles.size()))
        return fail(DRT_ERR_INVALID, "normals must be float[n_tris][3][3] in device memory on the renderer's device");
    if (int rc = scene_copy(r, scene)) return rc;
    if (int rc = surface_tables(r, scene)) return rc;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : r->stream;
    if (int rc = query_order(r, s)) return rc;
    SurfaceArgs a;
    a.refs = reinterpret_cast<const SurfRef *>(refs); a.out = reinterpret_cast<SurfRecord *>(out); a.n = n;
    a.own_normals = r->sf_normals.ptr; a.load_index = r->sf_order.ptr; a.normals = normals;
    HIP_TRY(launch_surface_lookup(r->view, a, r->num_cus, s));
    return query_recorded(r, s);
}

int drt_renderer_surface_weights(drt_renderer *r, const drt_scene *scene, uint64_t *cdf, void *hip_stream) {
    if (!r || !scene) return fail(DRT_ERR_INVALID, "null argument");
    if (scene->host.triangles.empty() && !scene->host.nodes.empty()) return DRT_OK;      // an empty table: nothing to write
    if (!cdf) return fail(DRT_ERR_INVALID, "null table pointer");
    if (((uintptr_t)cdf & 15u) != 0) return fail(DRT_ERR_INVALID, "the table must be 16-byte aligned");
    if (int rc = open_call(r)) return rc;
    if (!device_range(r, cdf, sizeof(uint64_t) * scene->host.triangles.size()))
        return fail(DRT_ERR_INVALID, "the table must be uint64[n_tris] in device memory on the renderer's device");
    if (int rc = scene_copy(r, scene)) return rc;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : r->stream;
    if (int rc = query_order(r, s)) return rc;
    if (int rc = enqueue_weights(r, cdf, s)) return rc;
    return query_recorded(r, s);
}

int drt_renderer_sample_surface(drt_renderer *r, const drt_scene *scene, uint32_t seed, uint32_t first, drt_hit *out, uint32_t n,
                                void *hip_stream) {
    if (!r || !scene) return fail(DRT_ERR_INVALID, "null argument");
    if (n == 0) return DRT_OK;
    if (!out) return fail(DRT_ERR_INVALID, "null result pointer");
    if (((uintptr_t)out & 15u) != 0) return fail(DRT_ERR_INVALID, "results must be 16-byte aligned");
    if (n > 0x7fffffffu) return fail(DRT_ERR_INVALID, "at most 2^31 - 1 samples per call");
    if ((uint64_t)first + n > ((uint64_t)1 << 32)) return fail(DRT_ERR_INVALID, "first + n must not exceed 2^32");
    if (int rc = open_call(r)) return rc;
    if (!on_renderer_device(r, out)) return fail(DRT_ERR_INVALID, "results must be device memory on the renderer's device");
    if (int rc = scene_copy(r, scene)) return rc;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : r->stream;
    if (int rc = query_order(r, s)) return rc;
    if (int rc = grow(r, r->sf_cdf, r->view.n_tris)) return rc;
    uint64_t *cdf = reinterpret_cast<uint64_t *>(r->sf_cdf.ptr);
    if (int rc = enqueue_weights(r, cdf, s)) return rc;                // the table is made again by every call: one pass over the triangles
    HIP_TRY(launch_surface_sample(cdf, r->view.n_tris, seed, first, reinterpret_cast<SurfRef *>(out), n, r->num_cus, s));
    return query_recorded(r, s);
}

}  // extern "C"
