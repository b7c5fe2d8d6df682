// drt_capi_distance.cpp -- the triangle-distance entry point of include/drt.h (drt_renderer_triangle_distance,
// kernel_tri_distance.hip): the triangle overlap entry's argument checks in its order (the handles, the mode, n == 0, the pointers, the
// alignment, n < 2^31, a pending batch, device memory), the scene upload, the nearest query's stream ordering and scratch, and the launch.
#include "renderer_state.hpp"

#include "tri_distance.hpp"

using namespace drt;

extern "C" {

// The closest-hit query's HBM stack ({ref, box2} entries).
int drt_renderer_triangle_distance(drt_renderer *r, const drt_scene *scene, const drt_tri *tris, const float *max_dist, drt_tri_near *out,
                                   uint32_t n, int32_t mode, void *hip_stream) {
    if (!r || !scene) return fail(DRT_ERR_INVALID, "null argument");
    if (mode != DRT_TRIDIST_NEAREST && mode != DRT_TRIDIST_ANY)
        return fail(DRT_ERR_INVALID, "mode " + std::to_string(mode) + ": 0 (nearest) or 1 (any) expected");
    if (n == 0) return DRT_OK;
    if (!tris || !out) return fail(DRT_ERR_INVALID, "null triangle or result pointer");
    if (((uintptr_t)tris & 15u) != 0 || ((uintptr_t)out & 15u) != 0 || ((uintptr_t)max_dist & 3u) != 0)
        return fail(DRT_ERR_INVALID, "tris and results must be 16-byte aligned, max_dist 4-byte aligned");
    hipStream_t s;
    if (int rc = query_open(r, scene, n, {tris, out, max_dist}, "triangles", "tris, max_dist and results", hip_stream, false, &s)) return rc;
    TriDistanceArgs a;
    a.tris = tris; a.max_dist = max_dist; a.out = out; a.frame = query_frame(r, n);
    HIP_TRY(launch_tri_distance(r->view, mode == DRT_TRIDIST_ANY, a, r->num_cus, s));
    return query_recorded(r, s);
}

}  // extern "C"
