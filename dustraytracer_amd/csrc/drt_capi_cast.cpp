// drt_capi_cast.cpp -- the triangle-cast entry point of include/drt.h (drt_renderer_triangle_cast, kernel_tri_cast.hip): the triangle
// distance entry's argument checks in its order (the handles, the mode, n == 0, the pointers, the alignment, n < 2^31, a pending batch,
// device memory), the scene upload, the nearest query's stream ordering and scratch, and the launch.
#include "renderer_state.hpp"

#include "tri_cast.hpp"

using namespace drt;

extern "C" {

// The closest-hit query's HBM stack ({ref, enter} entries).
int drt_renderer_triangle_cast(drt_renderer *r, const drt_scene *scene, const drt_tri *tris, const drt_motion *motions, drt_tri_hit *out,
                               uint32_t n, int32_t mode, void *hip_stream) {
    if (!r || !scene) return fail(DRT_ERR_INVALID, "null argument");
    if (mode != DRT_TRICAST_FIRST && mode != DRT_TRICAST_ANY)
        return fail(DRT_ERR_INVALID, "mode " + std::to_string(mode) + ": 0 (first) or 1 (any) expected");
    if (n == 0) return DRT_OK;
    if (!tris || !motions || !out) return fail(DRT_ERR_INVALID, "null triangle, motion or result pointer");
    if (((uintptr_t)tris & 15u) != 0 || ((uintptr_t)motions & 15u) != 0 || ((uintptr_t)out & 15u) != 0)
        return fail(DRT_ERR_INVALID, "tris, motions and results must be 16-byte aligned");
    hipStream_t s;
    if (int rc = query_open(r, scene, n, {tris, motions, out}, "casts", "tris, motions and results", hip_stream, false, &s)) return rc;
    TriCastArgs a;
    a.tris = tris; a.motions = motions; a.out = out; a.frame = query_frame(r, n);
    HIP_TRY(launch_tri_cast(r->view, mode == DRT_TRICAST_ANY, a, r->num_cus, s));
    return query_recorded(r, s);
}

}  // extern "C"
