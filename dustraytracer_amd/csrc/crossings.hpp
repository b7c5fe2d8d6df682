// crossings.hpp -- launch seam of kernel_crossings.hip (crossing counts of rays, the inside vote of points and the sign of a
// nearest record: include/drt.h drt_renderer_crossings / drt_renderer_inside / drt_renderer_signed_distance), and the triangle
// test restated with the determinant's sign.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_scene.hpp"
#ifdef __HIP__
#include "device_math.hpp"
#endif
#include "ray_query.hpp"

namespace drt {

// The three directions of the inside vote (drt.h "inside vote"): used as given, no component is zero.
constexpr float kInsideDirs[3][3] = {{0.6180340f, 0.4142136f, 0.6687403f},
                                     {-0.7320508f, 0.2360680f, 0.6403124f},
                                     {0.3166248f, -0.8660254f, 0.3872983f}};

enum class CrossingsOut : uint32_t {
    crossings = 0,               // ray mode: drt_crossings[n]
    votes = 1,                   // point mode: uint8_t[n], the number of rays voting inside
    side = 2,                    // point mode: the 4-byte `side` word at byte 28 of drt_nearest[n], -1 inside / +1 outside
};

// The grid, the claim heads and the HBM stack are the occlusion ray query's (ray_query.hpp): kRqThreads-thread workgroups,
// kRqWavesPerSimd waves per SIMD, kRqShards heads, kRqLdsLevelsOccluded reference-only stack levels in LDS and the rest in
// ray_query_stack_bytes(num_cus, levels, true) bytes of HBM.
struct CrossingsArgs {
    const void *in;              // drt_ray[n] (32 B, 16-B aligned) or drt_point[n] (16 B, 16-B aligned)
    void *out;                   // what `kind` says
    QueryFrame frame;            // n, tree depth, refill threshold, claim heads, HBM stack: 4 B stack entries
    uint32_t rule;               // point mode: 0 parity (count odd), 1 winding (winding != 0)
};

hipError_t launch_crossings(const SceneView &scene, CrossingsOut kind, const CrossingsArgs &args, int num_cus, hipStream_t stream);

#ifdef __HIP__                                      // device code: the .hip translation units only
// tri_intersect_flat (device_math.hpp, Intersection.cu:4-36) with det handed out: the same operations on the same values in the
// same order, so hit and t have tri_intersect_flat's bits.  u and v stay inside: a crossing has no use for them.
DRT_DEV bool tri_intersect_det(const Ray &ray, f3 v0, f3 e1, f3 e2, float &t, float &det) {
    f3 pvec = cross(ray.dir, e2);
    det = dot(e1, pvec);
    int ok = !(__builtin_fabsf(det) < DRT_TRIANGLE_EPSILON);
    float inv_det = exact_rcp_not_tiny(det);          // !ok covers |det| < 1e-6: whatever comes back there is not used
    f3 tvec = ray.orig - v0;
    float u = inv_det * dot(tvec, pvec);
    f3 qvec = cross(tvec, e1);
    float v = inv_det * dot(ray.dir, qvec);
    ok = ok & (int)(!(fminf(u, v) < 0.0f)) & (int)(!(fmaxf(u, u + v) > 1.0f));
    t = inv_det * dot(e2, qvec);
    ok = ok & (int)(t > DRT_TRIANGLE_EPSILON);
    return ok != 0;
}
#endif

}  // namespace drt
