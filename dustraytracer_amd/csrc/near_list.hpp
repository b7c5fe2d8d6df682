// near_list.hpp -- launch seam of kernel_near_list.hip (nearest-triangle lists of points, k-nearest and within-radius: include/drt.h
// drt_renderer_nearest_list), and the two routines of the nearest query restated.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_scene.hpp"
#ifdef __HIP__
#include "device_math.hpp"
#endif
#include "ray_query.hpp"

namespace drt {

// The grid, the claim heads and the HBM stack are the closest-hit ray query's (ray_query.hpp), as nearest.hpp's are: kRqThreads-thread
// workgroups, kRqWavesPerSimd waves per SIMD, kRqShards heads, kRqLdsLevelsClosest stack levels {ref, box2} in LDS and the rest in
// ray_query_stack_bytes(num_cus, levels, false) bytes of HBM.
struct NearListArgs {
    const void *points;          // drt_point[n] (16 B, 16-B aligned)
    const uint32_t *offsets;     // n + 1 words: point i owns near[offsets[i] .. offsets[i + 1]), clamped to near_capacity
    void *near;                  // drt_near[near_capacity] (16 B, 16-B aligned); may be null when near_capacity == 0
    void *surf;                  // drt_near_surf[near_capacity] (16 B, 16-B aligned) or null
    uint32_t *counts;            // n words or null: GATHER every listed triangle of the point, K the stored ones
    uint32_t near_capacity;
    QueryFrame frame;            // n, tree depth, refill threshold, claim heads, HBM stack: 8 B stack entries
};

// k_mode: DRT_NEAR_K (the search bound shrinks to the tail of a full list) or DRT_NEAR_GATHER (it never does)
hipError_t launch_near_list(const SceneView &scene, bool k_mode, const NearListArgs &args, int num_cus, hipStream_t stream);

#ifdef __HIP__                                      // device code: the .hip translation units only
// kernel_nearest.hip's box_dist2, restated: the same operations on the same values in the same order.  drt.h "box distance": a NaN
// coordinate of p drops out of both max (v_max_f32 in IEEE mode), so its axis contributes 0
DRT_DEV float near_box_dist2(f3 bmin, f3 bmax, f3 p) {
    const float dx = fmaxf(fmaxf(bmin.x - p.x, 0.0f), p.x - bmax.x);
    const float dy = fmaxf(fmaxf(bmin.y - p.y, 0.0f), p.y - bmax.y);
    const float dz = fmaxf(fmaxf(bmin.z - p.z, 0.0f), p.z - bmax.z);
    return dx * dx + dy * dy + dz * dz;
}

// kernel_nearest.hip's closest_on_triangle, restated: the same operations on the same values in the same order, so dist2, u and v
// have drt_renderer_nearest's bits.  drt.h "per triangle": cases 3, 5, 6 and 7 are each one quotient num / den of values all cases
// share; the chain picks its operands with the cases' priority, divides once, and then picks (u, v) over all seven, last case first
// so that the first matching one wins.
DRT_DEV float near_closest_on_triangle(f3 p, f3 v0, f3 e1, f3 e2, float &u, float &v) {
    const f3 ap = p - v0;
    const float d1 = dot(e1, ap), d2 = dot(e2, ap);
    const f3 bp = ap - e1;
    const float d3 = dot(e1, bp), d4 = dot(e2, bp);
    const f3 cp = ap - e2;
    const float d5 = dot(e1, cp), d6 = dot(e2, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float d43 = d4 - d3, d56 = d5 - d6;
    const bool c1 = d1 <= 0.0f && d2 <= 0.0f;
    const bool c2 = d3 >= 0.0f && d4 <= d3;
    const bool c3 = vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f;
    const bool c4 = d6 >= 0.0f && d5 <= d6;
    const bool c5 = vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f;
    const bool c6 = va <= 0.0f && d43 >= 0.0f && d56 >= 0.0f;
    float num = 1.0f, den = (va + vb) + vc;                    // 7: den = 1 / ((va + vb) + vc)
    num = c6 ? d43 : num; den = c6 ? d43 + d56 : den;           // 6: w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
    num = c5 ? d2 : num;  den = c5 ? d2 - d6 : den;             // 5: d2 / (d2 - d6)
    num = c3 ? d1 : num;  den = c3 ? d1 - d3 : den;             // 3: d1 / (d1 - d3)
    const float q = num / den;
    u = vb * q; v = vc * q;                                     // 7
    u = c6 ? 1.0f - q : u; v = c6 ? q : v;                      // 6
    u = c5 ? 0.0f : u;     v = c5 ? q : v;                      // 5
    u = c4 ? 0.0f : u;     v = c4 ? 1.0f : v;                   // 4
    u = c3 ? q : u;        v = c3 ? 0.0f : v;                   // 3
    u = c2 ? 1.0f : u;     v = c2 ? 0.0f : v;                   // 2
    u = c1 ? 0.0f : u;     v = c1 ? 0.0f : v;                   // 1
    const f3 diff = p - ((v0 + e1 * u) + e2 * v);
    return dot(diff, diff);
}
#endif

}  // namespace drt
