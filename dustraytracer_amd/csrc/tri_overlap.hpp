// tri_overlap.hpp -- launch seam of kernel_tri_overlap.hip (triangle overlap queries, the mesh triangles that each query triangle touches:
// include/drt.h drt_renderer_overlap_triangles), and the query's routines: the load of a drt_tri, its validity and bounds, and the
// triangle-triangle test.  The node cull is overlap.hpp's overlap_cull_passes, unchanged.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_scene.hpp"
#ifdef __HIP__
#include "device_math.hpp"
#endif
#include "overlap.hpp"
#include "ray_query.hpp"

namespace drt {

// The grid, the claim heads and the HBM stack are the occlusion ray query's (ray_query.hpp), as overlap.hpp's are.
struct TriOverlapArgs {
    const void *tris;            // drt_tri[n] (48 B, 16-B aligned)
    const uint32_t *offsets;     // n + 1 words: query i owns prims[offsets[i] .. offsets[i + 1]), clamped to prims_capacity (LIST only)
    int32_t *prims;              // int32[prims_capacity]; null when prims_capacity == 0
    uint32_t *counts;            // n words or null: LIST every listed triangle of the query, ANY 0 or 1
    uint32_t prims_capacity;
    QueryFrame frame;            // n, tree depth, refill threshold, claim heads, HBM stack: 4 B stack entries
};

// The triangle test needs more than the 64 VGPRs of kRqWavesPerSimd waves per SIMD (kernel_tri_overlap.hip): the kernel is bounded to
// this many, and its grid is this many workgroups per CU, which the HBM stack of ray_query_max_blocks workgroups holds.
constexpr int kTriOverlapWavesPerSimd = 5;
static_assert(kTriOverlapWavesPerSimd <= kRqWavesPerSimd, "the HBM stack is sized for kRqWavesPerSimd workgroups per CU");

// any_mode: DRT_OVERLAP_ANY (the traversal ends at the first listed triangle) or DRT_OVERLAP_LIST
hipError_t launch_tri_overlap(const SceneView &scene, bool any_mode, const TriOverlapArgs &args, int num_cus, hipStream_t stream);

#ifdef __HIP__                                      // device code: the .hip translation units only
// A query as the lane keeps it while it owns it: q0 and everything that depends on the query alone.  (q1 = q0 + a1 is not kept: the
// test is relative to q0 and reads the edges only.)
struct TriOverlapQuery { f3 q0, a1, a2, g, nq; };

// a drt_tri as its three 16-byte words hold it: v[0], v[1], v[2] and three pad words that are ignored
struct TriOverlapVerts { f3 q0, q1, q2; };
DRT_DEV TriOverlapVerts tri_overlap_load(const void *tris, uint32_t i) {
    const float4 *q = reinterpret_cast<const float4 *>(tris) + 3 * (size_t)i;
    const float4 a = q[0], b = q[1], c = q[2];                                // (c.y, c.z, c.w are the pad words)
    TriOverlapVerts t;
    t.q0 = mk3(a.x, a.y, a.z); t.q1 = mk3(a.w, b.x, b.y); t.q2 = mk3(b.z, b.w, c.x);
    return t;
}

// drt.h "validity": all nine coordinates satisfy fabsf(x) <= FLT_MAX (a NaN or an infinity fails)
DRT_DEV bool tri_overlap_finite(f3 v) { return fabsf(v.x) <= 3.402823466e+38f && fabsf(v.y) <= 3.402823466e+38f && fabsf(v.z) <= 3.402823466e+38f; }
DRT_DEV bool tri_overlap_valid(const TriOverlapVerts &t) { return tri_overlap_finite(t.q0) && tri_overlap_finite(t.q1) && tri_overlap_finite(t.q2); }

// drt.h "bounds": qmin[j] = min3(q0[j], q1[j], q2[j]), qmax likewise
DRT_DEV f3 tri_overlap_min(const TriOverlapVerts &t) {
    return mk3(overlap_min3(t.q0.x, t.q1.x, t.q2.x), overlap_min3(t.q0.y, t.q1.y, t.q2.y), overlap_min3(t.q0.z, t.q1.z, t.q2.z));
}
DRT_DEV f3 tri_overlap_max(const TriOverlapVerts &t) {
    return mk3(overlap_max3(t.q0.x, t.q1.x, t.q2.x), overlap_max3(t.q0.y, t.q1.y, t.q2.y), overlap_max3(t.q0.z, t.q1.z, t.q2.z));
}

// a1 = q1 - q0, a2 = q2 - q0, g = a2 - a1, nq = cross(a1, a2)
DRT_DEV TriOverlapQuery tri_overlap_query(const TriOverlapVerts &t) {
    TriOverlapQuery q;
    q.q0 = t.q0; q.a1 = t.q1 - t.q0; q.a2 = t.q2 - t.q0;
    q.g = q.a2 - q.a1; q.nq = cross(q.a1, q.a2);
    return q;
}

// one axis L: sq = (0, dot(L, a1), dot(L, a2)), st = (dot(L, p0), dot(L, p1), dot(L, p2)); ok iff min3(st) <= max3(sq) &&
// min3(sq) <= max3(st)
DRT_DEV bool tri_overlap_axis(f3 L, f3 a1, f3 a2, f3 p0, f3 p1, f3 p2) {
    const float q1 = dot(L, a1), q2 = dot(L, a2);
    const float t0 = dot(L, p0), t1 = dot(L, p1), t2 = dot(L, p2);
    return overlap_min3(t0, t1, t2) <= overlap_max3(0.f, q1, q2) && overlap_min3(0.f, q1, q2) <= overlap_max3(t0, t1, t2);
}

// drt.h "triangle test": the seventeen axes on the query and the stored (v0, e1, e2), relative to q0; listed iff none separates.
// Only the predicate leaves, so the order is free: the two normals come first and end most pairs whose bounds meet, then the nine
// cross products, then the six in-plane edge normals, which only a coplanar pair needs.  Within a group the axes are combined with &
// and the group ends with one branch: seventeen nested exits cost SGPR spills for the saved exec masks (kernel_tri_overlap.hip).
DRT_DEV bool tri_overlap_triangle(const TriOverlapQuery &q, f3 v0, f3 e1, f3 e2) {
    const f3 h = e2 - e1;
    const f3 p0 = v0 - q.q0, p1 = p0 + e1, p2 = p0 + e2;
    const f3 nt = cross(e1, e2);
    bool ok = tri_overlap_axis(q.nq, q.a1, q.a2, p0, p1, p2) & tri_overlap_axis(nt, q.a1, q.a2, p0, p1, p2);
    if (!ok) return false;
    const f3 A[3] = {q.a1, q.g, q.a2}, E[3] = {e1, h, e2};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) ok &= tri_overlap_axis(cross(A[i], E[j]), q.a1, q.a2, p0, p1, p2);
    if (!ok) return false;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        ok &= tri_overlap_axis(cross(q.nq, A[i]), q.a1, q.a2, p0, p1, p2);
        ok &= tri_overlap_axis(cross(nt, E[i]), q.a1, q.a2, p0, p1, p2);
    }
    return ok;
}
#endif

}  // namespace drt
