// overlap.hpp -- launch seam of kernel_overlap.hip (box overlap queries, the triangles that touch each query box: include/drt.h
// drt_renderer_overlap_boxes), and the query's three routines: the world bounds of a box, the node cull and the triangle test.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_scene.hpp"
#ifdef __HIP__
#include "device_math.hpp"
#endif
#include "ray_query.hpp"

namespace drt {

// The grid, the claim heads and the HBM stack are the occlusion ray query's (ray_query.hpp), as list_hits.hpp's are: kRqThreads-thread
// workgroups, kRqWavesPerSimd waves per SIMD, kRqShards heads, kRqLdsLevelsOccluded stack levels of bare node references in LDS and
// the rest in ray_query_stack_bytes(num_cus, levels, true) bytes of HBM.
struct OverlapArgs {
    const void *boxes;           // drt_box[n] (64 B, 16-B aligned)
    const uint32_t *offsets;     // n + 1 words: box i owns prims[offsets[i] .. offsets[i + 1]), clamped to prims_capacity (LIST only)
    int32_t *prims;              // int32[prims_capacity]; null when prims_capacity == 0
    uint32_t *counts;            // n words or null: LIST every listed triangle of the box, ANY 0 or 1
    uint32_t prims_capacity;
    QueryFrame frame;            // n, tree depth, refill threshold, claim heads, HBM stack: 4 B stack entries
};

// any_mode: DRT_OVERLAP_ANY (the traversal ends at the first listed triangle) or DRT_OVERLAP_LIST
hipError_t launch_overlap(const SceneView &scene, bool any_mode, const OverlapArgs &args, int num_cus, hipStream_t stream);

#ifdef __HIP__                                      // device code: the .hip translation units only
// A drt_box as its four 16-byte words hold it: centre, half extents and the three axes as given
struct OverlapBox { f3 center, half, ax0, ax1, ax2; };
DRT_DEV OverlapBox overlap_load_box(const void *boxes, uint32_t i) {
    const float4 *q = reinterpret_cast<const float4 *>(boxes) + 4 * (size_t)i;
    const float4 a = q[0], b = q[1], c = q[2], d = q[3];                      // (d.w is the pad word: ignored)
    OverlapBox o;
    o.center = mk3(a.x, a.y, a.z); o.half = mk3(a.w, b.x, b.y);
    o.ax0 = mk3(b.z, b.w, c.x); o.ax1 = mk3(c.y, c.z, c.w); o.ax2 = mk3(d.x, d.y, d.z);
    return o;
}

// drt.h "world bounds of the query": ext[j] = (|axis[0][j]| half[0] + |axis[1][j]| half[1]) + |axis[2][j]| half[2]
DRT_DEV f3 overlap_extent(const OverlapBox &b) {
    return mk3((fabsf(b.ax0.x) * b.half.x + fabsf(b.ax1.x) * b.half.y) + fabsf(b.ax2.x) * b.half.z,
               (fabsf(b.ax0.y) * b.half.x + fabsf(b.ax1.y) * b.half.y) + fabsf(b.ax2.y) * b.half.z,
               (fabsf(b.ax0.z) * b.half.x + fabsf(b.ax1.z) * b.half.y) + fabsf(b.ax2.z) * b.half.z);
}

// drt.h "node cull": closed comparisons, no arithmetic on the node; a NaN bound fails
DRT_DEV bool overlap_cull_passes(f3 qmin, f3 qmax, f3 bmin, f3 bmax) {
    return qmin.x <= bmax.x && bmin.x <= qmax.x && qmin.y <= bmax.y && bmin.y <= qmax.y && qmin.z <= bmax.z && bmin.z <= qmax.z;
}

DRT_DEV float overlap_min3(float a, float b, float c) { return fminf(fminf(a, b), c); }
DRT_DEV float overlap_max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// one edge axis L = (la, lb) on the two box axes (m, n), m < n, that it does not vanish on: s_i = la p_i[m] + lb p_i[n],
// r = half[m] |la| + half[n] |lb|, ok iff min3(s) <= r && max3(s) >= -r
DRT_DEV bool overlap_edge_axis(float la, float lb, float hm, float hn, float p0m, float p0n, float p1m, float p1n, float p2m, float p2n) {
    const float s0 = la * p0m + lb * p0n, s1 = la * p1m + lb * p1n, s2 = la * p2m + lb * p2n;
    const float r = hm * fabsf(la) + hn * fabsf(lb);
    return overlap_min3(s0, s1, s2) <= r && overlap_max3(s0, s1, s2) >= -r;
}

// the three edge axes cross(unit_k, E) of one edge E, k = 0, 1, 2: (0, -E.z, E.y), (E.z, 0, -E.x), (-E.y, E.x, 0)
DRT_DEV bool overlap_edge(f3 E, f3 h, f3 p0, f3 p1, f3 p2) {
    return overlap_edge_axis(-E.z, E.y, h.y, h.z, p0.y, p0.z, p1.y, p1.z, p2.y, p2.z) &&
           overlap_edge_axis(E.z, -E.x, h.x, h.z, p0.x, p0.z, p1.x, p1.z, p2.x, p2.z) &&
           overlap_edge_axis(-E.y, E.x, h.x, h.y, p0.x, p0.y, p1.x, p1.y, p2.x, p2.y);
}

// drt.h "triangle test": Akenine-Moller's 13 separating axes in the box's frame on the stored (v0, e1, e2); listed iff none separates
DRT_DEV bool overlap_triangle(const OverlapBox &b, f3 v0, f3 e1, f3 e2) {
    const f3 a = v0 - b.center;
    const f3 p0 = mk3(dot(b.ax0, a), dot(b.ax1, a), dot(b.ax2, a));
    const f3 f1 = mk3(dot(b.ax0, e1), dot(b.ax1, e1), dot(b.ax2, e1));
    const f3 f2 = mk3(dot(b.ax0, e2), dot(b.ax1, e2), dot(b.ax2, e2));
    const f3 p1 = p0 + f1, p2 = p0 + f2, g = f2 - f1;
    const f3 h = b.half;
    // the three box axes
    bool ok = overlap_min3(p0.x, p1.x, p2.x) <= h.x && overlap_max3(p0.x, p1.x, p2.x) >= -h.x;
    ok = ok && overlap_min3(p0.y, p1.y, p2.y) <= h.y && overlap_max3(p0.y, p1.y, p2.y) >= -h.y;
    ok = ok && overlap_min3(p0.z, p1.z, p2.z) <= h.z && overlap_max3(p0.z, p1.z, p2.z) >= -h.z;
    // the triangle's plane
    const f3 n = cross(f1, f2);
    const float d = dot(n, p0);
    const float r = (fabsf(n.x) * h.x + fabsf(n.y) * h.y) + fabsf(n.z) * h.z;
    ok = ok && fabsf(d) <= r;
    // the nine edge axes, E = f1, g, f2
    return ok && overlap_edge(f1, h, p0, p1, p2) && overlap_edge(g, h, p0, p1, p2) && overlap_edge(f2, h, p0, p1, p2);
}
#endif

}  // namespace drt
