// tri_distance.hpp -- launch seam of kernel_tri_distance.hip (triangle distance queries, the mesh triangle nearest each query triangle:
// include/drt.h drt_renderer_triangle_distance), and the query's routines: the node bound, the clamped segment-segment closest points
// and the fifteen candidates of a pair.  The load of a drt_tri, its validity and bounds and the seventeen-axis predicate are
// tri_overlap.hpp's, the point-triangle routine is near_list.hpp's, both unchanged.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_scene.hpp"
#ifdef __HIP__
#include "device_math.hpp"
#endif
#include "near_list.hpp"
#include "overlap.hpp"
#include "ray_query.hpp"
#include "tri_overlap.hpp"

namespace drt {

// The grid, the claim heads and the HBM stack are the closest-hit ray query's (ray_query.hpp), as nearest.hpp's are: kRqShards heads,
// kRqLdsLevelsClosest stack levels {ref, box2} in LDS and the rest in ray_query_stack_bytes(num_cus, levels, false) bytes of HBM.
struct TriDistanceArgs {
    const void *tris;            // drt_tri[n] (48 B, 16-B aligned)
    const float *max_dist;       // n floats or null (= infinite)
    void *out;                   // drt_tri_near[n] (48 B, 16-B aligned)
    QueryFrame frame;            // n, tree depth, refill threshold, claim heads, HBM stack: 8 B stack entries
};

// The pair test keeps the query's 21 floats and two triangles' worth of edges and offsets live: 107 VGPRs, which do not fit the 96 of
// kTriOverlapWavesPerSimd waves per SIMD without scratch (DESIGN 5.27 has the table).  The kernel is bounded to this many, and its
// grid is this many workgroups per CU, which the HBM stack of ray_query_max_blocks workgroups holds.
constexpr int kTriDistanceWavesPerSimd = 4;
static_assert(kTriDistanceWavesPerSimd <= kRqWavesPerSimd, "the HBM stack is sized for kRqWavesPerSimd workgroups per CU");

// any_mode: DRT_TRIDIST_ANY (a query ends at the first pair within its distance) or DRT_TRIDIST_NEAREST
hipError_t launch_tri_distance(const SceneView &scene, bool any_mode, const TriDistanceArgs &args, int num_cus, hipStream_t stream);

#ifdef __HIP__                                      // device code: the .hip translation units only
// drt.h "node bound": nearest's box distance with the point replaced by the query's interval [qmin, qmax]
DRT_DEV float tri_distance_box2(f3 bmin, f3 bmax, f3 qmin, f3 qmax) {
    const float dx = fmaxf(fmaxf(bmin.x - qmax.x, 0.0f), qmin.x - bmax.x);
    const float dy = fmaxf(fmaxf(bmin.y - qmax.y, 0.0f), qmin.y - bmax.y);
    const float dz = fmaxf(fmaxf(bmin.z - qmax.z, 0.0f), qmin.z - bmax.z);
    return dx * dx + dy * dy + dz * dz;
}

// drt.h "clamp": fminf(fmaxf(x, 0), 1) + 0 -- the sum makes a zero result +0 whichever zero fmaxf(-0, 0) returns
DRT_DEV float tri_distance_clamp(float x) { return fminf(fmaxf(x, 0.0f), 1.0f) + 0.0f; }

// drt.h "edge pairs": the clamped closest points of the segments P1 + d1 s and P2 + d2 t (Ericson 5.1.9, exact-zero degenerate cases,
// no epsilon), s and t in [0, 1].  The cases are not blocks: every lane divides three times, the cases select the operands.
//   a <= 0 && e <= 0   s = t = 0
//   a <= 0             s = 0, t = clamp(f / e)
//   e <= 0             t = 0, s = clamp(-c / a)
//   otherwise          s = den > 0 ? clamp((b f - c e) / den) : 0, t = (b s + f) / e; t < 0: t = 0, s = clamp(-c / a);
//                      t > 1: t = 1, s = clamp((b - c) / a)
DRT_DEV float tri_distance_segments(f3 P1, f3 d1, f3 P2, f3 d2, float &s, float &t, f3 &c1, f3 &c2) {
    const f3 r = P1 - P2;
    const float a = dot(d1, d1), e = dot(d2, d2), f = dot(d2, r), c = dot(d1, r), b = dot(d1, d2);
    const float den = a * e - b * b;
    const bool a0 = a <= 0.0f, e0 = e <= 0.0f;
    const float s_gen = den > 0.0f ? tri_distance_clamp((b * f - c * e) / den) : 0.0f;
    // t of the general case, and of a <= 0 (f / e): one quotient over e
    const float t_q = (a0 ? f : b * s_gen + f) / e;
    const bool lo = t_q < 0.0f, hi = t_q > 1.0f;              // (a NaN is neither)
    // s of e <= 0 and of t < 0 (-c / a), and of t > 1 ((b - c) / a): one quotient over a
    const float s_q = tri_distance_clamp(((hi && !e0) ? b - c : -c) / a);
    s = (e0 || lo || hi) ? s_q : s_gen;
    t = e0 ? 0.0f : lo ? 0.0f : hi ? 1.0f : t_q;
    if (a0) { s = 0.0f; t = e0 ? 0.0f : tri_distance_clamp(t_q); }
    c1 = P1 + d1 * s; c2 = P2 + d2 * t;
    const f3 diff = c1 - c2;
    return dot(diff, diff);
}

// The three edges of a triangle (o, x, y) (origin and two edge vectors) as drt.h lists them: (o, x), (o + x, y - x), (o + y, -y)
DRT_DEV f3 tri_distance_neg(f3 a) { return mk3(-a.x, -a.y, -a.z); }

// drt.h "pair distance": the smallest of the fifteen candidates of the query (0, a1, a2) and the stored (v0, e1, e2), relative to q0, and
// its index: d2 = +inf, cand = 0, and candidate k replaces them iff its dist2 < d2 (strict: the first wins a tie, a NaN never wins).  The
// witness is recomputed from (prim, candidate) when the query ends (tri_distance_witness): the same operations on the same values.
DRT_DEV float tri_distance_candidates(const TriOverlapQuery &q, f3 v0, f3 e1, f3 e2, int &cand) {
    const f3 h = e2 - e1;
    const f3 p0 = v0 - q.q0, p1 = p0 + e1, p2 = p0 + e2;
    const f3 zero = mk3(0.f, 0.f, 0.f);
    float best = __builtin_inff(), u, v;
    cand = 0;
    // 0..2: the query's vertices against the scene triangle
    const f3 Q[3] = {zero, q.a1, q.a2};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float d = near_closest_on_triangle(Q[k], p0, e1, e2, u, v);
        if (d < best) { best = d; cand = k; }
    }
    // 3..5: the scene triangle's vertices against the query triangle
    const f3 P[3] = {p0, p1, p2};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float d = near_closest_on_triangle(P[k], zero, q.a1, q.a2, u, v);
        if (d < best) { best = d; cand = 3 + k; }
    }
    // 6..14: query edge i against scene edge j.  The loop stays rolled, and the edges are selected, not indexed: unrolled, the nine
    // tests keep 142 VGPRs live and spill under the 128 of four waves per SIMD; an indexed array would live in scratch.
#pragma unroll 1
    for (int ij = 0; ij < 9; ij++) {
        const int i = ij / 3, j = ij - 3 * i;
        const f3 Q1 = i == 0 ? zero : i == 1 ? q.a1 : q.a2, D1 = i == 0 ? q.a1 : i == 1 ? q.g : tri_distance_neg(q.a2);
        const f3 P2 = j == 0 ? p0 : j == 1 ? p1 : p2, D2 = j == 0 ? e1 : j == 1 ? h : tri_distance_neg(e2);
        float s, t;
        f3 c1, c2;
        const float d = tri_distance_segments(Q1, D1, P2, D2, s, t, c1, c2);
        if (d < best) { best = d; cand = 6 + ij; }
    }
    return best;
}

// drt.h "result": the witness points (relative to q0) and (u, v) of candidate `cand` of the pair, by the routine that made it
DRT_DEV void tri_distance_witness(const TriOverlapQuery &q, f3 v0, f3 e1, f3 e2, int cand, f3 &cq, f3 &ct, float &u, float &v) {
    const f3 h = e2 - e1;
    const f3 p0 = v0 - q.q0, p1 = p0 + e1, p2 = p0 + e2;
    const f3 zero = mk3(0.f, 0.f, 0.f);
    if (cand < 3) {
        cq = cand == 0 ? zero : cand == 1 ? q.a1 : q.a2;
        (void)near_closest_on_triangle(cq, p0, e1, e2, u, v);
        ct = (p0 + e1 * u) + e2 * v;
    } else if (cand < 6) {
        ct = cand == 3 ? p0 : cand == 4 ? p1 : p2;
        float uq, vq;
        (void)near_closest_on_triangle(ct, zero, q.a1, q.a2, uq, vq);
        cq = (zero + q.a1 * uq) + q.a2 * vq;
        u = cand == 4 ? 1.0f : 0.0f; v = cand == 5 ? 1.0f : 0.0f;       // the scene triangle's own vertex
    } else {
        const int i = (cand - 6) / 3, j = (cand - 6) % 3;
        const f3 Q1 = i == 0 ? zero : i == 1 ? q.a1 : q.a2, D1 = i == 0 ? q.a1 : i == 1 ? q.g : tri_distance_neg(q.a2);
        const f3 P2 = j == 0 ? p0 : j == 1 ? p1 : p2, D2 = j == 0 ? e1 : j == 1 ? h : tri_distance_neg(e2);
        float s, t;
        (void)tri_distance_segments(Q1, D1, P2, D2, s, t, cq, ct);
        // the point P2 + D2 t of scene edge j in the triangle's (u, v): (t, 0), (1 - t, t), (0, 1 - t)
        u = j == 0 ? t : j == 1 ? 1.0f - t : 0.0f;
        v = j == 0 ? 0.0f : j == 1 ? t : 1.0f - t;
    }
}
#endif

}  // namespace drt
