// tri_cast.hpp -- launch seam of kernel_tri_cast.hip (triangle casts, the first contact of a translating triangle with the mesh:
// include/drt.h drt_renderer_triangle_cast), and the query's routines: the widened slab test, the ray-triangle and edge-edge entry
// times and the fifteen candidates of a pair.  The load of a drt_tri, its validity and bounds and the seventeen-axis predicate are
// tri_overlap.hpp's, unchanged.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_scene.hpp"
#ifdef __HIP__
#include "device_math.hpp"
#endif
#include "overlap.hpp"
#include "ray_query.hpp"
#include "tri_overlap.hpp"

namespace drt {

// The grid, the claim heads and the HBM stack are the closest-hit ray query's (ray_query.hpp), as sphere_cast.hpp's are: kRqShards
// heads, kRqLdsLevelsClosest stack levels {ref, enter} in LDS and the rest in ray_query_stack_bytes(num_cus, levels, false) bytes of HBM.
struct TriCastArgs {
    const void *tris;            // drt_tri[n] (48 B, 16-B aligned)
    const void *motions;         // drt_motion[n] = {d[3], tmax} (16 B, 16-B aligned)
    void *out;                   // drt_tri_hit[n] (48 B, 16-B aligned)
    QueryFrame frame;            // n, tree depth, refill threshold, claim heads, HBM stack: 8 B stack entries
};

// A lane keeps the query's 15 floats, the motion's 6 (d, inv_d) and the 6 of its extent for as long as it owns the cast; with the pair
// test that does not fit the 96 VGPRs of five waves per SIMD without scratch (DESIGN 5.28 has the table).  The kernel is bounded to
// this many, and its grid is this many workgroups per CU, which the HBM stack of ray_query_max_blocks workgroups holds.
constexpr int kTriCastWavesPerSimd = 4;
static_assert(kTriCastWavesPerSimd <= kRqWavesPerSimd, "the HBM stack is sized for kRqWavesPerSimd workgroups per CU");

// any_mode: DRT_TRICAST_ANY (a cast ends at the first pair with t < best) or DRT_TRICAST_FIRST
hipError_t launch_tri_cast(const SceneView &scene, bool any_mode, const TriCastArgs &args, int num_cus, hipStream_t stream);

#ifdef __HIP__                                      // device code: the .hip translation units only
DRT_DEV f3 tri_cast_neg(f3 a) { return mk3(-a.x, -a.y, -a.z); }

// drt.h "traversal": the node's box widened by the query's extent, [bmin - ext_hi, bmax - ext_lo] with ext_hi = qmax - q0 and
// ext_lo = qmin - q0, against the ray (q0, inv_d); fminf / fmaxf drop a NaN operand (0 * inf)
DRT_DEV bool tri_cast_slab(f3 bmin, f3 bmax, f3 ext_lo, f3 ext_hi, f3 o, f3 inv_d, float best, float &enter) {
    const f3 t0 = ((bmin - ext_hi) - o) * inv_d;
    const f3 t1 = ((bmax - ext_lo) - o) * inv_d;
    const f3 lo = mk3(fminf(t0.x, t1.x), fminf(t0.y, t1.y), fminf(t0.z, t1.z));
    const f3 hi = mk3(fmaxf(t1.x, t0.x), fmaxf(t1.y, t0.y), fmaxf(t1.z, t0.z));
    enter = fmaxf(fmaxf(lo.x, lo.y), lo.z);
    const float exit = fminf(fminf(hi.x, hi.y), hi.z);
    return enter <= exit && exit >= 0.0f && enter <= best;
}

// The three numerators of a candidate over one determinant, each already multiplied by sg = det < 0 ? -1 : 1 (exact), and ad = |det|:
// every test is a comparison of a numerator with 0 or with ad, and a parameter is fabsf(numerator) / ad, one division, formed only
// where it is used.
struct TriCastSolve { float n1, n2, nt, ad; bool ok; };

// drt.h "vertex candidates": the ray (o, d) against the triangle (v0, e1, e2), Moller-Trumbore without an epsilon.  n1, n2 = u, v.
DRT_DEV TriCastSolve tri_cast_ray(f3 o, f3 d, f3 v0, f3 e1, f3 e2) {
    const f3 pv = cross(d, e2);
    const float det = dot(e1, pv);
    const f3 tv = o - v0;
    const f3 qv = cross(tv, e1);
    const float sg = det < 0.0f ? -1.0f : 1.0f;
    TriCastSolve r;
    r.ad = __builtin_fabsf(det);
    r.n1 = dot(tv, pv) * sg; r.n2 = dot(d, qv) * sg; r.nt = dot(e2, qv) * sg;
    r.ok = det != 0.0f && r.n1 >= 0.0f && r.n2 >= 0.0f && r.n1 + r.n2 <= r.ad && r.nt >= 0.0f;
    return r;
}

// drt.h "edge candidates": a + ea s + d tau = b + eb w by Cramer's rule on the columns (ea, d, -eb).  n1, n2 = s, w.
DRT_DEV TriCastSolve tri_cast_edges(f3 a, f3 ea, f3 b, f3 eb, f3 d) {
    const f3 nb = tri_cast_neg(eb);
    const f3 c = cross(d, nb);
    const float det = dot(ea, c);
    const f3 rr = b - a;
    const float sg = det < 0.0f ? -1.0f : 1.0f;
    TriCastSolve r;
    r.ad = __builtin_fabsf(det);
    r.n1 = dot(rr, c) * sg; r.nt = dot(ea, cross(rr, nb)) * sg; r.n2 = dot(ea, cross(d, rr)) * sg;
    r.ok = det != 0.0f && r.n1 >= 0.0f && r.n1 <= r.ad && r.n2 >= 0.0f && r.n2 <= r.ad && r.nt >= 0.0f;
    return r;
}

DRT_DEV float tri_cast_quot(float n, float ad) { return __builtin_fabsf(n) / ad; }

// drt.h "pair": the smallest tau of the fifteen candidates of the query (0, a1, a2) moving along d and the stored (v0, e1, e2), relative
// to q0, and its index: tau = +inf, cand = 15, and candidate k replaces them iff it passes its tests and its tau < the best (strict: the
// first wins a tie).  The contact is recomputed from (prim, candidate) when the cast ends (tri_cast_contact).
DRT_DEV float tri_cast_candidates(const TriOverlapQuery &q, f3 d, f3 v0, f3 e1, f3 e2, int &cand) {
    const f3 h = e2 - e1;
    const f3 p0 = v0 - q.q0, p1 = p0 + e1, p2 = p0 + e2;
    const f3 zero = mk3(0.f, 0.f, 0.f);
    const f3 md = tri_cast_neg(d);
    float best = __builtin_inff();
    cand = 15;
    // 0..2: the query's vertices along d against the scene triangle.  All three loops are unrolled: 106 VGPRs, still 4 waves per SIMD and
    // no scratch, and a quarter to a third faster than the rolled loops' 103 on an MI355X; the selects fold away.
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const TriCastSolve r = tri_cast_ray(k == 0 ? zero : k == 1 ? q.a1 : q.a2, d, p0, e1, e2);
        if (r.ok) {
            const float tau = tri_cast_quot(r.nt, r.ad);
            if (tau < best) { best = tau; cand = k; }
        }
    }
    // 3..5: the scene triangle's vertices along -d against the query triangle
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const TriCastSolve r = tri_cast_ray(k == 0 ? p0 : k == 1 ? p1 : p2, md, zero, q.a1, q.a2);
        if (r.ok) {
            const float tau = tri_cast_quot(r.nt, r.ad);
            if (tau < best) { best = tau; cand = 3 + k; }
        }
    }
    // 6..14: query edge i against scene edge j.  The edges are selected, not indexed (tri_distance.hpp's reason: an indexed array would
    // live in scratch); unlike there the nine tests unrolled fit the 128 VGPRs of four waves per SIMD.
#pragma unroll
    for (int ij = 0; ij < 9; ij++) {
        const int i = ij / 3, j = ij - 3 * i;
        const f3 A = i == 0 ? zero : i == 1 ? q.a1 : q.a2, EA = i == 0 ? q.a1 : i == 1 ? q.g : tri_cast_neg(q.a2);
        const f3 B = j == 0 ? p0 : j == 1 ? p1 : p2, EB = j == 0 ? e1 : j == 1 ? h : tri_cast_neg(e2);
        const TriCastSolve r = tri_cast_edges(A, EA, B, EB, d);
        if (r.ok) {
            const float tau = tri_cast_quot(r.nt, r.ad);
            if (tau < best) { best = tau; cand = 6 + ij; }
        }
    }
    return best;
}

// drt.h "result": the contact point on the scene triangle (relative to q0), its (u, v) and the unflipped normal of candidate `cand`
// (0..14) of the pair, by the routine that made it
DRT_DEV void tri_cast_contact(const TriOverlapQuery &q, f3 d, f3 v0, f3 e1, f3 e2, int cand, f3 &ct, f3 &nrm, float &u, float &v) {
    const f3 h = e2 - e1;
    const f3 p0 = v0 - q.q0, p1 = p0 + e1, p2 = p0 + e2;
    const f3 zero = mk3(0.f, 0.f, 0.f);
    if (cand < 3) {
        const TriCastSolve r = tri_cast_ray(cand == 0 ? zero : cand == 1 ? q.a1 : q.a2, d, p0, e1, e2);
        u = tri_cast_quot(r.n1, r.ad); v = tri_cast_quot(r.n2, r.ad);
        ct = (p0 + e1 * u) + e2 * v;
        nrm = cross(e1, e2);
    } else if (cand < 6) {
        ct = cand == 3 ? p0 : cand == 4 ? p1 : p2;                          // the scene triangle's own vertex
        u = cand == 4 ? 1.0f : 0.0f; v = cand == 5 ? 1.0f : 0.0f;
        nrm = q.nq;
    } else {
        const int i = (cand - 6) / 3, j = (cand - 6) % 3;
        const f3 A = i == 0 ? zero : i == 1 ? q.a1 : q.a2, EA = i == 0 ? q.a1 : i == 1 ? q.g : tri_cast_neg(q.a2);
        const f3 B = j == 0 ? p0 : j == 1 ? p1 : p2, EB = j == 0 ? e1 : j == 1 ? h : tri_cast_neg(e2);
        const TriCastSolve r = tri_cast_edges(A, EA, B, EB, d);
        const float w = tri_cast_quot(r.n2, r.ad);
        ct = B + EB * w;
        // the point B + EB w of scene edge j in the triangle's (u, v): (w, 0), (1 - w, w), (0, 1 - w)
        u = j == 0 ? w : j == 1 ? 1.0f - w : 0.0f;
        v = j == 0 ? 0.0f : j == 1 ? w : 1.0f - w;
        nrm = cross(EA, EB);
    }
}
#endif

}  // namespace drt
