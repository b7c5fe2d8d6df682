// intersect.hpp -- launch seam of kernel_intersect.hip (triangle intersection segments, where each query triangle cuts the mesh:
// include/drt.h drt_renderer_intersect_triangles), and the query's routines: the two plane classifications and the segment of one
// pair.  The load of a drt_tri, its validity and bounds are tri_overlap.hpp's, the node cull is overlap.hpp's overlap_cull_passes and
// the cut point is section.hpp's section_cut, all unchanged.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_scene.hpp"
#ifdef __HIP__
#include "device_math.hpp"
#endif
#include "overlap.hpp"
#include "ray_query.hpp"
#include "section.hpp"
#include "tri_overlap.hpp"

namespace drt {

// The grid, the claim heads and the HBM stack are the occlusion ray query's (ray_query.hpp), as tri_overlap.hpp's are.
struct IntersectArgs {
    const void *tris;            // drt_tri[n] (48 B, 16-B aligned)
    const uint32_t *offsets;     // n + 1 words: query i owns out[offsets[i] .. offsets[i + 1]), clamped to out_capacity
    void *out;                   // drt_isect[out_capacity] (32 B, 16-B aligned); null when out_capacity == 0
    uint32_t *counts;            // n words or null: every record of the query, stored or not
    uint32_t out_capacity;
    QueryFrame frame;            // n, tree depth, refill threshold, claim heads, HBM stack: 4 B stack entries
};

// The launch bounds and the workgroups per CU of the two instantiations' grids (kernel_intersect.hip's header says how they were
// chosen): the count pass fits the 64 VGPRs of the other queries' 8 waves per SIMD, the fill needs 80.  The HBM stack of
// ray_query_max_blocks workgroups holds either.
constexpr int kIntersectCountWavesPerSimd = 8;
constexpr int kIntersectFillWavesPerSimd = 6;
static_assert(kIntersectCountWavesPerSimd <= kRqWavesPerSimd && kIntersectFillWavesPerSimd <= kRqWavesPerSimd,
              "the HBM stack is sized for kRqWavesPerSimd workgroups per CU");

// out_capacity == 0 launches the count-only instantiation, which reads no offsets and stores no record
hipError_t launch_intersect(const SceneView &scene, const IntersectArgs &args, int num_cus, hipStream_t stream);

#ifdef __HIP__                                      // device code: the .hip translation units only
// A query as the lane keeps it while it owns it: its three vertices and nq = cross(q1 - q0, q2 - q0)
struct IntersectQuery { f3 q0, q1, q2, nq; };
DRT_DEV IntersectQuery intersect_query(const TriOverlapVerts &t) {
    IntersectQuery q;
    q.q0 = t.q0; q.q1 = t.q1; q.q2 = t.q2;
    q.nq = cross(t.q1 - t.q0, t.q2 - t.q0);
    return q;
}

// the classes (s >= 0: above) of three signed values are not all the same
DRT_DEV bool intersect_split(float s0, float s1, float s2) {
    const bool a0 = s0 >= 0.f, a1 = s1 >= 0.f, a2 = s2 >= 0.f;
    return a0 != a1 || a1 != a2;
}

DRT_DEV float intersect_on(int j, f3 p) { return j == 0 ? p.x : (j == 1 ? p.y : p.z); }

// drt.h "cut points" of one triangle (w0, w1, w2) with signed values (s0, s1, s2) whose classes are not all the same: the apex k is
// the vertex alone in its class, X1 = cut(k, k+1) lies on edge k, X2 = cut(k, k+2) on edge (k+2) % 3.  Compares and selects only: an
// indexed array would go through scratch.
struct IntersectCuts { f3 x1, x2; int e1, e2; };
DRT_DEV IntersectCuts intersect_cuts(f3 w0, f3 w1, f3 w2, float s0, float s1, float s2) {
    const bool a0 = s0 >= 0.f, a1 = s1 >= 0.f, a2 = s2 >= 0.f;
    const int k = a1 == a2 ? 0 : (a0 == a2 ? 1 : 2);
    const bool k0 = k == 0, k1 = k == 1;
    const f3 vk = section_pick(k0, w0, section_pick(k1, w1, w2)), va = section_pick(k0, w1, section_pick(k1, w2, w0)),
             vb = section_pick(k0, w2, section_pick(k1, w0, w1));
    const float sk = k0 ? s0 : (k1 ? s1 : s2), sa = k0 ? s1 : (k1 ? s2 : s0), sb = k0 ? s2 : (k1 ? s0 : s1);
    const bool above = sk >= 0.f;
    IntersectCuts c;
    // lo is the below one of the two and hi the above one: the apex is hi when it is above
    c.x1 = section_cut(section_pick(above, va, vk), above ? sa : sk, section_pick(above, vk, va), above ? sk : sa);
    c.x2 = section_cut(section_pick(above, vb, vk), above ? sb : sk, section_pick(above, vk, vb), above ? sk : sb);
    c.e1 = k; c.e2 = k0 ? 2 : k - 1;
    return c;
}

// drt.h "signed values" to "record" for the query and the stored (v0, e1, e2): false = no record; true = the record's two 16-byte
// words (p, prim), (q, code).  The two classifications come first: they end most pairs whose bounds meet.
DRT_DEV bool intersect_segment(const IntersectQuery &q, f3 v0, f3 e1, f3 e2, int prim, float4 &r0, float4 &r1) {
    const f3 w1 = v0 + e1, w2 = v0 + e2;                                      // the world vertices; w0 = v0
    // the scene triangle against the query's plane: p_k = w_k - q0, s_k = dot(nq, p_k)
    const float s0 = dot(q.nq, v0 - q.q0), s1 = dot(q.nq, w1 - q.q0), s2 = dot(q.nq, w2 - q.q0);
    if (!intersect_split(s0, s1, s2)) return false;
    // the query against the scene triangle's plane: nt = cross(e1, e2), r_k = q_k - v0, u_k = dot(nt, r_k)
    const f3 nt = cross(e1, e2);
    const float u0 = dot(nt, q.q0 - v0), u1 = dot(nt, q.q1 - v0), u2 = dot(nt, q.q2 - v0);
    if (!intersect_split(u0, u1, u2)) return false;
    // line direction D = cross(nq, nt) and its largest axis j; no record unless fabsf(D[j]) > 0
    const f3 D = cross(q.nq, nt);
    int j = 0;
    if (fabsf(D.y) > fabsf(D.x)) j = 1;
    if (fabsf(D.z) > fabsf(intersect_on(j, D))) j = 2;
    const float Dj = intersect_on(j, D);
    if (!(fabsf(Dj) > 0.f)) return false;
    // cut points: the scene's carry its edge 0..2, the query's 4 + its edge
    const IntersectCuts T = intersect_cuts(v0, w1, w2, s0, s1, s2), Q = intersect_cuts(q.q0, q.q1, q.q2, u0, u1, u2);
    // intervals on axis j: (tl, th) = (T1, T2) if T1[j] <= T2[j], else (T2, T1); (ql, qh) likewise
    const bool tf = intersect_on(j, T.x1) <= intersect_on(j, T.x2), qf = intersect_on(j, Q.x1) <= intersect_on(j, Q.x2);
    const f3 tl = section_pick(tf, T.x1, T.x2), th = section_pick(tf, T.x2, T.x1);
    const f3 ql = section_pick(qf, Q.x1, Q.x2), qh = section_pick(qf, Q.x2, Q.x1);
    const int ctl = tf ? T.e1 : T.e2, cth = tf ? T.e2 : T.e1, cql = 4 + (qf ? Q.e1 : Q.e2), cqh = 4 + (qf ? Q.e2 : Q.e1);
    // lo = ql if ql[j] > tl[j] else tl; hi = qh if qh[j] < th[j] else th: on a tie the scene's point is kept
    const bool ul = intersect_on(j, ql) > intersect_on(j, tl), uh = intersect_on(j, qh) < intersect_on(j, th);
    const f3 lo = section_pick(ul, ql, tl), hi = section_pick(uh, qh, th);
    const int clo = ul ? cql : ctl, chi = uh ? cqh : cth;
    if (!(intersect_on(j, lo) <= intersect_on(j, hi))) return false;          // touching counts; a NaN fails
    // orientation: D[j] > 0: p = lo, q = hi; otherwise p = hi, q = lo
    const bool fwd = Dj > 0.f;
    const f3 p = section_pick(fwd, lo, hi), e = section_pick(fwd, hi, lo);
    const int cp = fwd ? clo : chi, cq = fwd ? chi : clo;
    r0 = make_float4(p.x, p.y, p.z, __int_as_float(prim));
    r1 = make_float4(e.x, e.y, e.z, __int_as_float(cp + 16 * cq));
    return true;
}
#endif

}  // namespace drt
