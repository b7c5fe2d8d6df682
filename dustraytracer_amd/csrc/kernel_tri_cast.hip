// kernel_tri_cast.hip -- triangle casts for gfx950: the first contact of a query triangle that translates along d with the mesh, its
// time, the contact point and normal (drt_renderer_triangle_cast).  The reference has no such query; include/drt.h states the rule,
// and every line below that computes a value cites the part of it that it implements (the arithmetic itself is in tri_cast.hpp and
// tri_overlap.hpp).
//
//   validity   tri_overlap.hpp's on the nine coordinates, and no NaN in d or tmax; an invalid cast pushes nothing: the miss record
//   extent     ext_lo[j] = min3(q0[j], q1[j], q2[j]) - q0[j], ext_hi likewise with max3, once per cast
//   node       the box [bmin - ext_hi, bmax - ext_lo] slab-tested with the ray (q0, inv_d): visited iff enter <= exit, exit >= 0,
//              enter <= best
//   pair       fifteen candidates relative to q0 -- 3 query vertices along d against the scene triangle, 3 scene vertices along -d
//              against the query triangle, 9 edge pairs -- the smallest tau is t; if the seventeen axes of the overlap predicate do
//              not separate the pair at the start, t = 0 and feature = candidate | 16
//   traversal  drt_renderer_sphere_cast's: best = tmax; a popped entry is dropped unless enter <= best; a leaf's triangles in order, a
//              pair wins on t < best or t == best with a smaller triangle index; an interior node pushes the farther child first.
//              Mode ANY ends the cast at the first pair with t < best.
//
// Grid, claim and stack: query_frame.hpp.  One cast per lane; stack entries {ref, enter}, kRqLdsLevelsClosest levels in LDS.
//
// Registers: a lane keeps q0, a1, a2, g, nq, d, inv_d and the two extents -- 27 floats -- and best, prim and feature for as long as it
// owns the cast; the contact is not kept but made again from (prim, candidate) when the cast ends.  The table of what was tried is in
// DESIGN 5.28; the bound is kTriCastWavesPerSimd waves per SIMD, and the grid is that many workgroups per CU.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "device_scene.hpp"
#include "device_access.hpp"
#include "tri_cast.hpp"
#include "query_frame.hpp"

namespace drt {

namespace {

template <bool ANY>
__global__ __launch_bounds__(kRqThreads, kTriCastWavesPerSimd) void tri_cast_kernel(const SceneView sc, const TriCastArgs a) {
    constexpr int K = kRqLdsLevelsClosest;
    __shared__ uint32_t s_ref[K][kRqThreads];
    __shared__ float s_enter[K][kRqThreads];
    const int tid = threadIdx.x;
    const uint32_t gthread = blockIdx.x * kRqThreads + tid;
    const StackLane st = {tid, gthread, gridDim.x * kRqThreads, a.frame.stack_levels, a.frame.stack_hbm};
    uint32_t shard = home_shard(gthread);
    int shards_empty = 0;

    int rid = -1;                                            // this lane's cast, -1 = idle
    f3 ext_lo = mk3(0.f, 0.f, 0.f), ext_hi = ext_lo;         // the query's bounds relative to q0
    f3 d = ext_lo, inv_d = ext_lo;
    TriOverlapQuery q = {};                                  // q0, a1, a2, g, nq: q0 is the ray's origin, a leaf's pair test reads the rest
    float best = 0.f;                                        // the first contact so far (prim -1 = none: best = tmax)
    int best_prim = -1, best_feature = -1;
    uint32_t sp = 0;

    for (;;) {
        // ---- refill: claim casts for the idle lanes (wave-uniform) ----
        const uint64_t idle = __ballot(rid < 0);
        if (claim_due(shards_empty, idle, a.frame)) {
            const bool was_idle = rid < 0;
            const Claimed c = claim_take(shard, shards_empty, rid, idle, a.frame);
            shard = c.shard; shards_empty = c.shards_empty; rid = c.rid;
            if (was_idle && rid >= 0) {
                // a new cast: three 16-byte loads (drt_tri) and one (drt_motion = d, tmax), its extent and edges
                const TriOverlapVerts t = tri_overlap_load(a.tris, (uint32_t)rid);
                const float4 m = reinterpret_cast<const float4 *>(a.motions)[(uint32_t)rid];
                ext_lo = tri_overlap_min(t) - t.q0; ext_hi = tri_overlap_max(t) - t.q0;   // (qmin - q0, qmax - q0)
                q = tri_overlap_query(t);
                d = mk3(m.x, m.y, m.z);
                inv_d = mk3(exact_rcp(d.x), exact_rcp(d.y), exact_rcp(d.z));
                best = m.w; best_prim = -1; best_feature = -1; sp = 0;
                // an invalid cast (a coordinate with fabsf(x) > FLT_MAX, a NaN in d or tmax) pushes nothing
                const bool valid = tri_overlap_valid(t) && d.x == d.x && d.y == d.y && d.z == d.z && best == best;
                if (valid && sc.root_ref != kNoNode) {
                    float enter;
                    if (tri_cast_slab(ld3(sc.root_min), ld3(sc.root_max), ext_lo, ext_hi, q.q0, inv_d, best, enter)) {
                        s_ref[0][tid] = sc.root_ref; s_enter[0][tid] = enter; sp = 1;
                    }
                }
            }
        }
        if (claim_drained(shards_empty, rid)) break;

        // ---- one traversal step per busy lane ----
        if (rid >= 0 && sp > 0) {
            float enter;
            const uint32_t ref = stack_pop(s_ref, s_enter, st, sp, enter);
            if (enter <= best) {
                if (ref & kLeafBit) {
                    const LeafRange leaf = sc.leaves[ref & ~kLeafBit];
                    for (int i = leaf.start; i < leaf.start + leaf.count; i++) {
                        const TriTest tri = load_tri(sc.tri_hot, i);
                        int feature;
                        float t = tri_cast_candidates(q, d, tri.v0, tri.e1, tri.e2, feature);
                        // the seventeen axes do not separate the pair at the start: it touches at t = 0, whatever the candidates say
                        if (tri_overlap_triangle(q, tri.v0, tri.e1, tri.e2)) { t = 0.0f; feature |= 16; }
                        if (t < best || (t == best && i < best_prim)) {                               // NaN never wins
                            const bool first = t < best;
                            best = t; best_prim = i; best_feature = feature;
                            if (ANY && first) { sp = 0; break; }                                      // mode ANY: the first pair with t < best
                        }
                    }
                } else {
                    const ChildPair c = load_children(sc.inner, ref);
                    float en1, en2;
                    const bool push1 = tri_cast_slab(c.min1, c.max1, ext_lo, ext_hi, q.q0, inv_d, best, en1);
                    const bool push2 = tri_cast_slab(c.min2, c.max2, ext_lo, ext_hi, q.q0, inv_d, best, en2);
                    push_far_first(s_ref, s_enter, st, sp, c.ref1, en1, push1, c.ref2, en2, push2);        // farther child first
                }
            }
        }

        // ---- finished lanes write their result and go idle ----
        if (rid >= 0 && sp == 0) {                                  // (rid < n: the claim never hands out more)
            // the miss record: zeros with t = tmax (best is still the motion's own word), prim = -1, feature = -1
            float4 o0 = make_float4(0.f, 0.f, 0.f, best), o1 = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
            float4 o2 = make_float4(0.f, 0.f, __int_as_float(-1), 0.f);
            if (best_prim >= 0) {
                o1.w = __int_as_float(best_prim); o2.z = __int_as_float(best_feature);
                if (!(best_feature & 16)) {
                    // the contact is that of the winning (prim, candidate): the same operations on the same values as the test.  A
                    // start overlap has no contact: point, normal, u and v stay zeros.
                    const TriTest tri = load_tri(sc.tri_hot, best_prim);
                    f3 ct, nrm;
                    float u, v;
                    tri_cast_contact(q, d, tri.v0, tri.e1, tri.e2, best_feature, ct, nrm, u, v);
                    const f3 p = q.q0 + ct;                          // point = q0 + c_scene
                    if (dot(nrm, d) > 0.0f) nrm = tri_cast_neg(nrm); // flipped against the motion
                    o0 = make_float4(p.x, p.y, p.z, best);
                    o1 = make_float4(nrm.x, nrm.y, nrm.z, __int_as_float(best_prim));
                    o2.x = u; o2.y = v;
                }
            }
            float4 *out = reinterpret_cast<float4 *>(a.out) + 3 * (size_t)(uint32_t)rid;
            out[0] = o0; out[1] = o1; out[2] = o2;
            rid = -1; best_prim = -1;
        }
    }
}

}  // namespace

hipError_t launch_tri_cast(const SceneView &sc, bool any_mode, const TriCastArgs &args, int num_cus, hipStream_t stream) {
    if (args.frame.n == 0) return hipSuccess;
    const uint32_t blocks = query_blocks(args.frame.n, num_cus, kTriCastWavesPerSimd);
    if (any_mode) hipLaunchKernelGGL(tri_cast_kernel<true>, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args);
    else hipLaunchKernelGGL(tri_cast_kernel<false>, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args);
    return hipGetLastError();
}

}  // namespace drt
