// kernel_nearest.hip -- batched nearest-surface queries for gfx950: the closest point on the mesh for arrays of points
// (drt_renderer_nearest).  The reference has no such query; include/drt.h states the rule, and every line below that computes
// a value cites the part of it that it implements.
//
//   triangle   closest point on (v0, e1, e2) after Ericson, Real-Time Collision Detection 5.1.5: six dot products, three
//              cross terms, the first of seven cases that matches gives (u, v); c = (v0 + e1 u) + e2 v, dist2 = |p - c|^2
//   box        per axis d = max(max(bmin - p, 0), p - bmax), box2 = (dx dx + dy dy) + dz dz
//   traversal  best = max_dist^2; a popped entry is dropped unless box2 < best; a leaf's triangles in order, strict <; an
//              interior node pushes each child with box2 < best, the farther one (b1 > b2 -> child 1) first
//
// Grid, claim and stack: query_frame.hpp.  One point per lane; stack entries {ref, box2}, kRqLdsLevelsClosest levels in LDS.
//
// The seven cases are not seven blocks: all of them share the dot products, four of them are one quotient each, so the case chain
// selects the quotient's operands and then (u, v) -- one division per triangle, no divergence inside the test.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "device_scene.hpp"
#include "device_access.hpp"
#include "nearest.hpp"
#include "query_frame.hpp"

namespace drt {

namespace {

// drt.h "box distance": a NaN coordinate of p drops out of both max (v_max_f32 in IEEE mode), so its axis contributes 0
DRT_DEV float box_dist2(f3 bmin, f3 bmax, f3 p) {
    const float dx = fmaxf(fmaxf(bmin.x - p.x, 0.0f), p.x - bmax.x);
    const float dy = fmaxf(fmaxf(bmin.y - p.y, 0.0f), p.y - bmax.y);
    const float dz = fmaxf(fmaxf(bmin.z - p.z, 0.0f), p.z - bmax.z);
    return dx * dx + dy * dy + dz * dz;
}

// drt.h "per triangle": (u, v) of the closest point and its squared distance.  Cases 3, 5, 6 and 7 are each one quotient
// num / den of values all cases share; the chain below picks its operands with the cases' priority (3 before 5 before 6 before
// 7), divides once, and then picks (u, v) over all seven, last case first so that the first matching one wins.  A lane whose
// case does not use the quotient may have divided by zero: the value is not selected.
DRT_DEV float closest_on_triangle(f3 p, f3 v0, f3 e1, f3 e2, float &u, float &v) {
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

__global__ __launch_bounds__(kRqThreads, kRqWavesPerSimd) void nearest_kernel(const SceneView sc, const NearestArgs a) {
    constexpr int K = kRqLdsLevelsClosest;
    __shared__ uint32_t s_ref[K][kRqThreads];
    __shared__ float s_box2[K][kRqThreads];
    const int tid = threadIdx.x;
    const uint32_t gthread = blockIdx.x * kRqThreads + tid;
    const StackLane st = {tid, gthread, gridDim.x * kRqThreads, a.frame.stack_levels, a.frame.stack_hbm};
    uint32_t shard = home_shard(gthread);
    int shards_empty = 0;

    int rid = -1;                                            // this lane's point, -1 = idle
    f3 p = mk3(0.f, 0.f, 0.f);
    float best = 0.f, best_u = 0.f, best_v = 0.f;            // the nearest so far (prim -1 = none): best = its dist2, else max_dist^2
    int best_prim = -1;
    uint32_t sp = 0;

    for (;;) {
        // ---- refill: claim points for the idle lanes (wave-uniform) ----
        const uint64_t idle = __ballot(rid < 0);
        if (claim_due(shards_empty, idle, a.frame)) {
            const bool was_idle = rid < 0;
            const Claimed c = claim_take(shard, shards_empty, rid, idle, a.frame);
            shard = c.shard; shards_empty = c.shards_empty; rid = c.rid;
            if (was_idle && rid >= 0) {
                // a new point: one 16-byte load (drt_point = p, max_dist)
                const float4 q = reinterpret_cast<const float4 *>(a.points)[(uint32_t)rid];
                p = mk3(q.x, q.y, q.z);
                best = q.w * q.w; best_prim = -1; best_u = 0.f; best_v = 0.f;
                if (sc.root_ref != kNoNode) {                 // the root goes on the stack with its box2: culled at its pop
                    s_ref[0][tid] = sc.root_ref; s_box2[0][tid] = box_dist2(ld3(sc.root_min), ld3(sc.root_max), p); sp = 1;
                }
            }
        }
        if (claim_drained(shards_empty, rid)) break;

        // ---- one traversal step per busy lane ----
        if (rid >= 0 && sp > 0) {
            float box2;
            const uint32_t ref = stack_pop(s_ref, s_box2, st, sp, box2);
            if (box2 < best) {
                if (ref & kLeafBit) {
                    const LeafRange leaf = sc.leaves[ref & ~kLeafBit];
                    for (int i = leaf.start; i < leaf.start + leaf.count; i++) {
                        const TriTest tri = load_tri(sc.tri_hot, i);
                        float u, v;
                        const float dist2 = closest_on_triangle(p, tri.v0, tri.e1, tri.e2, u, v);
                        if (dist2 < best) { best = dist2; best_prim = i; best_u = u; best_v = v; }   // NaN never wins
                    }
                } else {
                    const ChildPair c = load_children(sc.inner, ref);
                    const float b1 = box_dist2(c.min1, c.max1, p);
                    const float b2 = box_dist2(c.min2, c.max2, p);
                    const bool push1 = b1 < best, push2 = b2 < best;
                    push_far_first(s_ref, s_box2, st, sp, c.ref1, b1, push1, c.ref2, b2, push2);        // farther child first
                }
            }
        }

        // ---- finished lanes write their result and go idle ----
        if (rid >= 0 && sp == 0) {                                  // (rid < n: the claim never hands out more)
            float4 o0 = make_float4(0.f, 0.f, 0.f, best), o1 = make_float4(__int_as_float(-1), 0.f, 0.f, 0.f);
            if (best_prim >= 0) {
                // the point and the side are those of the winning (prim, u, v): the same operations on the same values as the test
                const TriTest tri = load_tri(sc.tri_hot, best_prim);
                const f3 c = (tri.v0 + tri.e1 * best_u) + tri.e2 * best_v;
                const float side = dot(p - c, ld3(sc.tri_hot[best_prim].fn)) < 0.0f ? -1.0f : 1.0f;
                o0 = make_float4(c.x, c.y, c.z, best);
                o1 = make_float4(__int_as_float(best_prim), best_u, best_v, side);
            }
            float4 *out = reinterpret_cast<float4 *>(a.out) + 2 * (size_t)(uint32_t)rid;
            out[0] = o0; out[1] = o1;
            rid = -1; best_prim = -1;
        }
    }
}

}  // namespace

hipError_t launch_nearest(const SceneView &sc, const NearestArgs &args, int num_cus, hipStream_t stream) {
    if (args.frame.n == 0) return hipSuccess;
    const uint32_t blocks = query_blocks(args.frame.n, num_cus);
    hipLaunchKernelGGL(nearest_kernel, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args);
    return hipGetLastError();
}

}  // namespace drt
