// kernel_near_list.hip -- nearest-triangle lists for gfx950: the triangles within max_dist of a point, sorted by (d2, prim), the first
// cap_i of them stored in the point's own segment of `near` (drt_renderer_nearest_list).  The reference has no such query;
// include/drt.h states the rule, and every line below that computes a value cites the part of it that it implements.
//
//   listed     drt_renderer_nearest's closest point on the stored (v0, e1, e2) (near_list.hpp restates it); a triangle is listed iff
//              dist2 < r2 = max_dist * max_dist (a NaN never is).  No alpha test.  d2, u, v are nearest's bits for that pair.
//   bound      keep(box2) = (mode K && stored == cap) ? box2 <= tail.d2 : box2 < r2, at every pop and every push.  Mode GATHER never
//              shrinks it, so its set of listed triangles does not depend on the order; mode K's records are defined by this traversal.
//   traversal  nearest's: the root is pushed with its box2, a popped entry is dropped unless keep, a leaf's triangles in order, an
//              interior node pushes each child that passes keep, the farther one (b1 > b2 -> child 1) first
//   order      a before b iff a.d2 < b.d2 || (a.d2 == b.d2 && a.prim < b.prim)  (a listed d2 is never NaN)
//   segment    cap = offsets[i+1] > offsets[i] ? the difference : 0, clamped so that offsets[i] + cap <= near_capacity; slots
//              0 .. stored - 1 the list, the rest of the cap slots the miss record {r2, -1, 0, 0}; counts[i] = total (GATHER) or
//              stored (K); surf, when given, is written for the same slots when the point finishes
//
// Grid, claim and stack: query_frame.hpp.  One point per lane; stack entries {ref, box2}, kRqLdsLevelsClosest levels in LDS.
//
// The list: kernel_list_hits.hip's.  A point's segment in global memory IS its sorted list.  The lane keeps base, cap, stored, total
// and, once stored == cap, the key of the last stored record in registers, so a candidate that is not before the tail of a full list
// touches no memory -- and in mode K that same key is the search bound.  Any other candidate is inserted from the back: records move
// up by one slot (one 16-byte load, one 16-byte store each) while the candidate comes before them, and a full list drops its last
// record.  Only the owning lane reads or writes a segment, with plain vector loads and stores: no fences.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "device_scene.hpp"
#include "device_access.hpp"
#include "near_list.hpp"
#include "query_frame.hpp"

namespace drt {

namespace {

// the order of the list: ascending d2, equal d2 by ascending prim
DRT_DEV bool comes_before(float d2, int prim, float other_d2, int other_prim) {
    return d2 < other_d2 || (d2 == other_d2 && prim < other_prim);
}

template <bool KMODE>
__global__ __launch_bounds__(kRqThreads, kRqWavesPerSimd) void near_list_kernel(const SceneView sc, const NearListArgs a) {
    constexpr int K = kRqLdsLevelsClosest;
    __shared__ uint32_t s_ref[K][kRqThreads];
    __shared__ float s_box2[K][kRqThreads];
    const int tid = threadIdx.x;
    const uint32_t gthread = blockIdx.x * kRqThreads + tid;
    const StackLane st = {tid, gthread, gridDim.x * kRqThreads, a.frame.stack_levels, a.frame.stack_hbm};
    uint32_t shard = home_shard(gthread);
    int shards_empty = 0;
    float4 *const near = reinterpret_cast<float4 *>(a.near);

    int rid = -1;                                            // this lane's point, -1 = idle
    f3 p = mk3(0.f, 0.f, 0.f);
    float r2 = 0.f;                                          // max_dist * max_dist: the point's own product
    uint32_t base = 0, cap = 0;                              // the point's segment: near[base .. base + cap)
    uint32_t stored = 0, total = 0;                          // records in the segment (<= cap), listed triangles so far
    float tail_d2 = 0.f;                                     // key of near[base + cap - 1], valid once stored == cap
    int tail_prim = 0;
    uint32_t sp = 0;

    // drt.h "search bound": mode K's shrinks to the tail of a full list, <= so that an equal d2 with a smaller prim is still found
    auto keep = [&](float box2) { return (KMODE && stored == cap) ? box2 <= tail_d2 : box2 < r2; };

    for (;;) {
        // ---- refill: claim points for the idle lanes (wave-uniform) ----
        const uint64_t idle = __ballot(rid < 0);
        if (claim_due(shards_empty, idle, a.frame)) {
            const bool was_idle = rid < 0;
            const Claimed c = claim_take(shard, shards_empty, rid, idle, a.frame);
            shard = c.shard; shards_empty = c.shards_empty; rid = c.rid;
            if (was_idle && rid >= 0) {
                // a new point: one 16-byte load (drt_point = p, max_dist) and the two offsets that bound its segment
                const float4 q = reinterpret_cast<const float4 *>(a.points)[(uint32_t)rid];
                const uint32_t o0 = a.offsets[(uint32_t)rid], o1 = a.offsets[(uint32_t)rid + 1u];
                p = mk3(q.x, q.y, q.z);
                r2 = q.w * q.w;
                // cap = offsets[i+1] > offsets[i] ? the difference : 0, clamped so that offsets[i] + cap <= near_capacity
                base = o0;
                cap = o1 > o0 ? o1 - o0 : 0u;
                const uint32_t room = o0 < a.near_capacity ? a.near_capacity - o0 : 0u;
                cap = cap < room ? cap : room;
                stored = 0; total = 0; sp = 0;
                // the root goes on the stack with its box2: culled at its pop.  Mode K with no room visits nothing.
                if (sc.root_ref != kNoNode && !(KMODE && cap == 0u)) {
                    s_ref[0][tid] = sc.root_ref; s_box2[0][tid] = near_box_dist2(ld3(sc.root_min), ld3(sc.root_max), p); sp = 1;
                }
            }
        }
        if (claim_drained(shards_empty, rid)) break;

        // ---- one traversal step per busy lane ----
        if (rid >= 0 && sp > 0) {
            float box2;
            const uint32_t ref = stack_pop(s_ref, s_box2, st, sp, box2);
            if (keep(box2)) {
                if (ref & kLeafBit) {
                    const LeafRange leaf = sc.leaves[ref & ~kLeafBit];
                    for (int i = leaf.start; i < leaf.start + leaf.count; i++) {
                        const TriTest tri = load_tri(sc.tri_hot, i);
                        float u, v;
                        const float dist2 = near_closest_on_triangle(p, tri.v0, tri.e1, tri.e2, u, v);
                        if (!(dist2 < r2)) continue;                                        // listed iff dist2 < r2; NaN never
                        total++;
                        // no room at all, or a full list whose tail the candidate does not come before: nothing touches memory
                        if (cap == 0u || (stored == cap && !comes_before(dist2, i, tail_d2, tail_prim))) continue;
                        // the slot that opens: the next free one, or the last one of a full list (whose record is dropped)
                        uint32_t j = stored < cap ? stored++ : cap - 1u;
                        const bool is_tail = j == cap - 1u;                                 // what lands there is the new tail key
                        float new_tail_d2 = dist2;
                        int new_tail_prim = i;
                        bool moved = false;
                        float4 *const seg = near + (size_t)base;
                        while (j > 0u) {                                                    // j <= cap - 1: inside the segment
                            const float4 o = seg[j - 1u];
                            if (!comes_before(dist2, i, o.x, __float_as_int(o.y))) break;
                            seg[j] = o;
                            if (!moved) { new_tail_d2 = o.x; new_tail_prim = __float_as_int(o.y); moved = true; }
                            --j;
                        }
                        seg[j] = make_float4(dist2, __int_as_float(i), u, v);
                        if (is_tail) { tail_d2 = new_tail_d2; tail_prim = new_tail_prim; }
                    }
                } else {
                    const ChildPair c = load_children(sc.inner, ref);
                    const float b1 = near_box_dist2(c.min1, c.max1, p);
                    const float b2 = near_box_dist2(c.min2, c.max2, p);
                    const bool push1 = keep(b1), push2 = keep(b2);
                    push_far_first(s_ref, s_box2, st, sp, c.ref1, b1, push1, c.ref2, b2, push2);        // farther child first
                }
            }
        }

        // ---- a finished point: surf of its list, the miss records behind it, its count, and the lane is free ----
        if (rid >= 0 && sp == 0) {                                  // (rid < n: the claim never hands out more)
            if (a.surf) {
                float4 *const surf = reinterpret_cast<float4 *>(a.surf) + (size_t)base;
                for (uint32_t j = 0; j < stored; j++) {
                    // the point and the side are those of the stored (prim, u, v): nearest's operations on the same values
                    const float4 o = near[(size_t)base + j];
                    const int prim = __float_as_int(o.y);
                    const TriTest tri = load_tri(sc.tri_hot, prim);
                    const f3 c = (tri.v0 + tri.e1 * o.z) + tri.e2 * o.w;
                    const float side = dot(p - c, ld3(sc.tri_hot[prim].fn)) < 0.0f ? -1.0f : 1.0f;
                    surf[j] = make_float4(c.x, c.y, c.z, side);
                }
                for (uint32_t j = stored; j < cap; j++) surf[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            const float4 miss = make_float4(r2, __int_as_float(-1), 0.f, 0.f);            // the point's own product
            for (uint32_t j = stored; j < cap; j++) near[(size_t)base + j] = miss;
            if (a.counts) a.counts[(uint32_t)rid] = KMODE ? stored : total;
            rid = -1;
        }
    }
}

}  // namespace

hipError_t launch_near_list(const SceneView &sc, bool k_mode, const NearListArgs &args, int num_cus, hipStream_t stream) {
    if (args.frame.n == 0) return hipSuccess;
    const uint32_t blocks = query_blocks(args.frame.n, num_cus);
    if (k_mode) hipLaunchKernelGGL(near_list_kernel<true>, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args);
    else hipLaunchKernelGGL(near_list_kernel<false>, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args);
    return hipGetLastError();
}

}  // namespace drt
