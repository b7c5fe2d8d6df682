// kernel_list_hits.hip -- ordered hit lists for gfx950: the triangles a ray passes through, sorted by (t, prim), the first cap_i of them
// stored in the ray's own segment of `hits` (drt_renderer_list_hits).  The reference has no such query; include/drt.h states the
// rule, and every line below that computes a value cites the part of it that it implements.
//
//   listed     tri_intersect_flat's test on the stored (v0, e1, e2); a triangle is listed iff it hits, t > tmin and t < tmax.  No
//              alpha test.  t, u, v are the test's own values: drt_renderer_trace_rays' bits for that pair.
//   traversal  drt_renderer_crossings', unchanged: the root is skipped if d < 0 || d > tmax, a child is pushed iff
//              d >= 0 && !(d > tmax), the farther one first.  Each triangle lies in one leaf, so the SET of listed triangles does not
//              depend on the order, and the order below is total: neither does the list.
//   order      a before b iff a.t < b.t || (a.t == b.t && a.prim < b.prim)  (a listed t is > 1e-6, never NaN)
//   segment    cap = offsets[i+1] > offsets[i] ? the difference : 0, clamped so that offsets[i] + cap <= hits_capacity; slots
//              0 .. min(cap, total) - 1 the list, the rest of the cap slots the miss record {tmax, -1, 0, 0}; counts[i] = total
//
// Grid, claim and stack: query_frame.hpp.  One ray per lane; stack entries ref, kRqLdsLevelsOccluded levels in LDS.
//
// The list: a ray's segment in global memory IS its sorted list.  The lane keeps base, cap, stored, total and, once stored == cap, the
// key of the last stored record in registers, so a candidate that is not before the tail of a full list touches no memory.  Any other
// candidate is inserted from the back: records move up by one slot (one 16-byte load, one 16-byte store each) while the candidate
// comes before them, and a full list drops its last record.  With the farther child pushed first, hits mostly arrive in order and the
// insert is an append.  Only the owning lane reads or writes a segment, with plain vector loads and stores: no fences.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "device_scene.hpp"
#include "device_access.hpp"
#include "list_hits.hpp"
#include "query_frame.hpp"

namespace drt {

namespace {

// the order of the list: ascending t, equal t by ascending prim
DRT_DEV bool comes_before(float t, int prim, float other_t, int other_prim) {
    return t < other_t || (t == other_t && prim < other_prim);
}

__global__ __launch_bounds__(kRqThreads, kRqWavesPerSimd) void list_hits_kernel(const SceneView sc, const ListHitsArgs a) {
    constexpr int K = kRqLdsLevelsOccluded;
    __shared__ uint32_t s_ref[K][kRqThreads];
    const int tid = threadIdx.x;
    const uint32_t gthread = blockIdx.x * kRqThreads + tid;
    const StackLane st = {tid, gthread, gridDim.x * kRqThreads, a.frame.stack_levels, a.frame.stack_hbm};
    uint32_t shard = home_shard(gthread);
    int shards_empty = 0;
    float4 *const hits = reinterpret_cast<float4 *>(a.hits);

    int rid = -1;                                            // this lane's ray, -1 = idle
    Ray ray;
    float tmin = 0.f, tmax = 0.f;
    uint32_t base = 0, cap = 0;                              // the ray's segment: hits[base .. base + cap)
    uint32_t stored = 0, total = 0;                          // records in the segment (<= cap), listed triangles so far
    float tail_t = 0.f;                                      // key of hits[base + cap - 1], valid once stored == cap
    int tail_prim = 0;
    uint32_t sp = 0;

    for (;;) {
        // ---- refill: claim rays for the idle lanes (wave-uniform) ----
        const uint64_t idle = __ballot(rid < 0);
        if (claim_due(shards_empty, idle, a.frame)) {
            const bool was_idle = rid < 0;
            const Claimed c = claim_take(shard, shards_empty, rid, idle, a.frame);
            shard = c.shard; shards_empty = c.shards_empty; rid = c.rid;
            if (was_idle && rid >= 0) {
                // a new ray: two 16-byte loads (drt_ray = org, tmin, dir, tmax) and the two offsets that bound its segment
                const float4 *r = reinterpret_cast<const float4 *>(a.rays) + 2 * (size_t)(uint32_t)rid;
                const float4 o = r[0], d = r[1];
                const uint32_t o0 = a.offsets[(uint32_t)rid], o1 = a.offsets[(uint32_t)rid + 1u];
                tmin = o.w; tmax = d.w;
                ray = make_ray(mk3(o.x, o.y, o.z), mk3(d.x, d.y, d.z));
                // cap = offsets[i+1] > offsets[i] ? the difference : 0, clamped so that offsets[i] + cap <= hits_capacity
                base = o0;
                cap = o1 > o0 ? o1 - o0 : 0u;
                const uint32_t room = o0 < a.hits_capacity ? a.hits_capacity - o0 : 0u;
                cap = cap < room ? cap : room;
                stored = 0; total = 0; sp = 0;
                // the root goes on the stack unless d < 0 || d > tmax (crossings' root rule)
                if (sc.root_ref != kNoNode) {
                    const float droot = slab_intersect(ld3(sc.root_min), ld3(sc.root_max), ray);
                    if (!(droot < 0 || droot > tmax)) { s_ref[0][tid] = sc.root_ref; sp = 1; }
                }
            }
        }
        if (claim_drained(shards_empty, rid)) break;

        // ---- one traversal step per busy lane ----
        if (rid >= 0 && sp > 0) {
            const uint32_t ref = stack_pop(s_ref, st, sp);
            if (ref & kLeafBit) {
                const LeafRange leaf = sc.leaves[ref & ~kLeafBit];
                for (int i = leaf.start; i < leaf.start + leaf.count; i++) {
                    const TriTest tri = load_tri(sc.tri_hot, i);
                    float t, u, v;
                    const bool h = tri_intersect_flat(ray, tri.v0, tri.e1, tri.e2, t, u, v);
                    if (!(h && t > tmin && t < tmax)) continue;                         // listed iff hit, t > tmin, t < tmax
                    total++;
                    // no room at all, or a full list whose tail the candidate does not come before: nothing touches memory
                    if (cap == 0u || (stored == cap && !comes_before(t, i, tail_t, tail_prim))) continue;
                    // the slot that opens: the next free one, or the last one of a full list (whose record is dropped)
                    uint32_t j = stored < cap ? stored++ : cap - 1u;
                    const bool is_tail = j == cap - 1u;                                 // what lands there is the new tail key
                    float new_tail_t = t;
                    int new_tail_prim = i;
                    bool moved = false;
                    float4 *const seg = hits + (size_t)base;
                    while (j > 0u) {                                                    // j <= cap - 1: inside the segment
                        const float4 p = seg[j - 1u];
                        if (!comes_before(t, i, p.x, __float_as_int(p.y))) break;
                        seg[j] = p;
                        if (!moved) { new_tail_t = p.x; new_tail_prim = __float_as_int(p.y); moved = true; }
                        --j;
                    }
                    seg[j] = make_float4(t, __int_as_float(i), u, v);
                    if (is_tail) { tail_t = new_tail_t; tail_prim = new_tail_prim; }
                }
            } else {
                const ChildPair c = load_children(sc.inner, ref);
                const float d1 = slab_intersect(c.min1, c.max1, ray);
                const float d2 = slab_intersect(c.min2, c.max2, ray);
                const bool push1 = d1 >= 0 && !(d1 > tmax), push2 = d2 >= 0 && !(d2 > tmax);
                push_far_first(s_ref, st, sp, c.ref1, d1, push1, c.ref2, d2, push2);            // farther child first
            }
        }

        // ---- a finished ray: the miss records behind its list, its total, and the lane is free ----
        if (rid >= 0 && sp == 0) {                                  // (rid < n: the claim never hands out more)
            const float4 miss = make_float4(tmax, __int_as_float(-1), 0.f, 0.f);          // the ray's own tmax word
            for (uint32_t j = stored; j < cap; j++) hits[(size_t)base + j] = miss;
            if (a.counts) a.counts[(uint32_t)rid] = total;
            rid = -1;
        }
    }
}

}  // namespace

hipError_t launch_list_hits(const SceneView &sc, const ListHitsArgs &args, int num_cus, hipStream_t stream) {
    if (args.frame.n == 0) return hipSuccess;
    const uint32_t blocks = query_blocks(args.frame.n, num_cus);
    hipLaunchKernelGGL(list_hits_kernel, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args);
    return hipGetLastError();
}

}  // namespace drt
