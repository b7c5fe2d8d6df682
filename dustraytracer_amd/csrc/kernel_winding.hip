// kernel_winding.hip -- generalised winding numbers for gfx950: w(q) = the sum over the triangles of the signed solid angle each
// subtends at q, over 4 pi, evaluated on the renderer's tree with one dipole term for a subtree that is far from the point
// (Barill et al. 2018, first order).  drt_renderer_winding_numbers / _winding_inside / _winding_signed_distance.  The reference has no
// such query; include/drt.h states the rule, and every line below that computes a value cites the part of it that it implements.
//
//   triangle   a = v0 - q, b = a + e1, c = a + e2, det = dot(a, cross(e1, e2)); 0 if det == 0, else 2 atan2(det, den) with the
//              project's own atan2 (winding.hpp restates both)
//   moment     per node {N, r2, p}: N = sum of 0.5 cross(e1, e2), p = the area-weighted centroid or the box centre, r2 = the squared
//              distance from p to the farthest corner of the node's stored box; a leaf sums its triangles in ascending index, a parent
//              is child 1 + child 2 for N, the area and the weighted sum
//   walk       depth-first from the root, child 1 first; d = p - q; a node is replaced by dot(d, N) / (dot(d, d) * sqrtf(dot(d, d)))
//              iff dot(d, d) > beta^2 r2; else an interior node is descended and a leaf adds its triangles in ascending index; one fp32
//              accumulator in steradians, in visit order; w = accumulator * (1 / (4 pi)) once, at the end
//
// The evaluation's grid, claim and stack: query_frame.hpp.  One point per lane, every trip of a wave's loop pops one node or adds
// one triangle per lane; stack entries ref, kRqLdsLevelsOccluded levels in LDS.  A result depends only on its point, the scene
// and beta: no float atomics, no cross-lane sums.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "device_scene.hpp"
#include "device_access.hpp"
#include "winding.hpp"
#include "query_frame.hpp"

namespace drt {

namespace {

// where a node reference's moment lies: interior nodes at their record index, leaf l at n_inner + l
DRT_DEV uint32_t moment_index(const SceneView &sc, uint32_t ref) { return (ref & kLeafBit) ? sc.n_inner + (ref & ~kLeafBit) : ref; }

// ------------------------------------------------------------------ the moments
// The box the tree stores for a node and the node's own reference, from the refit plan's `dest`: the child slot of the parent's
// InnerNode, or the root box.
struct NodeSlot { f3 lo, hi; uint32_t ref; };
DRT_DEV NodeSlot node_slot(const SceneView &sc, uint32_t dest) {
    NodeSlot s;
    if (dest == kRefitRootDest) {
        s.lo = ld3(sc.root_min); s.hi = ld3(sc.root_max); s.ref = sc.root_ref;
    } else if ((dest >> 1) >= sc.n_inner) {                  // (a plan that does not belong to this tree: nothing is read or written)
        s.lo = s.hi = mk3(0.f, 0.f, 0.f); s.ref = kNoNode;
    } else {
        const ChildPair c = load_children(sc.inner, dest >> 1);
        const bool second = (dest & 1u) != 0;
        s.lo = second ? c.min2 : c.min1; s.hi = second ? c.max2 : c.max1; s.ref = second ? c.ref2 : c.ref1;
    }
    return s;
}

// drt.h "node moment": p = S / A, or the centre of the stored box if A is 0 or anything is not finite; r2 to the farthest corner
DRT_DEV void store_moment(const SceneView &sc, const WindingMomentArgs &a, const NodeSlot &slot, f3 N, f3 S, float A) {
    const uint32_t at = moment_index(sc, slot.ref);
    if (at >= sc.n_inner + sc.n_leaves) return;              // (a plan that does not belong to this tree writes nothing)
    const float inf = __builtin_inff();
    f3 p = S / A;
    const bool ok = A > 0.0f && A < inf && __builtin_fabsf(p.x) < inf && __builtin_fabsf(p.y) < inf && __builtin_fabsf(p.z) < inf;
    if (!ok) p = 0.5f * (slot.lo + slot.hi);
    const float dx = fmaxf(__builtin_fabsf(p.x - slot.lo.x), __builtin_fabsf(slot.hi.x - p.x));
    const float dy = fmaxf(__builtin_fabsf(p.y - slot.lo.y), __builtin_fabsf(slot.hi.y - p.y));
    const float dz = fmaxf(__builtin_fabsf(p.z - slot.lo.z), __builtin_fabsf(slot.hi.z - p.z));
    const float r2 = dx * dx + dy * dy + dz * dz;
    float4 *m = reinterpret_cast<float4 *>(a.moments + at);
    m[0] = make_float4(N.x, N.y, N.z, r2);
    m[1] = make_float4(p.x, p.y, p.z, 0.0f);
    a.sums[at] = make_float4(S.x, S.y, S.z, A);
}

DRT_DEV void leaf_moment(const SceneView &sc, const WindingMomentArgs &a, uint32_t i) {
    const RefitLeaf leaf = a.leaves[i];
    f3 N = mk3(0.f, 0.f, 0.f), S = mk3(0.f, 0.f, 0.f);
    float A = 0.f;
    for (int k = leaf.start; k < leaf.start + leaf.count; k++) {
        if ((uint32_t)k >= sc.n_tris) break;
        const TriTest t = load_tri(sc.tri_hot, k);
        const f3 n = 0.5f * cross(t.e1, t.e2);
        const float area = sqrtf(dot(n, n));
        const f3 c = t.v0 + (t.e1 + t.e2) / 3.0f;
        N = N + n;
        A = A + area;
        S = S + area * c;
    }
    store_moment(sc, a, node_slot(sc, leaf.dest), N, S, A);
}

DRT_DEV void inner_moment(const SceneView &sc, const WindingMomentArgs &a, uint32_t i) {
    const RefitInner nd = a.levels[i];
    const NodeSlot slot = node_slot(sc, nd.dest);
    if ((slot.ref & kLeafBit) || slot.ref >= sc.n_inner) return;
    const uint2 kids = *reinterpret_cast<const uint2 *>(reinterpret_cast<const float4 *>(sc.inner + slot.ref) + 3);
    const uint32_t i1 = moment_index(sc, kids.x), i2 = moment_index(sc, kids.y);
    if (i1 >= sc.n_inner + sc.n_leaves || i2 >= sc.n_inner + sc.n_leaves) return;
    const float4 n1 = reinterpret_cast<const float4 *>(a.moments + i1)[0], n2 = reinterpret_cast<const float4 *>(a.moments + i2)[0];
    const float4 s1 = a.sums[i1], s2 = a.sums[i2];
    store_moment(sc, a, slot, mk3(n1.x, n1.y, n1.z) + mk3(n2.x, n2.y, n2.z), mk3(s1.x, s1.y, s1.z) + mk3(s2.x, s2.y, s2.z), s1.w + s2.w);
}

__global__ __launch_bounds__(kWnThreads) void winding_moments_leaves(const SceneView sc, const WindingMomentArgs a) {
    const uint32_t i = blockIdx.x * kWnThreads + threadIdx.x;
    if (i < a.n_leaves) leaf_moment(sc, a, i);
}

__global__ __launch_bounds__(kWnThreads) void winding_moments_height(const SceneView sc, const WindingMomentArgs a, uint32_t begin, uint32_t end) {
    const uint32_t i = begin + blockIdx.x * kWnThreads + threadIdx.x;
    if (i < end) inner_moment(sc, a, i);
}

// One workgroup walks the heights from `first` up: what a height wrote is read by the next after the barrier.
struct WindingTop { uint32_t begin[kRqMaxLevels + 2]; uint32_t heights; };
__global__ __launch_bounds__(kWnTopThreads) void winding_moments_top(const SceneView sc, const WindingMomentArgs a, const WindingTop top) {
    for (uint32_t h = 0; h < top.heights; h++) {
        for (uint32_t i = top.begin[h] + threadIdx.x; i < top.begin[h + 1]; i += kWnTopThreads) inner_moment(sc, a, i);
        __threadfence();
        __syncthreads();
    }
}

// ------------------------------------------------------------------ the evaluation
template <int MODE>
__global__ __launch_bounds__(kRqThreads, kRqWavesPerSimd) void winding_kernel(const SceneView sc, const WindingArgs a) {
    constexpr int K = kRqLdsLevelsOccluded;
    __shared__ uint32_t s_ref[K][kRqThreads];
    const int tid = threadIdx.x;
    const uint32_t gthread = blockIdx.x * kRqThreads + tid;
    const StackLane st = {tid, gthread, gridDim.x * kRqThreads, a.frame.stack_levels, a.frame.stack_hbm};
    uint32_t shard = home_shard(gthread);
    int shards_empty = 0;

    int rid = -1;                                            // this lane's point, -1 = idle
    f3 q = mk3(0.f, 0.f, 0.f);
    float acc = 0.f;                                         // steradians, in visit order
    uint32_t sp = 0;
    int tri = 0, tri_end = 0;                                // the triangles of the leaf under way that are still to add

    auto store = [&](float w) {
        if (MODE == (int)WindingOut::number) reinterpret_cast<float *>(a.out)[(uint32_t)rid] = w;
        else if (MODE == (int)WindingOut::inside) reinterpret_cast<uint8_t *>(a.out)[(uint32_t)rid] = w >= a.threshold ? 1 : 0;
        else reinterpret_cast<float *>(a.out)[8 * (size_t)(uint32_t)rid + 7] = w >= a.threshold ? -1.0f : 1.0f;
    };

    for (;;) {
        // ---- refill: claim points for the idle lanes (wave-uniform) ----
        const uint64_t idle = __ballot(rid < 0);
        if (claim_due(shards_empty, idle, a.frame)) {
            const bool was_idle = rid < 0;
            const Claimed c = claim_take(shard, shards_empty, rid, idle, a.frame);
            shard = c.shard; shards_empty = c.shards_empty; rid = c.rid;
            if (was_idle && rid >= 0) {
                // a new point: one 16-byte load (drt_point = p, max_dist; max_dist is not used)
                const float4 p4 = reinterpret_cast<const float4 *>(a.points)[(uint32_t)rid];
                q = mk3(p4.x, p4.y, p4.z);
                acc = 0.f; sp = 0; tri = tri_end = 0;
                const float inf = __builtin_inff();
                if (!(__builtin_fabsf(q.x) < inf && __builtin_fabsf(q.y) < inf && __builtin_fabsf(q.z) < inf)) {
                    store(__builtin_nanf(""));                        // a NaN or an infinity answers NaN without walking
                    rid = -1;
                } else if (sc.root_ref != kNoNode) { s_ref[0][tid] = sc.root_ref; sp = 1; }
            }
        }
        if (claim_drained(shards_empty, rid)) break;

        // ---- one step per busy lane: the next triangle of the leaf under way, or the next node -- replaced by its dipole, descended,
        // or, a leaf, opened.  A leaf's triangles are steps of their own so that one lane's leaf does not hold the wave for its whole
        // length; the order in which a lane adds is the visit order either way.
        if (rid >= 0 && tri < tri_end) {
            const TriTest t = load_tri(sc.tri_hot, tri);
            acc = acc + wn_solid_angle(q, t.v0, t.e1, t.e2);
            ++tri;
        } else if (rid >= 0 && sp > 0) {
            const uint32_t ref = stack_pop(s_ref, st, sp);
            const float4 *m = reinterpret_cast<const float4 *>(a.moments + moment_index(sc, ref));
            const float4 m0 = m[0], m1 = m[1];
            // what the node is, read next to its moment and not after the test: a leaf's range or an interior node's two references
            // (8 bytes either way), so that a step waits for memory once
            const bool is_leaf = (ref & kLeafBit) != 0;
            const uint2 what = is_leaf ? *reinterpret_cast<const uint2 *>(sc.leaves + (ref & ~kLeafBit))
                                       : *reinterpret_cast<const uint2 *>(reinterpret_cast<const float4 *>(sc.inner + ref) + 3);
            const f3 d = mk3(m1.x, m1.y, m1.z) - q;
            const float dd = dot(d, d);
            if (dd > a.beta2 * m0.w) {                                // (inf * 0 is a NaN: beta = inf never approximates)
                acc = acc + dot(d, mk3(m0.x, m0.y, m0.z)) / (dd * sqrtf(dd));
            } else if (is_leaf) {
                tri = (int)what.x; tri_end = tri + (int)what.y;      // LeafRange {start, count}: ascending index, from the next trip on
            } else {
                const uint2 kids = what;
                stack_push(s_ref, st, sp, kids.y, true);                        // child 2 first, so that child 1 is the next one popped
                stack_push(s_ref, st, sp, kids.x, true);
            }
        }

        // ---- a finished point: w = accumulator / (4 pi), one store ----
        if (rid >= 0 && sp == 0 && !(tri < tri_end)) {                // (rid < n: the claim never hands out more)
            store(acc * 0.0795774715f);
            rid = -1;
        }
    }
}

}  // namespace

hipError_t launch_winding_moments(const SceneView &sc, const WindingMomentArgs &a, const std::vector<uint32_t> &height_begin, hipStream_t stream) {
    if (a.n_leaves == 0) return hipSuccess;
    hipLaunchKernelGGL(winding_moments_leaves, dim3((a.n_leaves + kWnThreads - 1) / kWnThreads), dim3(kWnThreads), 0, stream, sc, a);
    const size_t heights = height_begin.empty() ? 0 : height_begin.size() - 1;
    // the first height from which on no height has more than kWnTopNodes nodes, and few enough heights for the argument
    size_t first_top = heights;
    while (first_top > 0 && height_begin[first_top] - height_begin[first_top - 1] <= (uint32_t)kWnTopNodes &&
           heights - (first_top - 1) <= (size_t)kRqMaxLevels + 1) first_top--;
    for (size_t h = 0; h < first_top; h++) {
        const uint32_t begin = height_begin[h], end = height_begin[h + 1];
        if (end > begin)
            hipLaunchKernelGGL(winding_moments_height, dim3((end - begin + kWnThreads - 1) / kWnThreads), dim3(kWnThreads), 0, stream, sc, a, begin, end);
    }
    if (first_top < heights) {
        WindingTop top;
        top.heights = (uint32_t)(heights - first_top);
        for (size_t h = first_top; h <= heights; h++) top.begin[h - first_top] = height_begin[h];
        hipLaunchKernelGGL(winding_moments_top, dim3(1), dim3(kWnTopThreads), 0, stream, sc, a, top);
    }
    return hipGetLastError();
}

hipError_t launch_winding(const SceneView &sc, WindingOut kind, const WindingArgs &args, int num_cus, hipStream_t stream) {
    if (args.frame.n == 0) return hipSuccess;
    const uint32_t blocks = query_blocks(args.frame.n, num_cus);
    if (kind == WindingOut::number) hipLaunchKernelGGL(winding_kernel<0>, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args);
    else if (kind == WindingOut::inside) hipLaunchKernelGGL(winding_kernel<1>, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args);
    else hipLaunchKernelGGL(winding_kernel<2>, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args);
    return hipGetLastError();
}

}  // namespace drt
