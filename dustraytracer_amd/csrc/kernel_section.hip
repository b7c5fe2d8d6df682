// kernel_section.hip -- plane sections for gfx950: the segments where each query plane cuts the mesh, one 32-byte record per cut triangle
// in ascending triangle index, the first cap_i of them stored in the plane's own segment of `out` (drt_renderer_plane_sections).  The
// reference has no such query; include/drt.h states the rule, and every line below that computes a value cites the part of it that it
// implements (the arithmetic itself is in section.hpp).
//
//   valid      all four words of the plane satisfy fabsf(x) <= FLT_MAX; an invalid plane pushes nothing and lists nothing
//   cull       cmin[j] = n[j] >= 0 ? bmin[j] : bmax[j], cmax[j] the other one; a box passes iff s(cmin) < 0 && s(cmax) >= 0, s(x) =
//              dot(n, x) - d.  The root is tested against the scene's root box.
//   cut        a triangle is cut iff the classes (s >= 0: above) of v0, v0 + e1, v0 + e2 are not all the same
//   record     apex k alone in its class, P = cut(k, k+1), Q = cut(k, k+2), P -> Q for an apex above and Q -> P below, code = k + 4 * above
//   segment    drt_renderer_overlap_boxes': cap = offsets[i+1] > offsets[i] ? the difference : 0, clamped so that offsets[i] + cap <=
//              out_capacity; slots 0 .. min(cap, total) - 1 the list, the rest of the cap slots the miss record; counts[i] = total.  Mode
//              ANY has no segment: the work ends at the first chunk of leaves with a cut triangle and counts[i] is 0 or 1.
//
// Shape: ONE WAVE PER PLANE on a persistent grid -- a plane's list is routinely longer than a leaf, and a batch is 10^2 to 10^4 planes, so
// one plane per lane (the shape of every other list kernel here) would leave the chip idle behind a few serial inserts.  Lane 0 claims the
// wave's next plane with one vector atomicAdd on one of the kRqShards sharded heads and broadcasts it.  No two waves exchange data, and
// the workgroup (4 waves) is only a packaging: there is no barrier and no LDS.
//
// Expansion, level-synchronous and order-preserving.  The wave owns two worklists of node references in HBM (2 * n_leaves words of
// SectionArgs::work) and alternates between them.  One step takes the current list in chunks of 64, one entry per lane: a leaf entry is
// carried over as it is, an interior entry loads its child-pair record, culls both children and emits 0, 1 or 2 references, child 1
// before child 2.  Two ballots ("emits at least one", "emits two") and the mbcnt of each give a lane its output position behind a
// wave-uniform running base, so the next list keeps the left-to-right order of the tree.  The steps end when a list holds leaves only:
// at most `depth` of them.  The entries of a list are roots of disjoint subtrees, so no list is longer than n_leaves; the stores are
// bounded by that all the same.
// A level is written by some lanes and read by others of the same wave: a workgroup-scope release / acquire fence pair stands between
// writing a list and reading it.
//
// Emission.  The final list is taken in chunks of 64 leaves, one leaf per lane: each lane tests its leaf's triangles in order and counts
// the cuts, a wave prefix sum of the counts gives each lane its base behind the wave-uniform total, and while that total is below the
// capacity the lane walks its leaf a second time and writes its records at base + j.  On the builder's trees the leaves of a list are
// ascending triangle ranges (the host checks it: section_leaves_ascending), so the records are in ascending triangle index without a
// sort or an insert.  After the last chunk the lanes stride over [min(total, cap), cap) with miss records and lane 0 writes the count.
// Only the owning wave touches a segment, with plain 16-byte vector stores.
//
// Registers: the compiler's resource remarks are recorded in DESIGN.md 5.22.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "device_scene.hpp"
#include "device_access.hpp"
#include "section.hpp"

namespace drt {

namespace {

// number of lanes below this one that are set in `mask` (v_mbcnt)
DRT_DEV uint32_t lanes_below(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// inclusive prefix sum over the 64 lanes of the wave
DRT_DEV uint32_t wave_inclusive_sum(uint32_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)v, d);
        if (lane >= d) v += up;
    }
    return v;
}

template <bool ANY>
__global__ __launch_bounds__(kSectionThreads, kSectionBoundWavesPerSimd) void section_kernel(const SceneView sc, const SectionArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * kSectionThreads + threadIdx.x) >> 6;
    if (wave >= a.waves) return;                              // (wave-uniform: the grid is whole workgroups)
    uint32_t *const list0 = a.work + (size_t)2 * a.list_words * wave, *const list1 = list0 + a.list_words;
    float4 *const out = reinterpret_cast<float4 *>(a.out);
    uint32_t shard = wave % kRqShards;                        // home shard of this wave; on to the next one when it is empty
    int shards_empty = 0;

    while (shards_empty < kRqShards) {
        // ---- claim: lane 0 takes the next plane of the shard, the wave hears of it ----
        const uint32_t s_begin = (uint32_t)((uint64_t)a.n * shard / kRqShards);
        const uint32_t s_len = (uint32_t)((uint64_t)a.n * (shard + 1) / kRqShards) - s_begin;
        uint32_t claimed = 0xFFFFFFFFu;
        if (lane == 0) {
            const uint32_t b = atomicAdd(a.heads + shard * kRqShardStride, 1u);
            if (b < s_len) claimed = s_begin + b;
        }
        const uint32_t rid = (uint32_t)__shfl((int)claimed, 0);
        if (rid >= a.n) { shard = (shard + 1) % kRqShards; shards_empty++; continue; }

        const SectionPlane pl = section_load_plane(a.planes, rid);
        uint32_t base = 0, cap = 0;                           // the plane's segment: out[base .. base + cap)
        if (!ANY) {
            // cap = offsets[i+1] > offsets[i] ? the difference : 0, clamped so that offsets[i] + cap <= out_capacity
            const uint32_t o0 = a.offsets[rid], o1 = a.offsets[rid + 1u];
            base = o0;
            cap = o1 > o0 ? o1 - o0 : 0u;
            const uint32_t room = o0 < a.out_capacity ? a.out_capacity - o0 : 0u;
            cap = cap < room ? cap : room;
        }

        // ---- expansion: from the root to a list of leaves, level by level ----
        uint32_t *cur = list0, *nxt = list1;
        uint32_t len = 0;
        bool inner_left = false;
        // an invalid plane pushes nothing; the root is tested against the scene's root box
        if (sc.root_ref != kNoNode && section_valid(pl) && section_cull_passes(pl, ld3(sc.root_min), ld3(sc.root_max))) {
            if (lane == 0) cur[0] = sc.root_ref;
            len = 1;
            inner_left = (sc.root_ref & kLeafBit) == 0u;
        }
        for (int level = 0; inner_left && level < kRqMaxLevels; level++) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");            // the list just written ...
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");            // ... is read by other lanes of this wave
            uint32_t n_out = 0;
            uint64_t inner_any = 0;
            for (uint32_t c = 0; c < len; c += 64u) {
                const uint32_t idx = c + (uint32_t)lane;
                uint32_t first = 0, second = 0, emits = 0;
                if (idx < len) {
                    const uint32_t ref = cur[idx];
                    if (ref & kLeafBit) { first = ref; emits = 1; }           // a leaf entry is carried over as it is
                    else if (ref < sc.n_inner) {
                        const ChildPair ch = load_children(sc.inner, ref);
                        const bool p1 = section_cull_passes(pl, ch.min1, ch.max1), p2 = section_cull_passes(pl, ch.min2, ch.max2);
                        emits = (p1 ? 1u : 0u) + (p2 ? 1u : 0u);
                        first = p1 ? ch.ref1 : ch.ref2;                       // child 1 before child 2
                        second = ch.ref2;
                    }
                }
                const uint64_t one = __ballot(emits >= 1u), two = __ballot(emits == 2u);
                const uint32_t pos = n_out + lanes_below(one) + lanes_below(two);
                if (emits >= 1u && pos < a.list_words) nxt[pos] = first;
                if (emits == 2u && pos + 1u < a.list_words) nxt[pos + 1u] = second;
                inner_any |= __ballot((emits >= 1u && !(first & kLeafBit)) || (emits == 2u && !(second & kLeafBit)));
                n_out += (uint32_t)__popcll(one) + (uint32_t)__popcll(two);
            }
            len = n_out < a.list_words ? n_out : a.list_words;
            inner_left = inner_any != 0;
            uint32_t *const t = cur; cur = nxt; nxt = t;
        }
        if (inner_left) len = 0;                               // (deeper than the 64 levels the entry point admits: nothing is listed)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

        // ---- emission: the leaves of the final list, 64 at a time, one per lane ----
        uint32_t total = 0;                                    // cut triangles so far (wave-uniform)
        for (uint32_t c = 0; c < len; c += 64u) {
            const uint32_t idx = c + (uint32_t)lane;
            int start = 0, count = 0;
            if (idx < len) {
                const uint32_t leaf_id = cur[idx] & ~kLeafBit;
                if (leaf_id < sc.n_leaves) { const LeafRange leaf = sc.leaves[leaf_id]; start = leaf.start; count = leaf.count; }
            }
            if (start < 0 || count < 0 || (uint32_t)start > sc.n_tris || (uint32_t)count > sc.n_tris - (uint32_t)start) count = 0;
            uint32_t cuts = 0;
            for (int i = start; i < start + count; i++) {
                const TriTest tri = load_tri(sc.tri_hot, i);
                cuts += section_test(pl, tri.v0, tri.e1, tri.e2).cut ? 1u : 0u;
            }
            const uint32_t incl = wave_inclusive_sum(cuts, lane);
            const uint32_t chunk_total = (uint32_t)__shfl((int)incl, 63);
            if (!ANY && total < cap && cuts != 0u) {           // the wave-uniform total is below the capacity: this chunk stores
                uint32_t slot = total + (incl - cuts);
                for (int i = start; i < start + count && slot < cap; i++) {
                    const TriTest tri = load_tri(sc.tri_hot, i);
                    const SectionTri t = section_test(pl, tri.v0, tri.e1, tri.e2);
                    if (!t.cut) continue;
                    float4 w0, w1;
                    section_record(t, i, w0, w1);
                    float4 *const rec = out + 2 * ((size_t)base + slot);
                    rec[0] = w0; rec[1] = w1;
                    slot++;
                }
            }
            total += chunk_total;
            if (ANY && total != 0u) break;                     // the work ends at the first chunk with a cut triangle
        }

        // ---- the miss record behind the list, and the count ----
        if (!ANY) {
            const float4 miss0 = make_float4(0.f, 0.f, 0.f, __int_as_float(-1)), miss1 = make_float4(0.f, 0.f, 0.f, 0.f);
            for (uint32_t j = (total < cap ? total : cap) + (uint32_t)lane; j < cap; j += 64u) {
                float4 *const rec = out + 2 * ((size_t)base + j);
                rec[0] = miss0; rec[1] = miss1;
            }
        }
        if (lane == 0 && a.counts) a.counts[rid] = ANY ? (total != 0u ? 1u : 0u) : total;
    }
}

}  // namespace

hipError_t launch_section(const SceneView &sc, bool any_mode, const SectionArgs &args, hipStream_t stream) {
    if (args.n == 0) return hipSuccess;
    const uint32_t blocks = (args.waves * 64u + kSectionThreads - 1) / kSectionThreads;
    if (any_mode) hipLaunchKernelGGL(section_kernel<true>, dim3(blocks), dim3(kSectionThreads), 0, stream, sc, args);
    else hipLaunchKernelGGL(section_kernel<false>, dim3(blocks), dim3(kSectionThreads), 0, stream, sc, args);
    return hipGetLastError();
}

}  // namespace drt
