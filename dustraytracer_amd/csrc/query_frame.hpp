// query_frame.hpp -- what every batched query kernel shares (ray_query, radiance, nearest, crossings, list_hits, sphere_cast,
// near_list, overlap, tri_overlap, intersect, tri_distance, tri_cast, winding): the claim that deals queries to idle lanes, the
// two-tier traversal stack, and the launch size.  A kernel keeps what it alone knows -- the visit condition, the leaf loop, the
// child test, the result -- and its main loop reads: claim; if (new) { load, seed }; if (drained) break; pop; its own body; pushes;
// its own write-out.
//
// Grid: persistent, 8 workgroups of 256 threads per CU (= 8 waves per SIMD, fewer where a kernel's registers ask for it), one
// query per lane, "while-while with dynamic fetch" (Aila & Laine 2009): every trip of a wave's loop is one traversal step (one
// node popped per busy lane).
// Claim: the n queries are split into kRqShards contiguous shards (shard_range), each with a head counter kRqShardStride words
// from the next.  Once at least `refill_min` lanes of a wave are idle (64 = the plain form: a wave takes new queries only when
// all are done), lane 0 claims that many with ONE atomicAdd on the wave's current shard, clips the claim to the shard, and the
// idle lanes take the claimed indices in lane order (ballot / mbcnt).  A shard that gives nothing sends the wave to the next one;
// after kRqShards empty answers the wave has seen them all.  A result depends only on its query and the scene: traversal order
// is per lane, the claim only decides who runs it.
// Stack: entry [level][thread] -- the bottom K levels in the kernel's LDS arrays (one bank per lane), the rest in a renderer-owned
// HBM array with the same coalesced layout, [(level - K) * grid threads + thread].  An entry is a 32-bit node reference, or
// {reference, float key} (8 bytes in HBM) where the kernel culls a node again at its pop.  `levels` is the tree depth: the stack
// never holds more entries, and a push beyond it is dropped.
#pragma once
#include "ray_query.hpp"
#if defined(__HIPCC__)
#include "device_math.hpp"        // DRT_DEV
#endif

namespace drt {

struct ShardRange { uint32_t begin, len; };
// shard `shard` of n queries: [n * shard / kRqShards, n * (shard + 1) / kRqShards) -- contiguous, disjoint, covering [0, n)
__host__ __device__ constexpr ShardRange shard_range(uint32_t n, uint32_t shard) {
    const uint32_t begin = (uint32_t)((uint64_t)n * shard / kRqShards);
    return ShardRange{begin, (uint32_t)((uint64_t)n * (shard + 1) / kRqShards) - begin};
}

// workgroups of a launch over n queries: one thread per query up to the resident grid, `waves` workgroups per CU and never more
// than ray_query_max_blocks, which sizes the HBM stack
inline uint32_t query_blocks(uint32_t n, int num_cus, int waves = kRqWavesPerSimd) {
    const uint32_t want = n / kRqThreads + (n % kRqThreads != 0 ? 1u : 0u);
    const uint32_t resident = (uint32_t)std::max(1, num_cus) * (uint32_t)waves;
    return std::min<uint32_t>(want, std::min<uint32_t>(resident, (uint32_t)ray_query_max_blocks(num_cus)));
}

#if defined(__HIPCC__)

// rank of this lane among the lanes set in `mask` (v_mbcnt): the claim hands queries to idle lanes in lane order
DRT_DEV int lane_rank(uint64_t mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// The claim's state is two plain locals of the kernel: `shard`, the shard this wave claims from (its home shard, then on to the next
// one when that is empty), and `shards_empty`, the empty answers so far (kRqShards of them = nothing is left anywhere).  The
// functions below take them, and the lane's rid, by value and hand the new values back: a local whose address goes to a helper is
// promoted to a register only after the helper is inlined, which reorders the loop's values and, in ray_query_kernel<occluded>,
// doubled the reloads of spilled SGPRs in the traversal step.
DRT_DEV uint32_t home_shard(uint32_t gthread) { return (gthread >> 6) % kRqShards; }

// The refill, in two halves so that the kernel's block nests under the wave-uniform test as it does under the lane's:
//     const uint64_t idle = __ballot(rid < 0);
//     if (claim_due(shards_empty, idle, frame)) {
//         const bool was_idle = rid < 0;
//         const Claimed c = claim_take(shard, shards_empty, rid, idle, frame);
//         shard = c.shard; shards_empty = c.shards_empty; rid = c.rid;
//         if (was_idle && rid >= 0) { load the query, seed the stack }
//     }
// due: enough lanes of the wave are idle and a shard may still hold queries; wave-uniform
DRT_DEV bool claim_due(int shards_empty, uint64_t idle, const QueryFrame &f) {
    const uint32_t n_idle = (uint32_t)__popcll(idle);
    return shards_empty < kRqShards && (n_idle >= f.refill_min || n_idle == 64u);
}
// take: claims queries for the idle lanes: the wave's new shard and count, and the lane's new rid (< f.n), or the one it had
struct Claimed { uint32_t shard; int shards_empty; int rid; };
DRT_DEV Claimed claim_take(uint32_t shard, int shards_empty, int rid, uint64_t idle, const QueryFrame &f) {
    const uint32_t n_idle = (uint32_t)__popcll(idle);
    const int my_rank = lane_rank(idle);
    const bool was_idle = rid < 0;
    uint32_t filled = 0;
    while (filled < n_idle && shards_empty < kRqShards) {
        const uint32_t want = n_idle - filled;
        const ShardRange s = shard_range(f.n, shard);
        // lane 0 claims and clips the claim to the shard; start / got go to the wave (64-bit signed arithmetic: the
        // shard's remainder len - b is negative once other waves have emptied it)
        int64_t start = 0, got = 0;
        if ((threadIdx.x & 63) == 0) {
            const int64_t b = (int64_t)atomicAdd(f.heads + shard * kRqShardStride, want);
            const int64_t left = (int64_t)s.len - b;
            if (left > 0) { start = (int64_t)s.begin + b; got = left < (int64_t)want ? left : (int64_t)want; }
        }
        start = __shfl(start, 0);
        got = __shfl(got, 0);
        if (got <= 0) { shard = (shard + 1) % kRqShards; shards_empty++; continue; }
        const int64_t k = (int64_t)my_rank - (int64_t)filled;
        if (was_idle && k >= 0 && k < got && start + k < (int64_t)f.n) rid = (int)(start + k);
        filled += (uint32_t)got;
    }
    return Claimed{shard, shards_empty, rid};
}
// nothing left to claim and no lane of the wave busy: the wave's loop ends
DRT_DEV bool claim_drained(int shards_empty, int rid) { return shards_empty >= kRqShards && __ballot(rid >= 0) == 0; }

// where this thread's stack lives beyond its LDS levels
struct StackLane {
    int tid;                     // thread in the workgroup: the LDS column
    uint32_t gthread, gthreads;  // thread in the grid, grid threads: the HBM column and pitch
    uint32_t levels;             // QueryFrame::stack_levels
    uint32_t *hbm;               // QueryFrame::stack_hbm
};

// entry [level][tid] of a kernel's LDS array, as an LDS access: a C++ reference to the array is a generic pointer, and a generic
// LDS access next to the generic HBM one invites the compiler to merge the two into one flat access
template <class T, int K>
DRT_DEV __attribute__((address_space(3))) T &lds_at(T (&s)[K][kRqThreads], uint32_t level, int tid) {
    return *(__attribute__((address_space(3))) T *)&s[level][tid];
}

// 4-byte entries.  pop: sp > 0 on entry; store: unguarded; push: iff `push` and a level is free
template <int K>
DRT_DEV uint32_t stack_pop(const uint32_t (&s_ref)[K][kRqThreads], const StackLane &st, uint32_t &sp) {
    --sp;
    return sp < (uint32_t)K ? lds_at(s_ref, sp, st.tid) : st.hbm[(size_t)(sp - K) * st.gthreads + st.gthread];
}
template <int K>
DRT_DEV void stack_store(uint32_t (&s_ref)[K][kRqThreads], const StackLane &st, uint32_t &sp, uint32_t ref) {
    if (sp < (uint32_t)K) lds_at(s_ref, sp, st.tid) = ref;
    else st.hbm[(size_t)(sp - K) * st.gthreads + st.gthread] = ref;
    ++sp;
}
template <int K>
DRT_DEV void stack_push(uint32_t (&s_ref)[K][kRqThreads], const StackLane &st, uint32_t &sp, uint32_t ref, bool push) {
    if (push && sp < st.levels) stack_store(s_ref, st, sp, ref);
}

// 8-byte entries {ref, key}
template <int K>
DRT_DEV uint32_t stack_pop(const uint32_t (&s_ref)[K][kRqThreads], const float (&s_key)[K][kRqThreads], const StackLane &st,
                                              uint32_t &sp, float &key) {
    --sp;
    uint32_t ref;
    if (sp < (uint32_t)K) {
        ref = lds_at(s_ref, sp, st.tid); key = lds_at(s_key, sp, st.tid);
    } else {
        const uint2 e = reinterpret_cast<const uint2 *>(st.hbm)[(size_t)(sp - K) * st.gthreads + st.gthread];
        ref = e.x; key = __uint_as_float(e.y);
    }
    return ref;
}
template <int K>
DRT_DEV void stack_store(uint32_t (&s_ref)[K][kRqThreads], float (&s_key)[K][kRqThreads], const StackLane &st, uint32_t &sp,
                                            uint32_t ref, float key) {
    if (sp < (uint32_t)K) { lds_at(s_ref, sp, st.tid) = ref; lds_at(s_key, sp, st.tid) = key; }
    else reinterpret_cast<uint2 *>(st.hbm)[(size_t)(sp - K) * st.gthreads + st.gthread] = make_uint2(ref, __float_as_uint(key));
    ++sp;
}

// the ordered kernels' two children: the one with the larger key goes on first (key1 > key2 -> child 1), so the nearer one is
// popped first; each only if its push flag is set and a level is free
template <int K>
DRT_DEV void push_far_first(uint32_t (&s_ref)[K][kRqThreads], const StackLane &st, uint32_t &sp, uint32_t ref1, float key1,
                                               bool push1, uint32_t ref2, float key2, bool push2) {
    const bool far1 = key1 > key2;
    const uint32_t ra = far1 ? ref1 : ref2, rb = far1 ? ref2 : ref1;
    const bool pa = far1 ? push1 : push2, pb = far1 ? push2 : push1;
#pragma unroll
    for (int k = 0; k < 2; k++)
        if ((k == 0 ? pa : pb) && sp < st.levels) stack_store(s_ref, st, sp, k == 0 ? ra : rb);
}
template <int K>
DRT_DEV void push_far_first(uint32_t (&s_ref)[K][kRqThreads], float (&s_key)[K][kRqThreads], const StackLane &st, uint32_t &sp,
                                               uint32_t ref1, float key1, bool push1, uint32_t ref2, float key2, bool push2) {
    const bool far1 = key1 > key2;
    const uint32_t ra = far1 ? ref1 : ref2, rb = far1 ? ref2 : ref1;
    const float ka = far1 ? key1 : key2, kb = far1 ? key2 : key1;
    const bool pa = far1 ? push1 : push2, pb = far1 ? push2 : push1;
#pragma unroll
    for (int k = 0; k < 2; k++)
        if ((k == 0 ? pa : pb) && sp < st.levels) stack_store(s_ref, s_key, st, sp, k == 0 ? ra : rb, k == 0 ? ka : kb);
}

#endif  // __HIPCC__

}  // namespace drt
