// kernel_contour.hip -- section contours (include/drt.h drt_renderer_chain_sections): the segments of every plane chained into open
// polylines and closed loops by the mesh's edge adjacency.  Integers only: no coordinate is read.
//
// One lane per record over the whole batch, in phases that are separate launches (a phase reads what other lanes of the phase
// before wrote; no workgroup ever waits for another one):
//   keys      the plane that owns the record (binary search in splits, then the clamped range is checked) and a dense 4-byte array
//             of the records' prim: the link's binary search strides over 4 bytes, not over 32-byte records
//   link      drt.h "link": the exit edge, its twin, the record of the twin's triangle in the plane's range (binary search in the keys:
//             a miss record's prim -1 is the largest unsigned key, so the whole range is ascending), the check of its entry edge;
//             succ[j] = m and atomicMin(pred[m], j).  The link is injective, so the minimum is the only writer of its word; on input
//             that no fill wrote (a triangle twice in one range) the smallest index wins ...
//   init      ... and a record whose successor took another predecessor loses its link (status 3): succ and pred are exact inverses,
//             so every component is a simple path or a simple cycle whatever the input.  The jumping state of every record.
//   jump x R  pointer jumping along pred, ping-pong between two 16-byte states per record (one 16-byte load per dependent step).  A
//             record's window is the 2^k records behind it; when the window's far end is ranked (it knows its head and its distance
//             to it) the record is ranked too.  A record on a cycle never is: it carries the smallest index of its window and the
//             offset at which the window first meets it, which, once the window holds the whole cycle, are the cycle's start and the
//             record's rank behind it -- the cut in front of the start needs no second pass.  R = ceil(log2(total)) rounds are
//             launched, because the host does not know the longest chain; a round flags whether it ranked a record or moved
//             a minimum, and the next round returns at once when it did not (then nothing is left to do: while a path has unranked
//             records, the one at depth 2^k is ranked by round k, and a cycle whose minima all stand still has them all equal).
//   tail      the last record of every chain stores the chain's length at its first record (a plain store: one writer per chain)
//   scan      a two-level exclusive scan over the record index of "length, if the record starts a chain", as kernel_adaptive.hip
//             scans its counts.  The scan is global, not segmented: the chains and miss records of a range partition it, and a record
//             outside every range counts 1, so every range sums to its own size and the scan at a chain's first record IS its
//             position.  The counts of chains and of closed chains ride along; a range's first and last records add their
//             difference to chains[] (two integer atomics per word: the order does not matter).
//   scatter   slots[position of the first record + rank] = {record, first, length, flags}
//
// Everything behind the link is also what the intersection curves run (kernel_curve.hip, through contour.hpp launch_chain_phases), over
// one range [0, total) instead of a range per plane: the three kernels that look at ranges are templates on that, kWhole.
//
// Bounds on any input: a record's prim and code are checked before they index the adjacency; pred, succ and the states hold record
// indices below total; a position is written only inside its plane's range (else the record is written as a chain of one at its own
// index), which input with overlapping ranges needs.
#include <hip/hip_runtime.h>

#include "contour.hpp"

namespace drt {

namespace {

#define CT_DEV static __device__ __forceinline__

using Range = ContourRange;

// (contour.hpp: kernel_curve.hip reads ranges and records the same way)
CT_DEV Range plane_range(const uint32_t *splits, uint32_t i, uint32_t total) { return contour_range(splits, i, total); }
CT_DEV uint32_t seg_word(const void *segs, uint32_t j, int word) { return contour_seg_word(segs, j, word); }

// The range a record's position must lie in: its plane's, or in a kWhole launch (contour.hpp launch_chain_phases) the whole list
template <bool kWhole>
CT_DEV Range record_range(const ContourArgs &a, uint32_t owner) {
    if (kWhole) { Range r; r.lo = 0u; r.hi = a.total; return r; }
    return plane_range(a.splits, owner, a.total);
}

// the edges a record is entered and left through: valid iff code < 8 and its apex < 3
CT_DEV bool code_edges(uint32_t code, uint32_t &in, uint32_t &out) {
    const uint32_t k = code & 3u;
    const bool up = (code >> 2) != 0u;
    const uint32_t k2 = k == 0u ? 2u : k - 1u;         // (k + 2) % 3
    in = up ? k : k2;
    out = up ? k2 : k;
    return code < 8u && k < 3u;
}

__global__ __launch_bounds__(kContourThreads) void contour_keys_kernel(const ContourArgs a) {
    const uint32_t j = blockIdx.x * kContourThreads + threadIdx.x;
    if (j >= a.total) return;
    a.owner[j] = contour_owner(a.splits, a.n, a.total, j);      // the last plane whose range starts at or before j
    a.key[j] = seg_word(a.segs, j, 3);
    a.pred[j] = kContourNone;
}

__global__ __launch_bounds__(kContourThreads) void contour_link_kernel(const ContourArgs a) {
    const uint32_t j = blockIdx.x * kContourThreads + threadIdx.x;
    if (j >= a.total) return;
    const uint32_t owner = a.owner[j];
    const uint32_t prim = a.key[j];
    uint32_t in, out;
    const bool valid = code_edges(seg_word(a.segs, j, 7), in, out);
    uint32_t link = kContourFlag | 5u;                  // a miss record (and what cannot be read as a record)
    if (owner != kContourNone && valid && prim < a.n_tris) {
        const int32_t twin = a.adj[3u * prim + out];
        if (twin < 0) link = kContourFlag | (twin == -1 ? 1u : 2u);
        else {
            const uint32_t target = (uint32_t)twin / 3u;
            const Range r = plane_range(a.splits, owner, a.total);
            uint32_t lo = r.lo, hi = r.hi;
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (a.key[mid] < target) lo = mid + 1;
                else hi = mid;
            }
            link = kContourFlag | 3u;
            if (lo < r.hi && a.key[lo] == target) {
                uint32_t in_m, out_m;
                const bool valid_m = code_edges(seg_word(a.segs, lo, 7), in_m, out_m);
                if (valid_m && 3u * target + in_m == (uint32_t)twin) {
                    link = lo;
                    atomicMin(&a.pred[lo], j);
                } else link = kContourFlag | 4u;
            }
        }
    }
    a.succ[j] = link;
}

__global__ __launch_bounds__(kContourThreads) void contour_init_kernel(const ContourArgs a) {
    const uint32_t j = blockIdx.x * kContourThreads + threadIdx.x;
    if (j >= a.total) return;
    const uint32_t link = a.succ[j];
    if (!(link & kContourFlag) && a.pred[link] != j) a.succ[j] = kContourFlag | 3u;
    const uint32_t p = a.pred[j];
    a.state[0][j] = p == kContourNone ? make_uint4(j | kContourFlag, 0u, j, 0u) : make_uint4(p, 0u, j, 0u);
}

__global__ __launch_bounds__(kContourThreads) void contour_jump_kernel(const ContourArgs a, int round) {
    if (round > 0 && a.moved[round] == 0u) return;       // the round before moved nothing: every later round returns here
    const uint32_t j = blockIdx.x * kContourThreads + threadIdx.x;
    bool moved = false;
    if (j < a.total) {
        const uint4 *from = a.state[round & 1];
        uint4 s = from[j];
        if (!(s.x & kContourFlag)) {
            const uint4 far = from[s.x];
            const uint32_t step = 1u << round;          // the records between j and its ancestor
            if (far.x & kContourFlag) {
                s = make_uint4(far.x, step + far.y, s.z, 0u);
                moved = true;
            } else {
                if (far.z < s.z) {
                    s.z = far.z; s.y = step + far.y;
                    moved = true;
                }
                s.x = far.x;
            }
        }
        a.state[(round + 1) & 1][j] = s;
    }
    // One flag for the next round, not a count: a count took one atomic per wave on one word, and at 3.9 million records those
    // 60 000 same-address atomics were 0.66 of a round's 0.69 ms.  A workgroup votes, and stores only while the flag still reads 0.
    const bool any = __syncthreads_or(moved) != 0;
    if (any && threadIdx.x == 0 && __hip_atomic_load(&a.moved[round + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u)
        __hip_atomic_store(&a.moved[round + 1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// What the jumping left of record j: its chain's first record, its rank in the chain, and whether the chain is closed
struct Ranked { uint32_t start, rank; bool closed; };
CT_DEV Ranked ranked(const uint4 s) {
    Ranked r;
    r.closed = !(s.x & kContourFlag);
    r.start = r.closed ? s.z : (s.x & ~kContourFlag);
    r.rank = s.y;
    return r;
}

__global__ __launch_bounds__(kContourThreads) void contour_tail_kernel(const ContourArgs a, const uint4 *state) {
    const uint32_t j = blockIdx.x * kContourThreads + threadIdx.x;
    if (j >= a.total) return;
    const Ranked r = ranked(state[j]);
    const uint32_t link = a.succ[j];
    if ((link & kContourFlag) || (r.closed && link == r.start)) a.key[r.start] = r.rank + 1u;     // (the keys are spent: the lengths)
}

struct Sums { uint32_t length, chains, closed; };

// what record j adds to the scans
template <bool kWhole>
CT_DEV Sums scan_term(const ContourArgs &a, const uint4 *state, uint32_t j) {
    Sums t = { 0u, 0u, 0u };
    if (j >= a.total) return t;
    if (!kWhole && a.owner[j] == kContourNone) { t.length = 1u; return t; }
    const Ranked r = ranked(state[j]);
    if (r.start != j) return t;
    t.length = a.key[j];
    t.chains = a.succ[j] != (kContourFlag | 5u) ? 1u : 0u;
    t.closed = r.closed ? t.chains : 0u;
    return t;
}

CT_DEV uint32_t wave_inclusive(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(v, d, 64);
        if (lane >= d) v += up;
    }
    return v;
}

// The exclusive prefix of this lane's `mine` among the workgroup's lanes and the workgroup's sums.  Ends with a barrier.
CT_DEV Sums block_exclusive(Sums mine, Sums *s_wave, Sums *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Sums incl = { wave_inclusive(mine.length), wave_inclusive(mine.chains), wave_inclusive(mine.closed) };
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    Sums before = { 0u, 0u, 0u }, all = { 0u, 0u, 0u };
#pragma unroll
    for (int w = 0; w < kContourThreads / 64; w++) {
        const Sums t = s_wave[w];
        if (w < wave) { before.length += t.length; before.chains += t.chains; before.closed += t.closed; }
        all.length += t.length; all.chains += t.chains; all.closed += t.closed;
    }
    __syncthreads();
    *total = all;
    Sums r = { before.length + incl.length - mine.length, before.chains + incl.chains - mine.chains, before.closed + incl.closed - mine.closed };
    return r;
}

template <bool kWhole>
__global__ __launch_bounds__(kContourThreads) void contour_block_sums_kernel(const ContourArgs a, const uint4 *state) {
    __shared__ Sums s_wave[kContourThreads / 64];
    const uint32_t first = blockIdx.x * kContourScanBlock + threadIdx.x * kContourScanItems;
    Sums mine = { 0u, 0u, 0u };
#pragma unroll
    for (int k = 0; k < kContourScanItems; k++) {
        const Sums t = scan_term<kWhole>(a, state, first + k);
        mine.length += t.length; mine.chains += t.chains; mine.closed += t.closed;
    }
    Sums total;
    (void)block_exclusive(mine, s_wave, &total);
    if (threadIdx.x == 0) {
        a.block_sums[3u * blockIdx.x] = total.length;
        a.block_sums[3u * blockIdx.x + 1] = total.chains;
        a.block_sums[3u * blockIdx.x + 2] = total.closed;
    }
}

// the block sums become their own exclusive prefix sums, in place; one workgroup, in chunks with a carry
__global__ __launch_bounds__(kContourThreads) void contour_scan_sums_kernel(const ContourArgs a, uint32_t n_blocks) {
    __shared__ Sums s_wave[kContourThreads / 64];
    Sums carry = { 0u, 0u, 0u };
    for (uint32_t chunk = 0; chunk < n_blocks; chunk += kContourThreads) {
        const uint32_t b = chunk + threadIdx.x;
        Sums mine = { 0u, 0u, 0u };
        if (b < n_blocks) { mine.length = a.block_sums[3u * b]; mine.chains = a.block_sums[3u * b + 1]; mine.closed = a.block_sums[3u * b + 2]; }
        Sums total;
        const Sums before = block_exclusive(mine, s_wave, &total);
        if (b < n_blocks) {
            a.block_sums[3u * b] = carry.length + before.length;
            a.block_sums[3u * b + 1] = carry.chains + before.chains;
            a.block_sums[3u * b + 2] = carry.closed + before.closed;
        }
        carry.length += total.length; carry.chains += total.chains; carry.closed += total.closed;
    }
}

template <bool kWhole>
__global__ __launch_bounds__(kContourThreads) void contour_offsets_kernel(const ContourArgs a, const uint4 *state) {
    __shared__ Sums s_wave[kContourThreads / 64];
    const uint32_t first = blockIdx.x * kContourScanBlock + threadIdx.x * kContourScanItems;
    Sums v[kContourScanItems], mine = { 0u, 0u, 0u };
#pragma unroll
    for (int k = 0; k < kContourScanItems; k++) {
        v[k] = scan_term<kWhole>(a, state, first + k);
        mine.length += v[k].length; mine.chains += v[k].chains; mine.closed += v[k].closed;
    }
    Sums total;
    Sums run = block_exclusive(mine, s_wave, &total);
    run.length += a.block_sums[3u * blockIdx.x];
    run.chains += a.block_sums[3u * blockIdx.x + 1];
    run.closed += a.block_sums[3u * blockIdx.x + 2];
#pragma unroll
    for (int k = 0; k < kContourScanItems; k++) {
        const uint32_t j = first + k;
        if (j < a.total) {
            a.pred[j] = run.length;                      // (the predecessors are spent: the positions)
            const uint32_t owner = kWhole ? 0u : a.owner[j];
            if (a.chains && owner != kContourNone) {
                const Range r = record_range<kWhole>(a, owner);
                if (j == r.lo) {
                    atomicSub(&a.chains[2u * owner], run.chains);
                    atomicSub(&a.chains[2u * owner + 1], run.closed);
                }
                if (j == r.hi - 1u) {
                    atomicAdd(&a.chains[2u * owner], run.chains + v[k].chains);
                    atomicAdd(&a.chains[2u * owner + 1], run.closed + v[k].closed);
                }
            }
        }
        run.length += v[k].length; run.chains += v[k].chains; run.closed += v[k].closed;
    }
}

template <bool kWhole>
__global__ __launch_bounds__(kContourThreads) void contour_scatter_kernel(const ContourArgs a, const uint4 *state) {
    const uint32_t j = blockIdx.x * kContourThreads + threadIdx.x;
    if (j >= a.total) return;
    const uint32_t owner = kWhole ? 0u : a.owner[j];
    if (owner == kContourNone) return;
    const Ranked r = ranked(state[j]);
    const uint32_t link = a.succ[j];
    const uint32_t status = (link & kContourFlag) ? (link & 7u) : 0u;
    const uint32_t first = a.pred[r.start], length = a.key[r.start];
    const uint32_t pos = first + r.rank;
    const Range range = record_range<kWhole>(a, owner);
    uint4 *slots = reinterpret_cast<uint4 *>(a.slots);
    if (first >= range.lo && pos >= first && pos < range.hi) slots[pos] = make_uint4(j, first, length, (r.closed ? 1u : 0u) | (status << 1));
    else slots[j] = make_uint4(j, j, 1u, status << 1);
}

}  // namespace

template <bool kWhole>
static void launch_phases(const ContourArgs &a, hipStream_t stream) {
    const int rounds = contour_rounds(a.total);
    const dim3 block(kContourThreads);
    const dim3 lanes((a.total + kContourThreads - 1) / kContourThreads);
    const uint32_t n_blocks = contour_scan_blocks(a.total);
    hipLaunchKernelGGL(contour_init_kernel, lanes, block, 0, stream, a);
    for (int k = 0; k < rounds; k++) hipLaunchKernelGGL(contour_jump_kernel, lanes, block, 0, stream, a, k);
    const uint4 *state = a.state[rounds & 1];
    hipLaunchKernelGGL(contour_tail_kernel, lanes, block, 0, stream, a, state);
    hipLaunchKernelGGL(contour_block_sums_kernel<kWhole>, dim3(n_blocks), block, 0, stream, a, state);
    hipLaunchKernelGGL(contour_scan_sums_kernel, dim3(1), block, 0, stream, a, n_blocks);
    hipLaunchKernelGGL(contour_offsets_kernel<kWhole>, dim3(n_blocks), block, 0, stream, a, state);
    hipLaunchKernelGGL(contour_scatter_kernel<kWhole>, lanes, block, 0, stream, a, state);
}

hipError_t launch_chain_phases(const ContourArgs &a, bool whole, hipStream_t stream) {
    if (whole) launch_phases<true>(a, stream);
    else launch_phases<false>(a, stream);
    return hipGetLastError();
}

hipError_t launch_contour(const ContourArgs &a, hipStream_t stream) {
    const dim3 block(kContourThreads);
    const dim3 lanes((a.total + kContourThreads - 1) / kContourThreads);
    hipError_t e = hipMemsetAsync(a.moved, 0, (kContourMaxRounds + 1) * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    if (a.chains) {
        e = hipMemsetAsync(a.chains, 0, (size_t)a.n * 2 * sizeof(uint32_t), stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(contour_keys_kernel, lanes, block, 0, stream, a);
    hipLaunchKernelGGL(contour_link_kernel, lanes, block, 0, stream, a);
    return launch_chain_phases(a, false, stream);
}

}  // namespace drt
