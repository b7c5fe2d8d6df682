// contour.hpp -- launch seam of kernel_contour.hip (section contours, the chaining of a plane's segments into open polylines and
// closed loops: include/drt.h drt_renderer_chain_sections), the layout of its scratch and the number of its jumping rounds; and the
// seam through which kernel_curve.hip (intersection curves: drt_renderer_chain_intersections) runs the same phases behind a link of
// its own.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace drt {

constexpr int kContourThreads = 256;             // one lane per record
constexpr int kContourScanItems = 4;             // records per lane of the scan kernels
constexpr int kContourScanBlock = kContourThreads * kContourScanItems;
constexpr uint32_t kContourNone = 0xffffffffu;   // no predecessor / no owner
constexpr uint32_t kContourFlag = 0x80000000u;   // succ: no successor, the low bits are the exit status; state.x: the record is ranked
constexpr int kContourMaxRounds = 31;            // total < 2^31

// Rounds of pointer jumping that rank every chain of up to `total` records: the smallest R with 2^R >= total
inline int contour_rounds(uint32_t total) {
    int r = 0;
    while (((uint64_t)1 << r) < total) r++;
    return r;
}
inline uint32_t contour_scan_blocks(uint32_t total) { return (total + kContourScanBlock - 1) / kContourScanBlock; }

// The scratch of one call, in words, carved from one allocation: two 16-byte states per record (ping-pong), four words per record,
// three sums per scan block, one flag per round (+ 1).  The state comes first: it is read and written as 16-byte words.
inline size_t contour_scratch_words(uint32_t total) {
    return (size_t)total * 12 + (size_t)contour_scan_blocks(total) * 3 + (kContourMaxRounds + 1);
}

struct ContourArgs {
    const void *segs;            // drt_section[total] (32 B, 16-B aligned)
    const uint32_t *splits;      // n + 1 words
    void *slots;                 // drt_chain_slot[total] (16 B, 16-B aligned)
    uint32_t *chains;            // 2 n words or null
    const int32_t *adj;          // 3 * n_tris words: the uploaded scene's edge adjacency
    uint32_t n, total, n_tris;
    // scratch (contour_scratch_words)
    uint4 *state[2];             // {ancestor | ranked flag, rank or offset of the minimum, minimum index seen, -}
    uint32_t *key;               // prim of every record, 0xffffffff for a miss record; later the chain lengths (at a chain's first record)
    uint32_t *owner;             // the plane that owns the record, or none
    uint32_t *succ;              // the successor, or flag | exit status
    uint32_t *pred;              // the predecessor, or none; later the exclusive scan (the position of a chain's first record)
    uint32_t *block_sums;        // 3 per scan block
    uint32_t *moved;             // moved[k + 1] != 0: round k still moved a record; zeroed in front (round 0 always runs)
    // intersection curves only (kernel_curve.hip): there `n` counts queries, `chains` is the three words of counts, and the phases
    // behind the link run over the single range [0, total)
    const int32_t *query_adj;    // 3 n words: the query mesh's edge adjacency
};

inline void contour_carve(ContourArgs &a, uint32_t *work) {
    const size_t t = a.total;
    a.state[0] = reinterpret_cast<uint4 *>(work);
    a.state[1] = a.state[0] + t;
    uint32_t *w = work + 8 * t;
    a.key = w; a.owner = w + t; a.succ = w + 2 * t; a.pred = w + 3 * t;
    a.block_sums = w + 4 * t;
    a.moved = a.block_sums + (size_t)contour_scan_blocks(a.total) * 3;
}

// drt.h "inputs": the range of plane / query i as drt_renderer_plane_sections clamps cap_i -- a decreasing pair is empty, nothing
// beyond total
struct ContourRange { uint32_t lo, hi; };
static __device__ __forceinline__ ContourRange contour_range(const uint32_t *splits, uint32_t i, uint32_t total) {
    const uint32_t lo = splits[i], end = splits[i + 1];
    uint32_t cap = end > lo ? end - lo : 0u;
    if (lo >= total) cap = 0u;
    else cap = cap < total - lo ? cap : total - lo;
    ContourRange r;
    r.lo = lo; r.hi = lo + cap;
    return r;
}

// The owner of record j: the last range that starts at or before j (a binary search, as if splits ascended), if it holds j
static __device__ __forceinline__ uint32_t contour_owner(const uint32_t *splits, uint32_t n, uint32_t total, uint32_t j) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (splits[mid] <= j) lo = mid + 1;
        else hi = mid;
    }
    if (lo == 0) return kContourNone;
    const ContourRange r = contour_range(splits, lo - 1, total);
    return j >= r.lo && j < r.hi ? lo - 1 : kContourNone;
}

static __device__ __forceinline__ uint32_t contour_seg_word(const void *segs, uint32_t j, int word) {
    return reinterpret_cast<const uint32_t *>(segs)[(size_t)j * 8 + word];
}

// Enqueues every phase on `stream`: no host synchronisation, no workgroup waits for another one
hipError_t launch_contour(const ContourArgs &args, hipStream_t stream);

// The phases behind the link -- init, the jumping rounds, tail, scan, scatter -- over what keys and link left in key, succ and pred.
// whole = false: per plane, by owner and splits, as launch_contour runs them.  whole = true: one range [0, total) that every record
// belongs to (owner and splits are not read), a record without a chain (succ = flag | 5) is a chain of one where its index puts it,
// and chains[0..1] = {chains, closed ones} of the whole list.  `moved` must have been zeroed on the stream in front.
hipError_t launch_chain_phases(const ContourArgs &args, bool whole, hipStream_t stream);

// Intersection curves: keys / owner, the link across triangles and queries, then launch_chain_phases(whole)
hipError_t launch_curves(const ContourArgs &args, hipStream_t stream);

}  // namespace drt
