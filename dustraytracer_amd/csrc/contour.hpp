// contour.hpp -- launch seam of kernel_contour.hip (section contours, the chaining of a plane's segments into open polylines and
// closed loops: include/drt.h drt_renderer_chain_sections), the layout of its scratch and the number of its jumping rounds.
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

// Enqueues every phase on `stream`: no host synchronisation, no workgroup waits for another one
hipError_t launch_contour(const ContourArgs &args, hipStream_t stream);

}  // namespace drt
