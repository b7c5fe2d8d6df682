// topology.hpp -- launch seams of kernel_topology.hip (mesh topology: include/drt.h drt_renderer_shell_labels, drt_renderer_boundary_loops
// and drt_renderer_shell_terms), the layout of its scratch and the bounds on its launches.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "device_scene.hpp"

namespace drt {

constexpr int kTopoThreads = 256;                // one lane per half-edge, triangle or record
constexpr int kTopoScanItems = 4;                // items per lane of the scan kernels
constexpr int kTopoScanBlock = kTopoThreads * kTopoScanItems;
constexpr uint32_t kTopoNone = 0xffffffffu;      // no predecessor
constexpr uint32_t kTopoFlag = 0x80000000u;      // succ: no successor, the low bits are the exit status; state.x: the record is ranked
constexpr int kTopoMaxRounds = 31;               // jumping rounds of the loops: fewer than 2^31 records
constexpr int kTopoStepGroup = 8;                // labelling steps enqueued between two looks at the step's mode
enum : uint32_t { kTopoDone = 0u, kTopoHook = 1u, kTopoJump = 2u };      // what a labelling step did

inline int topo_log2_ceil(uint32_t n) {          // the smallest L with 2^L >= n
    int l = 0;
    while (((uint64_t)1 << l) < n) l++;
    return l;
}
inline uint32_t topo_scan_blocks(uint32_t n) { return (n + kTopoScanBlock - 1) / kTopoScanBlock; }

// The hard cap on labelling steps.  A round is one hook step and the jump steps that make every tree a star again.
// Stars with a neighbouring star at least halve every two rounds, so 2 L rounds leave none (L = ceil(log2 n_tris)) and one more hook
// step sees that; a hook forest is at most n_tris deep, so a round has at most L jump steps.
inline uint32_t topo_max_steps(uint32_t n_tris) {
    const uint32_t l = (uint32_t)topo_log2_ceil(n_tris);
    return (2u * l + 2u) * (l + 2u);
}

// ---- labelling: label[t] = the smallest triangle index of t's shell
struct TopoLabelArgs {
    const int32_t *adj;          // 3 * n_tris words
    uint32_t n_tris;
    int32_t *label;              // n_tris: every triangle's root as of the last jump step (all trees are stars when a hook step reads it)
    uint32_t *parent;            // scratch, n_tris: parent[t] <= t always
    uint32_t *mode;              // scratch, topo_max_steps + 1 words, zeroed: mode[k] = what step k did
    uint32_t *more;              // scratch, as many: more[k] != 0: hook step k hooked a root / jump step k left a lane below a non-root
};
inline size_t topo_label_words(uint32_t n_tris) { return (size_t)n_tris + 2 * ((size_t)topo_max_steps(n_tris) + 1); }
inline void topo_label_carve(TopoLabelArgs &a, uint32_t *work) {
    a.parent = work;
    a.mode = work + a.n_tris;
    a.more = a.mode + topo_max_steps(a.n_tris) + 1;
}
hipError_t launch_topo_label_init(const TopoLabelArgs &a, hipStream_t stream);
// steps first .. first + count - 1, each of which returns at once when the one before it was the last
hipError_t launch_topo_label_steps(const TopoLabelArgs &a, uint32_t first, uint32_t count, hipStream_t stream);

// ---- counts and the ascending list of boundary half-edges
struct TopoCountArgs {
    const int32_t *adj;
    const int32_t *label;
    uint32_t n_tris;
    uint32_t *counts;            // 3 words: shells, open half-edges, bad half-edges
    uint32_t *block_sums;        // 3 per scan block over the half-edges (shells, open, bad); after the scan their exclusive prefixes
    uint32_t *boundary;          // the half-edges with adj == -1, ascending (topo_compact only)
};
hipError_t launch_topo_counts(const TopoCountArgs &a, hipStream_t stream);       // block sums, their scan, counts
hipError_t launch_topo_compact(const TopoCountArgs &a, uint32_t n_boundary, hipStream_t stream);      // after launch_topo_counts, on its block_sums

// ---- boundary loops over the n_rec records of `boundary`
struct TopoLoopArgs {
    const int32_t *adj;
    const uint32_t *boundary;    // n_rec half-edges, ascending
    uint32_t n_tris, n_rec;
    void *slots;                 // drt_loop_slot[capacity] or null
    uint32_t capacity;
    uint32_t *counts;            // 3 words: records, loops, closed loops
    // scratch (topo_loop_words)
    uint4 *state[2];             // {ancestor | ranked flag, rank or offset of the minimum, minimum index seen, -}
    uint32_t *length;            // at a loop's first record: its length
    uint32_t *succ;              // the successor, or flag | exit status
    uint32_t *pred;              // the predecessor, or none; later the exclusive scan (the position of a loop's first record)
    uint32_t *block_sums;        // 3 per scan block
    uint32_t *moved;             // moved[k + 1] != 0: round k still moved a record; zeroed in front
};
inline size_t topo_loop_words(uint32_t n_rec) { return (size_t)n_rec * 11 + (size_t)topo_scan_blocks(n_rec) * 3 + (kTopoMaxRounds + 1); }
inline void topo_loop_carve(TopoLoopArgs &a, uint32_t *work) {
    const size_t n = a.n_rec;
    a.state[0] = reinterpret_cast<uint4 *>(work);       // (the allocation is 256-byte aligned; the states come first)
    a.state[1] = a.state[0] + n;
    uint32_t *w = work + 8 * n;
    a.length = w; a.succ = w + n; a.pred = w + 2 * n;
    a.block_sums = w + 3 * n;
    a.moved = a.block_sums + (size_t)topo_scan_blocks(a.n_rec) * 3;
}
// Enqueues every phase on `stream`: no host synchronisation, no workgroup waits for another one.  n_rec > 0.
hipError_t launch_topo_loops(const TopoLoopArgs &a, hipStream_t stream);

// ---- measure terms: terms[4 t .. 4 t + 3] = {c.x, c.y, c.z, w} of triangle t
hipError_t launch_topo_terms(const TriHot *tris, uint32_t n_tris, double *terms, hipStream_t stream);

}  // namespace drt
