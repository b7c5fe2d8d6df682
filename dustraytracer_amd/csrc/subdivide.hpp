// subdivide.hpp -- launch seam of kernel_subdivide.hip (one level of midpoint or Loop subdivision of an indexed mesh on the device:
// include/drt.h drt_renderer_subdivide) and the sizes of its scratch.  The connectivity is kernel_adjacency.hip's, by index and with
// the edges numbered (adjacency.hpp: launch_adjacency); the fixed-point scale is the smoothing's (weld.hpp: launch_smooth_maximum).
//
// Scratch beyond what the adjacency call uses, all recomputed by every call:
//   adj, edge    3 N words each                                                   24 bytes per triangle   (sd_adj, sd_edge)
//   half_edge    3 N words: the capacity, E of them are written                   12 bytes per triangle   (sd_half_edge)
//   counts       the word E, then with Loop n_int[V] and n_cr[V]                  8 bytes per vertex      (sd_cnt)
//   sums         with Loop 3 V int64 words twice: the interior set in the words of wd_acc, where the adjacency's `other` lay until
//                its last launch was over (stream order), and the crease set      24 + 24 bytes per vertex (wd_acc, sd_acc)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "weld.hpp"

namespace drt {

enum class SubdivideScheme : int32_t { midpoint = 0, loop = 1 };      // drt.h DRT_SUBDIVIDE_MIDPOINT / DRT_SUBDIVIDE_LOOP

constexpr uint32_t kSubdivideNaN = 0x7FC00000u;         // the three words of the odd vertex of an unusable edge

struct SubdivideArgs {
    const float *vertices;       // [V][3]
    const int32_t *faces;        // [N][3]
    uint32_t n_vertices, n_tris;
    const int32_t *adj;          // [3 N]: launch_adjacency's, by index
    const int32_t *edge;         // [3 N]
    const int32_t *half_edge;    // [E] of 3 N
    const uint32_t *edge_count;  // one word: E (not read when n_tris == 0)
    long long *acc_int;          // 3 V zeroed words: the sums over the interior edges (Loop)
    long long *acc_cr;           // 3 V zeroed words: the sums over the crease edges (Loop)
    uint32_t *n_int, *n_cr;      // V zeroed words each (Loop)
    const uint32_t *max_bits;    // one word: the bits of M, launch_smooth_maximum's (Loop)
    float *out_vertices;         // [capacity][3] or null
    int32_t *parents;            // [capacity][2] or null
    uint32_t capacity;
    int32_t *out_faces;          // [4 N][3]
    uint32_t *vertex_count;      // one word: V + E, stored or not
};

// Enqueues the children (and the count), then, with a capacity, the edges -- odd vertices, their parents, with Loop the sums -- and
// the finish -- even vertices and their parents: three launches in stream order, none of which waits for anything within a launch.
// The caller has enqueued launch_adjacency, the zeroing of the sums and counts and, with Loop, launch_smooth_maximum before.
hipError_t launch_subdivide(SubdivideScheme scheme, const SubdivideArgs &args, int num_cus, hipStream_t stream);

}  // namespace drt
