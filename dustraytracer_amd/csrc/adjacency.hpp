// adjacency.hpp -- launch seam of kernel_adjacency.hip (edge adjacency of a triangle list on the device, by bit-equal positions or by
// vertex index, the numbering of its undirected edges, and boundary vertices: include/drt.h drt_renderer_tri_adjacency /
// drt_renderer_face_adjacency / drt_renderer_boundary_vertices) and the sizes of its scratch.
//
// Scratch per triangle (3 half-edges), all 32-bit words, recomputed by every call:
//   table    weld_table_slots(3 N) words, 2 x 3 N rounded up to a power of two: 24 to 48 bytes      (shared: wd_table)
//   rep      3 N words                                                          12 bytes             (shared: wd_rep)
//   other    3 N words                                                          12 bytes             (shared: the words of wd_acc)
//   blocks   one word per 256 half-edges, only when the edges are numbered      0.05 bytes           (shared: wd_blocks)
// 48 to 72 bytes per triangle in all.  The scene route adds the compacted positions, 36 bytes per triangle, for the length of the call.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "weld.hpp"

namespace drt {

constexpr uint32_t kAdjNone = 0xFFFFFFFFu;              // other[rep]: no second half-edge in the group; rep[h]: h has zero length
constexpr uint32_t kAdjMany = 0u;                       // other[rep]: three or more in the group (half-edge 0 is never a second one)

// drt_renderer_adjacency_route: how the uploaded scene's table was made (0: not yet).  The device route is taken at every size: measured
// on an MI355X the first topology call is 6.3 to 6.6 times faster with it from 11 167 triangles, the smallest scene measured, to 2^20
// (DESIGN 5.35); no crossover by count showed, so none is chosen.
constexpr int kAdjRouteHost = 1, kAdjRouteDevice = 2;

enum class AdjacencyKey : int32_t { position = 3, index = 1 };     // words per end of a half-edge

struct AdjacencyArgs {
    const unsigned char *first;  // end e of triangle t is the key's words at first + t * tri_stride + e * vertex_stride
    uint32_t tri_stride;         // bytes: 36, 48 or 128 by position, 12 by index
    uint32_t vertex_stride;      // bytes: 12 or 32 by position, 4 by index
    uint32_t half_edges;         // 3 N, < 2^31
    uint32_t *table;             // weld_table_slots(half_edges) words, all kWeldEmpty before the insert
    uint32_t mask;               // slots - 1
    uint32_t *rep;               // half_edges words: the slot after the insert; after the resolve the smallest half-edge of h's group
    uint32_t *other;             // half_edges words, all kAdjNone before the resolve: see kAdjNone / kAdjMany
    uint32_t *block_totals;      // weld_blocks(half_edges) words (edges only)
    int32_t *adj;                // [3 N]
    int32_t *edge;               // [3 N] or null: with half_edge and edge_count
    int32_t *half_edge;          // [capacity]
    uint32_t capacity;
    uint32_t *edge_count;        // one word: E, stored or not
};

// Enqueues the two fills, insert, resolve (+ block totals), with edges the offsets and the numbering, and classify: three launches
// and two memsets, or five and two, in stream order; none waits for anything within a launch.
hipError_t launch_adjacency(AdjacencyKey key, const AdjacencyArgs &args, hipStream_t stream);

struct BoundaryArgs {
    const int32_t *faces;        // [N][3]
    const int32_t *adj;          // [3 N]
    uint32_t n_tris, n_vertices;
    uint32_t flags;              // bit 0: -2 counts as well as -1
    uint8_t *out;                // [V], zeroed
};

hipError_t launch_boundary_vertices(const BoundaryArgs &args, hipStream_t stream);

}  // namespace drt
