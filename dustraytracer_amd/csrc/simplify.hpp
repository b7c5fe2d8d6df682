// simplify.hpp -- launch seam of kernel_simplify.hip (mesh simplification by vertex clustering: include/drt.h drt_renderer_simplify), the
// sizes of its scratch, and the rule's integer helpers for host and device: the cell of a vertex, its key, the cell centre and the
// fixed-point terms, digit for digit as drt.h states them.  The exponent of a maximum and the powers of two are weld.hpp's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "weld.hpp"

namespace drt {

constexpr int kSimplifyThreads = 256;                   // 4 waves per workgroup
constexpr uint32_t kSimplifyScanBlock = 256;            // items per workgroup of a flag scan: one per thread
constexpr uint32_t kSimplifyEmpty = 0xFFFFFFFFu;        // a free slot of the table (no vertex index reaches it: V < 2^31)
constexpr uint32_t kSimplifyOutside = 0xFFFFFFFFu;      // the key of a vertex that is not in the grid (X Y Z < 2^31: no key reaches it)
constexpr int kSimplifyWords = 12;                      // 64-bit sums per cluster: acc[3], A00 A01 A02 A11 A12 A22, b[3]
constexpr int kSimplifyMeanWords = 3;                   // ... of which mean placement uses the first three

inline uint32_t simplify_blocks(uint32_t items) { return (items + kSimplifyScanBlock - 1) / kSimplifyScanBlock; }
// slots of the table: the power of two that is at least 2 V (and at least 64), so the table is never more than half full
inline uint64_t simplify_table_slots(uint32_t n_vertices) {
    uint64_t s = 64;
    while (s < 2ull * n_vertices) s <<= 1;
    return s;
}

enum class SimplifyPlacement : int32_t { mean = 0, quadric = 1 };       // drt.h DRT_SIMPLIFY_MEAN / DRT_SIMPLIFY_QUADRIC

struct SimplifyGrid { float lo[3], cell[3]; uint32_t dims[3]; };

struct SimplifyArgs {
    const float *vertices;       // [V][3]
    const int32_t *faces;        // [N][3]
    uint32_t n_vertices, n_tris; // V > 0
    SimplifyGrid grid;
    // scratch
    uint32_t *key;               // V words: the key of every vertex, kSimplifyOutside if it is not in the grid
    uint32_t *table;             // simplify_table_slots(V) words, all kSimplifyEmpty before the insert
    uint32_t mask;               // slots - 1
    uint32_t *rep;               // V words: the vertex's slot after the insert, its representative after the resolve
    uint32_t *block_totals;      // simplify_blocks(max(V, N)) words
    uint32_t *cnt;               // V zeroed words: the in-grid members of cluster c
    long long *sums;             // kSimplifyWords (quadric) or kSimplifyMeanWords (mean) zeroed words per cluster, V clusters' worth
    uint32_t *max_bits;          // one zeroed word: the bits of L
    bool combine_runs;           // the sums add runs of equal cluster ids across the lanes of a wave first (the default): the same bytes
    // outputs
    int32_t *cluster;            // [V]
    float *out_vertices;         // [vertex_capacity][3]
    int32_t *first;              // [vertex_capacity]
    uint32_t vertex_capacity;
    int32_t *out_faces;          // [tri_capacity][3]
    int32_t *source;             // [tri_capacity]
    uint32_t tri_capacity;
    uint32_t *counts;            // two words: C, M
};

// Enqueues the whole call in stream order: the table's fill, keys + insert, resolve + block totals, offsets, number + scatter of
// first, the gather of the other members' ids, (quadric) the maximum of l, the sums over the vertices, (quadric) the sums over the
// corners, the finish, and the faces' flag scan, offsets and scatter.  No launch waits for anything within itself.
hipError_t launch_simplify(SimplifyPlacement placement, const SimplifyArgs &args, int num_cus, hipStream_t stream);

// ---- the rule's arithmetic, for host and device ----
#ifdef __HIP__
#define DRT_SIMPLIFY_HD __host__ __device__ __forceinline__
#else
#define DRT_SIMPLIFY_HD inline
#endif

DRT_SIMPLIFY_HD bool simplify_finite(float f) { return __builtin_fabsf(f) <= 3.402823466e+38f; }

// drt.h "cell of a vertex": f = (p - lo) / cell, two fp32 operations; in the grid iff 0 <= f < (float)dims; i = (int)f.  False if
// the coordinate is outside (p is finite: the caller has looked).
DRT_SIMPLIFY_HD bool simplify_cell(float p, float lo, float cell, uint32_t dims, uint32_t &i) {
    const float f = (p - lo) / cell;
    if (!(f >= 0.0f && f < (float)dims)) return false;
    i = (uint32_t)(int)f;
    return true;
}

// the key of a position, ix + X (iy + Y iz) < 2^31, or kSimplifyOutside
DRT_SIMPLIFY_HD uint32_t simplify_key(const SimplifyGrid &g, float x, float y, float z) {
    if (!simplify_finite(x) || !simplify_finite(y) || !simplify_finite(z)) return kSimplifyOutside;
    uint32_t ix, iy, iz;
    if (!simplify_cell(x, g.lo[0], g.cell[0], g.dims[0], ix) || !simplify_cell(y, g.lo[1], g.cell[1], g.dims[1], iy) ||
        !simplify_cell(z, g.lo[2], g.cell[2], g.dims[2], iz))
        return kSimplifyOutside;
    return ix + g.dims[0] * (iy + g.dims[1] * iz);
}

// drt.h "position of a cluster": the centre of cell i along one axis, g = lo + ((float)i + 0.5f) * cell, each operation rounded
DRT_SIMPLIFY_HD float simplify_centre(float lo, float cell, uint32_t i) { return lo + ((float)i + 0.5f) * cell; }

// (int64) trunc((double)x * 2^30)
DRT_SIMPLIFY_HD long long simplify_fixed(float x) { return weld_fixed(x, 0x1p30); }

}  // namespace drt
