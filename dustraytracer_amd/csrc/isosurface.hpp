// isosurface.hpp -- launch seam of kernel_isosurface.hip (isosurface extraction, watertight triangles from a 3-D field by marching
// tetrahedra: include/drt.h drt_renderer_isosurface), the sizing of its grid, and the rule's tables: the six tetrahedra of a cube,
// which of them are mirror images, the 16-row triangle table and the edge a table entry names.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace drt {

constexpr int kIsoThreads = 256;              // 4 waves per workgroup; a wave never talks to another one
constexpr int kIsoCountWavesPerSimd = 8;      // the wave slots the persistent grid is sized by: what the count pass's 36 VGPRs ...
constexpr int kIsoFillWavesPerSimd = 5;       // ... and the fill pass's 85 attain
constexpr int kIsoChunk = 63;                 // cubes of a row per step of a wave: lane 63 only lends its column to lane 62

struct IsoArgs {
    const float *field;          // float32 [Z][Y][X]
    const uint32_t *offsets;     // rows + 1 words: row r owns out[offsets[r] .. offsets[r + 1]), clamped to out_capacity (fill only)
    void *out;                   // drt_iso_tri[out_capacity] (48 B, 16-B aligned); null in the count pass
    uint32_t *counts;            // rows words or null: every triangle of the row, stored or not
    uint32_t out_capacity;
    uint32_t dims[3];            // samples X, Y, Z
    uint32_t cubes[3];           // cubes per axis: dims - 1, or dims + 1 with a border
    uint32_t rows;               // cubes[1] * cubes[2]
    uint32_t waves;              // waves of the grid that work: iso_waves()
    int32_t pad;                 // 1 with a border (cube c's first corner is lattice index c - 1), else 0
    int32_t swap;                // flip: every triangle's vertices 1 and 2 change places once more
    float level, border;         // border: the virtual layer's value, NaN without one
    float lo[3], cell[3];
};

// waves of a launch: min(rows, the chip's wave slots for that pass), at least one
inline uint32_t iso_waves(uint32_t rows, int num_cus, bool fill) {
    const size_t w = std::min<size_t>((size_t)std::max(1, num_cus) * 4 * (fill ? kIsoFillWavesPerSimd : kIsoCountWavesPerSimd), rows);
    return (uint32_t)std::max<size_t>(w, 1);
}

// fill: the pass that stores records (out != null); otherwise the count pass
hipError_t launch_isosurface(bool fill, const IsoArgs &args, hipStream_t stream);

// drt.h "cubes": tetrahedron i is (0, DRT_ISO_TET_B(i), DRT_ISO_TET_C(i), 7); "triangles": tetrahedra 1, 2 and 5 are mirror images
#define DRT_ISO_TET_B(i) ((i) < 2 ? 1 : ((i) < 4 ? 2 : 4))
#define DRT_ISO_TET_C(i) ((i) == 0 || (i) == 2 ? 3 : ((i) == 1 || (i) == 4 ? 5 : 6))
#define DRT_ISO_MIRROR(i) ((i) == 1 || (i) == 2 || (i) == 5)

// drt.h "table": a row is up to two triangles of three edge numbers; packed three bits per edge, triangle 0 in bits 0-8, triangle 1
// in bits 9-17, the number of triangles in bits 18-19.  Edge numbers: 0 = (0,1), 1 = (0,2), 2 = (0,3), 3 = (1,2), 4 = (1,3), 5 = (2,3).
#define DRT_ISO_ROW0() 0u
#define DRT_ISO_ROW1(a, b, c) ((uint32_t)(a) | (uint32_t)(b) << 3 | (uint32_t)(c) << 6 | 1u << 18)
#define DRT_ISO_ROW2(a, b, c, d, e, f) \
    ((uint32_t)(a) | (uint32_t)(b) << 3 | (uint32_t)(c) << 6 | (uint32_t)(d) << 9 | (uint32_t)(e) << 12 | (uint32_t)(f) << 15 | 2u << 18)
#define DRT_ISO_TABLE                                                                                                                  \
    { DRT_ISO_ROW0(),                 /*  0 ----                       */ DRT_ISO_ROW1(0, 2, 1),          /*  1 0 above                */ \
      DRT_ISO_ROW1(0, 3, 4),          /*  2 1 above                    */ DRT_ISO_ROW2(1, 3, 4, 1, 4, 2), /*  3 0 1 above              */ \
      DRT_ISO_ROW1(1, 5, 3),          /*  4 2 above                    */ DRT_ISO_ROW2(2, 5, 3, 2, 3, 0), /*  5 0 2 above              */ \
      DRT_ISO_ROW2(0, 1, 5, 0, 5, 4), /*  6 1 2 above                  */ DRT_ISO_ROW1(2, 5, 4),          /*  7 3 below                */ \
      DRT_ISO_ROW1(2, 4, 5),          /*  8 3 above                    */ DRT_ISO_ROW2(0, 4, 5, 0, 5, 1), /*  9 0 3 above              */ \
      DRT_ISO_ROW2(3, 5, 2, 3, 2, 0), /* 10 1 3 above                  */ DRT_ISO_ROW1(1, 3, 5),          /* 11 2 below                */ \
      DRT_ISO_ROW2(1, 2, 4, 1, 4, 3), /* 12 2 3 above                  */ DRT_ISO_ROW1(0, 4, 3),          /* 13 1 below                */ \
      DRT_ISO_ROW1(0, 1, 2),          /* 14 0 below                    */ DRT_ISO_ROW0() /* 15 ---- */ }

}  // namespace drt
