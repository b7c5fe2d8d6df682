// weld.hpp -- launch seam of kernel_weld.hip (vertex welding, vertex normals and smoothing: include/drt.h drt_renderer_weld /
// drt_renderer_vertex_normals / drt_renderer_smooth_vertices), the sizes of its scratch, and the rules' integer arithmetic: the
// exponent of a maximum and the fixed-point scale made from it, digit for digit as drt.h states them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

namespace drt {

constexpr int kWeldThreads = 256;                       // 4 waves per workgroup
constexpr uint32_t kWeldScanBlock = 256;                // corners per workgroup of the flag scan: one per thread
constexpr uint32_t kWeldEmpty = 0xFFFFFFFFu;            // a free slot of the table (no corner index reaches it: 3 N < 2^31)

// the corners of a call, 3 N, and the workgroups of its scan
inline uint32_t weld_blocks(uint32_t corners) { return (corners + kWeldScanBlock - 1) / kWeldScanBlock; }
// slots of the table: the power of two that is at least 2 * corners (and at least 64), so the table is never more than half full
inline uint64_t weld_table_slots(uint32_t corners) {
    uint64_t s = 64;
    while (s < 2ull * corners) s <<= 1;
    return s;
}

struct WeldArgs {
    const unsigned char *tris;   // corner c = 3 t + k is the three words at tris + t * stride + 12 k
    uint32_t stride;             // 36 or 48 bytes
    uint32_t corners;            // 3 N, < 2^31
    uint32_t *table;             // weld_table_slots(corners) words, all kWeldEmpty before the insert
    uint32_t mask;               // slots - 1
    uint32_t *rep;               // corners words: the corner's slot after the insert, its representative after the resolve
    uint32_t *block_totals;      // weld_blocks(corners) words
    int32_t *faces;              // [N][3]
    int32_t *first;              // [capacity]
    float *vertices;             // [capacity][3] or null
    uint32_t capacity;
    uint32_t *vertex_count;      // one word: V, stored or not
};

// Enqueues the table's fill with kWeldEmpty, insert, resolve + block totals, the offsets, number + scatter, and the gather of the
// other corners' ids: five launches and one memset in stream order, none of which waits for anything within a launch.
hipError_t launch_weld(const WeldArgs &args, hipStream_t stream);

enum class NormalWeight : int32_t { angle = 0, area = 1 };      // drt.h DRT_NORMALS_ANGLE / DRT_NORMALS_AREA

struct NormalsArgs {
    const float *vertices;       // [V][3]
    const int32_t *faces;        // [N][3]
    uint32_t n_vertices, n_tris;
    long long *acc;              // 3 V zeroed words: the fixed-point sums
    uint32_t *max_bits;          // one zeroed word: the bits of M (area weights)
    float *out;                  // [V][3]
};

hipError_t launch_vertex_normals(NormalWeight weight, const NormalsArgs &args, int num_cus, hipStream_t stream);

struct SmoothArgs {
    const float *src;            // [V][3]: the step's input positions p
    float *dst;                  // [V][3]: p'
    const int32_t *faces;        // [N][3]
    const uint8_t *fixed;        // [V] or null
    uint32_t n_vertices, n_tris;
    long long *acc;              // 3 V words, zeroed before every step, ...
    uint32_t *cnt;               // ... and V words behind them
    uint32_t *max_bits;          // two words: step s reads word s & 1, which the step before (or the first launch) has made, and
                                 // leaves the maximum of p' in the other one
    uint32_t step;
    float factor;
};

// The maximum of the first step's input into word 0 of max_bits (one launch).
hipError_t launch_smooth_maximum(const SmoothArgs &args, int num_cus, hipStream_t stream);
// One step: the sums over the triangles, then the update of every vertex (two launches; the caller zeroes acc and cnt first).
hipError_t launch_smooth_step(const SmoothArgs &args, int num_cus, hipStream_t stream);

// ---- the rules' integer arithmetic, for host and device ----
#ifdef __HIP__
#define DRT_WELD_HD __host__ __device__ __forceinline__
#else
#define DRT_WELD_HD inline
#endif

// drt.h "exponent": e = floor(log2 M) of a positive finite fp32 M given by its bits, denormals included (the double of an fp32
// value is always a normal number, so its exponent field is e + 1023)
DRT_WELD_HD int weld_exponent(uint32_t m_bits) {
    float m;
    __builtin_memcpy(&m, &m_bits, 4);
    const double d = (double)m;
    uint64_t b;
    __builtin_memcpy(&b, &d, 8);
    return (int)((b >> 52) & 0x7FFu) - 1023;
}
// 2^k as a double, -1022 <= k <= 1023
DRT_WELD_HD double weld_pow2(int k) {
    const uint64_t b = (uint64_t)(k + 1023) << 52;
    double d;
    __builtin_memcpy(&d, &b, 8);
    return d;
}
// drt.h "fixed point": (int64) trunc((double)x * scale); the product is exact, the conversion truncates towards zero
DRT_WELD_HD long long weld_fixed(float x, double scale) { return (long long)((double)x * scale); }

}  // namespace drt
