// kernel_isosurface.hip -- isosurface extraction for gfx950: marching tetrahedra over a float32 [Z][Y][X] field, one 48-byte triangle
// record per emitted triangle in ascending cube, tetrahedron and table order, the first cap_r of a row stored in the row's own segment
// of `out` (drt_renderer_isosurface).  The reference has no such call; include/drt.h states the rule, and every line below that
// computes a value cites the part of it that it implements (the tables are in isosurface.hpp).
//
//   samples    lattice index (i, j, k) lies at lo + ((float)idx + 0.5f) * cell per component; with a border the indices -1 and dims[k]
//              exist too and hold `border`
//   cubes      one per 2x2x2 block of neighbouring samples, corners c = dx + 2 dy + 4 dz, tetrahedra (0,1,3,7) (0,1,5,7) (0,2,3,7)
//              (0,2,6,7) (0,4,5,7) (0,4,6,7)
//   class      above iff f >= level; a tetrahedron with a corner that fails fabsf(f) <= FLT_MAX emits nothing
//   vertex     on a tetrahedron edge whose ends differ in class, from the end a with the smaller corner number to the other end b:
//              t = (level - fa) / (fb - fa), P = pa + (pb - pa) * t per component
//   triangles  the 16-row table by the 4-bit case (bit j: local vertex j above); vertices 1 and 2 change places in the mirror-image
//              tetrahedra 1, 2 and 5, and once more with flip
//   record     v[3][3], cube, code = tetrahedron | case << 4, 0; the miss record is cube = 0xffffffff and zeros
//   segment    drt_renderer_plane_sections': cap = offsets[r+1] > offsets[r] ? the difference : 0, clamped so that offsets[r] + cap <=
//              out_capacity; slots 0 .. min(cap, total) - 1 the list, the rest of the cap slots the miss record; counts[r] = total
//
// Shape: ONE WAVE PER ROW on a persistent grid -- a row is the run of cubes along x of one (y, z), and wave w takes rows w, w + waves,
// ...: every row costs the same loads, so there is nothing to claim and no atomic.  No two waves exchange data, and the workgroup
// (4 waves) is only a packaging: there is no barrier and no LDS.
//
// A step takes kIsoChunk = 63 cubes of the row.  Lane l loads the four samples of column x0 + l (dy, dz in {0, 1}: corners 0, 2, 4, 6
// of its cube); corners 1, 3, 5, 7 are the column of lane l + 1, and lane 63 lends its column and owns no cube.  The other choice -- 64
// cubes and a second, divergent load on lane 63 -- saves one lane in 64 and costs every step a second load instruction; the stride of
// 63 keeps one uniform, coalesced load per sample row.  A load's index is clamped into the grid and the value is replaced by `border`
// where the index was outside: an index test and a select, no branch.
//
// A lane packs its column's four classes and four finiteness bits into one word and receives the next lane's word by ONE cross-lane
// move.  A cube whose eight corners share a class emits nothing whatever else holds, so a step in which no cube is mixed ends right
// there (one ballot): most steps of a real field, in both passes.  Otherwise the two words give each tetrahedron's 4-bit case by fixed
// bit selections (a tetrahedron that is not finite has case 0), and the triangles of a case are (0x01210 >> 4 * popcount) & 3.
// Count pass: a lane adds up its cubes' triangles over the steps of the row, one wave reduction and one store end the row.
// Fill pass: an inclusive wave prefix sum of the lanes' counts behind a wave-uniform running total numbers the step's triangles in
// record order, so a row's records are in ascending x with no atomics and no sort.  The cubes that are cut are few -- two to four
// lanes of a row through a sphere -- so the triangles are dealt out again: triangle g of the step is computed by lane g % 64, which
// finds its source lane by a binary search over the prefix sums (six cross-lane moves with a per-lane source) and fetches that cube's
// eight samples, cases and base the same way.  All 64 lanes interpolate, and consecutive lanes write consecutive records, each as
// three 16-byte stores.  A row with no capacity (and no counts to write) is skipped as a whole.  After the last step the lanes stride
// over [min(total, cap), cap) with miss records.
//
// Registers: the compiler's resource remarks are recorded in DESIGN.md 5.32 (no scratch, no LDS).
#include <hip/hip_runtime.h>

#include "isosurface.hpp"

namespace drt {

namespace {

#define ISO_DEV __device__ __forceinline__

__device__ const uint32_t kIsoTable[16] = DRT_ISO_TABLE;

// inclusive prefix sum over the 64 lanes of the wave
ISO_DEV uint32_t iso_inclusive_sum(uint32_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)v, d);
        if (lane >= d) v += up;
    }
    return v;
}

ISO_DEV uint32_t iso_wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}

// one row of samples along x: the pointer to its first sample, clamped into the grid, and whether (iy, iz) was inside
struct IsoRow { const float *p; bool ok; };
ISO_DEV IsoRow iso_row(const IsoArgs &a, int iy, int iz) {
    const int iyc = min(max(iy, 0), (int)a.dims[1] - 1), izc = min(max(iz, 0), (int)a.dims[2] - 1);
    IsoRow r;
    r.p = a.field + ((size_t)izc * a.dims[1] + (size_t)iyc) * a.dims[0];
    r.ok = iy == iyc && iz == izc;
    return r;
}

// drt.h "class": fabsf(f) <= FLT_MAX
ISO_DEV bool iso_finite(float f) { return fabsf(f) <= 3.402823466e+38f; }

// drt.h "samples": lo + ((float)idx + 0.5f) * cell
ISO_DEV float iso_pos(float lo, float cell, int idx) { return lo + ((float)idx + 0.5f) * cell; }

// A column's mask: bits 0..3 the classes of its four samples (dy + 2 dz), bits 4..7 whether they are finite.  Corner c of a cube
// lies in the lane's own column (dx = 0) or in the next lane's (dx = 1), at bit c >> 1.
template <int C>
ISO_DEV uint32_t iso_corner(uint32_t own, uint32_t next, int shift) { return (((C & 1) ? next : own) >> ((C >> 1) + shift)) & 1u; }

// the 4-bit case of tetrahedron (0, B, C, 7) from the two column masks; 0 if a corner is not finite
template <int B, int C>
ISO_DEV uint32_t iso_case(uint32_t own, uint32_t next) {
    const uint32_t c = iso_corner<0>(own, next, 0) | iso_corner<B>(own, next, 0) << 1 | iso_corner<C>(own, next, 0) << 2 | iso_corner<7>(own, next, 0) << 3;
    const uint32_t fin = iso_corner<0>(own, next, 4) & iso_corner<B>(own, next, 4) & iso_corner<C>(own, next, 4) & iso_corner<7>(own, next, 4);
    return fin ? c : 0u;
}

// drt.h "triangles": one when one corner is alone in its class, two when the classes split two and two
ISO_DEV uint32_t iso_triangles(uint32_t c) { return (0x01210u >> (4 * __popc(c))) & 3u; }

struct IsoCube {
    float f0, f1, f2, f3, f4, f5, f6, f7;      // the samples by corner number
    float x0, x1, y0, y1, z0, z1;              // the positions of the two lattice planes per axis
};

// drt.h "vertex" on edge e of tetrahedron (0, B, C, 7): from local vertex p to local vertex q > p
ISO_DEV void iso_vertex(const IsoCube &q, uint32_t B, uint32_t C, float fB, float fC, float level, uint32_t e, float &x, float &y, float &z) {
    const uint32_t lp = e < 3u ? 0u : (e < 5u ? 1u : 2u), lq = e < 3u ? e + 1u : (e < 5u ? e - 1u : 3u);
    const uint32_t ca = lp == 0u ? 0u : (lp == 1u ? B : C), cb = lq == 1u ? B : (lq == 2u ? C : 7u);
    const float fa = lp == 0u ? q.f0 : (lp == 1u ? fB : fC), fb = lq == 1u ? fB : (lq == 2u ? fC : q.f7);
    const float ax = (ca & 1u) ? q.x1 : q.x0, ay = (ca & 2u) ? q.y1 : q.y0, az = (ca & 4u) ? q.z1 : q.z0;
    const float bx = (cb & 1u) ? q.x1 : q.x0, by = (cb & 2u) ? q.y1 : q.y0, bz = (cb & 4u) ? q.z1 : q.z0;
    const float t = (level - fa) / (fb - fa);
    x = ax + (bx - ax) * t; y = ay + (by - ay) * t; z = az + (bz - az) * t;
}

// One triangle of a cube: the j-th of the cube's list -- tetrahedron 0..5, then the table's triangle 0..1 -- as a record's three
// 16-byte words.  cases: the six 4-bit cases, tetrahedron T in bits 4 T .. 4 T + 3.  T picks its corners B and C and their samples by
// selects, so that a lane can compute any triangle of any cube of the step.
ISO_DEV void iso_triangle(const IsoCube &q, uint32_t cases, uint32_t j, bool flip, float level, uint32_t cube, float4 &w0, float4 &w1, float4 &w2) {
    const float f1 = q.f1, f2 = q.f2, f3 = q.f3, f4 = q.f4, f5 = q.f5, f6 = q.f6;     // (values, so that a select picks a register)
    uint32_t T = 0, cs = 0, k = 0;
    bool found = false;
#pragma unroll
    for (uint32_t t = 0; t < 6u; t++) {
        const uint32_t c = (cases >> (4u * t)) & 15u, nt = iso_triangles(c);
        const bool take = !found && j < nt;
        T = take ? t : T; cs = take ? c : cs; k = take ? j : k;
        found = found || take;
        j -= found ? 0u : nt;
    }
    const uint32_t row = kIsoTable[cs];
    const uint32_t tri = row >> (9u * k);
    const uint32_t B = DRT_ISO_TET_B(T), C = DRT_ISO_TET_C(T);
    const float fB = T < 2u ? f1 : (T < 4u ? f2 : f4), fC = C == 3u ? f3 : (C == 5u ? f5 : f6);
    const bool swap = (DRT_ISO_MIRROR(T)) != flip;            // mirror-image tetrahedra, and once more with flip
    const uint32_t e0 = tri & 7u, ea = (tri >> 3) & 7u, eb = (tri >> 6) & 7u;
    const uint32_t e1 = swap ? eb : ea, e2 = swap ? ea : eb;
    float v[9];
    iso_vertex(q, B, C, fB, fC, level, e0, v[0], v[1], v[2]);
    iso_vertex(q, B, C, fB, fC, level, e1, v[3], v[4], v[5]);
    iso_vertex(q, B, C, fB, fC, level, e2, v[6], v[7], v[8]);
    w0 = make_float4(v[0], v[1], v[2], v[3]);
    w1 = make_float4(v[4], v[5], v[6], v[7]);
    w2 = make_float4(v[8], __uint_as_float(cube), __uint_as_float(T | cs << 4), 0.f);
}

template <bool FILL>
__global__ __launch_bounds__(kIsoThreads) void iso_kernel(const IsoArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * kIsoThreads + threadIdx.x) >> 6;
    if (wave >= a.waves) return;                              // (wave-uniform: the grid is whole workgroups)
    const uint32_t nx = a.cubes[0], ny = a.cubes[1];
    const int X = (int)a.dims[0];

    for (uint32_t row = wave; row < a.rows; row += a.waves) {
        uint32_t base = 0, cap = 0;                           // the row's segment: out[base .. base + cap)
        if (FILL) {
            // cap = offsets[r+1] > offsets[r] ? the difference : 0, clamped so that offsets[r] + cap <= out_capacity
            const uint32_t o0 = a.offsets[row], o1 = a.offsets[row + 1u];
            base = o0;
            cap = o1 > o0 ? o1 - o0 : 0u;
            const uint32_t room = o0 < a.out_capacity ? a.out_capacity - o0 : 0u;
            cap = cap < room ? cap : room;
            if (cap == 0u && !a.counts) continue;             // nothing to store and nothing to report: the row costs two words
        }
        float4 *const seg = reinterpret_cast<float4 *>(a.out) + 3 * (size_t)base;
        const uint32_t cz = row / ny, cy = row - cz * ny;
        const int iy = (int)cy - a.pad, iz = (int)cz - a.pad; // the lattice index of the cubes' corner 0
        const IsoRow r00 = iso_row(a, iy, iz), r10 = iso_row(a, iy + 1, iz), r01 = iso_row(a, iy, iz + 1), r11 = iso_row(a, iy + 1, iz + 1);
        IsoCube q;
        q.y0 = iso_pos(a.lo[1], a.cell[1], iy); q.y1 = iso_pos(a.lo[1], a.cell[1], iy + 1);
        q.z0 = iso_pos(a.lo[2], a.cell[2], iz); q.z1 = iso_pos(a.lo[2], a.cell[2], iz + 1);

        uint32_t total = 0;                                   // FILL: triangles so far (wave-uniform); count: this lane's share
        for (uint32_t x0 = 0; x0 < nx; x0 += (uint32_t)kIsoChunk) {
            const uint32_t cx = x0 + (uint32_t)lane;
            const int ix = (int)cx - a.pad;
            const int ixc = min(max(ix, 0), X - 1);           // the load stays inside the grid ...
            const bool xin = ix == ixc;                       // ... and a sample from outside it reads `border`
            const float l0 = r00.p[ixc], l2 = r10.p[ixc], l4 = r01.p[ixc], l6 = r11.p[ixc];
            const float f0 = (xin && r00.ok) ? l0 : a.border, f2 = (xin && r10.ok) ? l2 : a.border;
            const float f4 = (xin && r01.ok) ? l4 : a.border, f6 = (xin && r11.ok) ? l6 : a.border;
            // class: above iff f >= level; finite iff fabsf(f) <= FLT_MAX -- of the lane's own column, and by one move of the next one's
            const uint32_t own = (f0 >= a.level ? 1u : 0u) | (f2 >= a.level ? 2u : 0u) | (f4 >= a.level ? 4u : 0u) | (f6 >= a.level ? 8u : 0u) |
                                 (iso_finite(f0) ? 16u : 0u) | (iso_finite(f2) ? 32u : 0u) | (iso_finite(f4) ? 64u : 0u) | (iso_finite(f6) ? 128u : 0u);
            const uint32_t next = (uint32_t)__shfl_down((int)own, 1);
            const bool owns = lane < kIsoChunk && cx < nx;
            // a cube whose corners are all below or all above emits nothing, finite or not: a step without a mixed cube ends here
            const uint32_t any = (own | next) & 15u, all = own & next & 15u;
            if (__ballot(owns && any != 0u && all != 15u) == 0ull) continue;
            const uint32_t c0 = iso_case<1, 3>(own, next), c1 = iso_case<1, 5>(own, next), c2 = iso_case<2, 3>(own, next),
                           c3 = iso_case<2, 6>(own, next), c4 = iso_case<4, 5>(own, next), c5 = iso_case<4, 6>(own, next);
            uint32_t n = iso_triangles(c0) + iso_triangles(c1) + iso_triangles(c2) + iso_triangles(c3) + iso_triangles(c4) + iso_triangles(c5);
            if (!owns) n = 0u;
            if (!FILL) { total += n; continue; }
            const uint32_t incl = iso_inclusive_sum(n, lane);
            const uint32_t step_total = (uint32_t)__shfl((int)incl, 63);
            if (total < cap && step_total != 0u) {            // the wave-uniform total is below the capacity: this step stores
                // Triangle g of the step goes to lane g % 64, whichever lane's cube it comes from: the lanes whose cubes are cut are
                // few, and this way all 64 compute and their records are neighbours in memory.  The source lane s is the first one
                // with incl[s] > g; its samples, cases and base come over by cross-lane moves with a per-lane source.
                const uint32_t cases = c0 | c1 << 4 | c2 << 8 | c3 << 12 | c4 << 16 | c5 << 20, excl = incl - n;
                const uint32_t room = cap - total;
                for (uint32_t g0 = 0; g0 < step_total && g0 < room; g0 += 64u) {
                    const uint32_t g = g0 + (uint32_t)lane;
                    int s = 0;
#pragma unroll
                    for (int b = 32; b >= 1; b >>= 1) {
                        const uint32_t v = (uint32_t)__shfl((int)incl, s + b - 1);
                        if (v <= g) s += b;
                    }
                    IsoCube t = q;                            // (y and z planes of the row)
                    t.f0 = __shfl(f0, s); t.f2 = __shfl(f2, s); t.f4 = __shfl(f4, s); t.f6 = __shfl(f6, s);
                    const int s1 = s < 63 ? s + 1 : 63;       // (lane 63 owns no cube: never a source)
                    t.f1 = __shfl(f0, s1); t.f3 = __shfl(f2, s1); t.f5 = __shfl(f4, s1); t.f7 = __shfl(f6, s1);
                    const uint32_t s_cases = (uint32_t)__shfl((int)cases, s), s_excl = (uint32_t)__shfl((int)excl, s);
                    const int sx = (int)(x0 + (uint32_t)s) - a.pad;
                    t.x0 = iso_pos(a.lo[0], a.cell[0], sx); t.x1 = iso_pos(a.lo[0], a.cell[0], sx + 1);
                    float4 w0, w1, w2;
                    iso_triangle(t, s_cases, g - s_excl, a.swap != 0, a.level, row * nx + x0 + (uint32_t)s, w0, w1, w2);
                    if (g < step_total && g < room) {
                        float4 *const rec = seg + 3 * ((size_t)total + g);
                        rec[0] = w0; rec[1] = w1; rec[2] = w2;
                    }
                }
            }
            total += step_total;
        }

        if (!FILL) {
            const uint32_t sum = iso_wave_sum(total);
            if (lane == 0) a.counts[row] = sum;
            continue;
        }
        // ---- the miss record behind the list, and the count ----
        const float4 miss = make_float4(0.f, __uint_as_float(0xFFFFFFFFu), 0.f, 0.f), zero = make_float4(0.f, 0.f, 0.f, 0.f);
        for (uint32_t j = (total < cap ? total : cap) + (uint32_t)lane; j < cap; j += 64u) {
            float4 *const rec = seg + 3 * (size_t)j;
            rec[0] = zero; rec[1] = zero; rec[2] = miss;
        }
        if (lane == 0 && a.counts) a.counts[row] = total;
    }
}

}  // namespace

hipError_t launch_isosurface(bool fill, const IsoArgs &args, hipStream_t stream) {
    if (args.rows == 0) return hipSuccess;
    const uint32_t blocks = (args.waves * 64u + kIsoThreads - 1) / kIsoThreads;
    if (fill) hipLaunchKernelGGL(iso_kernel<true>, dim3(blocks), dim3(kIsoThreads), 0, stream, args);
    else hipLaunchKernelGGL(iso_kernel<false>, dim3(blocks), dim3(kIsoThreads), 0, stream, args);
    return hipGetLastError();
}

}  // namespace drt
