// kernel_simplify.hip -- mesh simplification by vertex clustering for gfx950 (drt_renderer_simplify).  The reference has no such call;
// include/drt.h states the rule, and every line below that computes a value cites the part of it that it implements.  None of the
// kernels reads a scene or a tree.
//
//   clusters  insert   one lane per vertex: its key (simplify.hpp) into key[v]; an in-grid vertex then goes into an insert-only
//                      open-addressing table of vertex indices, hashed by pcg_hash over the key, linear probing.  A free slot is claimed
//                      with atomicCAS(slot, empty, v); a slot that holds a vertex of the same key takes atomicMin(slot, v); a slot of
//                      another key is passed.  Once claimed a slot's KEY never changes (only the index in it falls), so every vertex of
//                      one cell ends in the same slot whatever the order, and that slot ends holding the smallest of them.  The table is
//                      at most half full, so a probe always ends; a lane waits for no other lane's progress.  A vertex outside the grid
//                      skips the table: it is its own representative.
//             resolve  rep[v] = table[slot] (or v), the flag rep[v] == v, and the workgroup's total of them
//             offsets  ONE workgroup turns the block totals into exclusive offsets, a block at a trip with a running carry, and stores C
//             number   representative v is cluster id = offset + flags in front of it: ascending first; cluster[v] and first[id]
//             gather   every other vertex copies cluster[rep[v]]
//   sums      maximum  (quadric) one atomicMax per wave on the bits of the largest l of the contributing triangles
//             vertices one lane per in-grid vertex: cnt[c] += 1 and three 64-bit integer adds of r
//             corners  (quadric) one lane per triangle: nine 64-bit integer adds per corner in a cluster of several members
//             Integer sums are the same bytes in any order and in any grouping; float atomics are not.  Both launches combine runs
//             of neighbouring lanes that name one cluster across the wave before the atomic (simplify_run_sums): on a remeshed
//             surface at 4:1 and 8:1 per axis that is 3.0 and 4.4 times as fast as one atomic per term, which
//             DRT_SIMPLIFY_SUMS=plain still selects, for measuring.
//   finish             one lane per stored cluster: a copy of its only member, or the float64 solve of drt.h in the order written there
//   faces     flags    keep[t], block totals; the same offsets launch stores M; the scatter of out_faces and source
//   The three-launch scan is kernel_weld.hip's shape: no look-back, no flag, no spin.
//
// Registers: the compiler's resource remarks are recorded in DESIGN.md 5.34 (no scratch).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_math.hpp"
#include "simplify.hpp"

namespace drt {

namespace {

#define SIMP_DEV __device__ __forceinline__

__global__ __launch_bounds__(kSimplifyThreads) void simplify_insert_kernel(const SimplifyArgs a) {
    const uint32_t v = blockIdx.x * kSimplifyThreads + threadIdx.x;
    if (v >= a.n_vertices) return;
    const f3 p = ld3(a.vertices + 3 * (size_t)v);
    const uint32_t key = simplify_key(a.grid, p.x, p.y, p.z);
    a.key[v] = key;
    if (key == kSimplifyOutside) return;                                        // a cluster of its own: rep[v] is not read
    uint32_t slot = pcg_hash(key) & a.mask;
    // at most mask + 1 probes: the table holds at most V <= (mask + 1) / 2 keys, so a free or an equal slot comes first.  The key of
    // the vertex a slot holds is made again from its position, an input: key[held] is another lane's store of this launch
    for (uint32_t tries = 0; tries <= a.mask; tries++) {
        const uint32_t held = atomicCAS(&a.table[slot], kSimplifyEmpty, v);
        if (held == kSimplifyEmpty) break;                                      // claimed
        const f3 q = ld3(a.vertices + 3 * (size_t)held);                        // (held < V: a vertex index; its key again from its position)
        if (simplify_key(a.grid, q.x, q.y, q.z) == key) { atomicMin(&a.table[slot], v); break; }
        slot = (slot + 1u) & a.mask;
    }
    a.rep[v] = slot;
}

// inclusive sum of v over the workgroup's kSimplifyScanBlock threads: a wave scan, then the four wave totals through LDS
SIMP_DEV uint32_t simplify_block_inclusive(uint32_t v, uint32_t *s_wave) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)v, d);
        if (lane >= d) v += up;
    }
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    uint32_t before = 0;
#pragma unroll
    for (int w = 0; w < kSimplifyThreads / 64; w++) before += w < wave ? s_wave[w] : 0u;
    __syncthreads();                                                            // s_wave is free again
    return before + v;
}

__global__ __launch_bounds__(kSimplifyThreads) void simplify_resolve_kernel(const SimplifyArgs a) {
    __shared__ uint32_t s_wave[kSimplifyThreads / 64];
    const uint32_t v = blockIdx.x * kSimplifyScanBlock + threadIdx.x;
    uint32_t flag = 0;
    if (v < a.n_vertices) {
        const uint32_t rep = a.key[v] == kSimplifyOutside ? v : a.table[a.rep[v]];     // the smallest vertex of v's cell, or v itself
        a.rep[v] = rep;
        flag = rep == v ? 1u : 0u;
    }
    const uint32_t incl = simplify_block_inclusive(flag, s_wave);
    if (threadIdx.x == kSimplifyScanBlock - 1) a.block_totals[blockIdx.x] = incl;
}

__global__ __launch_bounds__(kSimplifyThreads) void simplify_offsets_kernel(uint32_t *block_totals, uint32_t n_blocks, uint32_t *total) {
    __shared__ uint32_t s_wave[kSimplifyThreads / 64];
    __shared__ uint32_t s_total;
    uint32_t carry = 0;                                                         // (the same in every thread)
    for (uint32_t base = 0; base < n_blocks; base += kSimplifyScanBlock) {
        const uint32_t b = base + threadIdx.x;
        const uint32_t v = b < n_blocks ? block_totals[b] : 0u;
        const uint32_t incl = simplify_block_inclusive(v, s_wave);
        if (b < n_blocks) block_totals[b] = carry + (incl - v);                 // exclusive: the flags in front of block b
        if (threadIdx.x == kSimplifyScanBlock - 1) s_total = incl;
        __syncthreads();
        carry += s_total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;                                       // C or M, stored or not
}

__global__ __launch_bounds__(kSimplifyThreads) void simplify_number_kernel(const SimplifyArgs a) {
    __shared__ uint32_t s_wave[kSimplifyThreads / 64];
    const uint32_t v = blockIdx.x * kSimplifyScanBlock + threadIdx.x;
    const bool is_rep = v < a.n_vertices && a.rep[v] == v;
    const uint32_t incl = simplify_block_inclusive(is_rep ? 1u : 0u, s_wave);
    if (!is_rep) return;
    const uint32_t id = a.block_totals[blockIdx.x] + incl - 1u;                 // clusters are numbered in ascending first
    a.cluster[v] = (int32_t)id;
    if (id < a.vertex_capacity) a.first[id] = (int32_t)v;                       // a smaller capacity stores the first `capacity` clusters
}

__global__ __launch_bounds__(kSimplifyThreads) void simplify_gather_kernel(const SimplifyArgs a) {
    const uint32_t v = blockIdx.x * kSimplifyThreads + threadIdx.x;
    if (v >= a.n_vertices) return;
    const uint32_t rep = a.rep[v];
    if (rep != v) a.cluster[v] = a.cluster[rep];                                // (cluster[rep] is the launch before's; no lane writes it here)
}

// ------------------------------------------------------------------ the sums

SIMP_DEV bool simplify_finite3(f3 v) { return simplify_finite(v.x) && simplify_finite(v.y) && simplify_finite(v.z); }
SIMP_DEV void simplify_add(long long *p, long long v) { atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v); }

// the cell indices of a key
SIMP_DEV void simplify_unpack(const SimplifyGrid &g, uint32_t key, uint32_t &ix, uint32_t &iy, uint32_t &iz) {
    const uint32_t yz = key / g.dims[0];
    ix = key - yz * g.dims[0];
    iz = yz / g.dims[1];
    iy = yz - iz * g.dims[1];
}

// drt.h "position of a cluster": the centre g of the cell of `key`
SIMP_DEV f3 simplify_cell_centre(const SimplifyGrid &g, uint32_t key) {
    uint32_t ix, iy, iz;
    simplify_unpack(g, key, ix, iy, iz);
    return mk3(simplify_centre(g.lo[0], g.cell[0], ix), simplify_centre(g.lo[1], g.cell[1], iy), simplify_centre(g.lo[2], g.cell[2], iz));
}

// r = (p - g) / cell per component in fp32
SIMP_DEV f3 simplify_offset(const SimplifyGrid &g, uint32_t key, f3 p) {
    const f3 c = simplify_cell_centre(g, key);
    return mk3((p.x - c.x) / g.cell[0], (p.y - c.y) / g.cell[1], (p.z - c.z) / g.cell[2]);
}

// a triangle's indices, positions and normal; false if it contributes nothing: an index outside [0, V) (a bounds check), a coordinate
// that is not finite, or l = sqrtf(dot(n, n)) that is 0 or not finite
struct SimplifyTri { uint32_t i[3]; f3 v[3]; f3 n; float l; };
SIMP_DEV bool simplify_triangle(const SimplifyArgs &a, uint32_t t, SimplifyTri &tri) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        tri.i[k] = (uint32_t)a.faces[3 * (size_t)t + k];                        // (a negative index is a large unsigned one)
        ok = ok && tri.i[k] < a.n_vertices;
    }
    if (!ok) return false;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        tri.v[k] = ld3(a.vertices + 3 * (size_t)tri.i[k]);
        ok = ok && simplify_finite3(tri.v[k]);
    }
    if (!ok) return false;
    tri.n = cross(tri.v[1] - tri.v[0], tri.v[2] - tri.v[0]);
    tri.l = sqrtf(dot(tri.n, tri.n));
    return tri.l > 0.0f && simplify_finite(tri.l);                              // (a NaN fails the first test)
}

uint32_t grid_for(uint32_t n, int num_cus) {                                    // enough workgroups for every item, at most 8 per CU
    const uint32_t want = (n + kSimplifyThreads - 1) / kSimplifyThreads;
    return std::max<uint32_t>(1, std::min<uint32_t>(want, (uint32_t)std::max(1, num_cus) * 8u));
}

__global__ __launch_bounds__(kSimplifyThreads) void simplify_maximum_kernel(const SimplifyArgs a) {
    const uint32_t stride = gridDim.x * kSimplifyThreads;
    uint32_t best = 0;
    for (uint32_t t = blockIdx.x * kSimplifyThreads + threadIdx.x; t < a.n_tris; t += stride) {
        SimplifyTri tri;
        if (simplify_triangle(a, t, tri)) best = max(best, __float_as_uint(tri.l));     // (l > 0: the bits order as the values do)
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, d));
    if ((threadIdx.x & 63) == 0 && best) atomicMax(a.max_bits, best);           // one atomic per wave
}

// The run-combining form of the sums (RUNS, the default): neighbouring lanes of a wave often name the same cluster, so a run of lanes
// with equal cluster ids adds its terms across lanes first and its first lane issues one atomic per word.  Integer sums are the same bytes
// however they are grouped.  Every lane of the wave calls this (inactive lanes are runs of their own that add nothing); on return
// `head` is set in the first lane of every active run, whose v holds the run's sums.  Cross-lane moves only: no LDS, no waiting.
template <int W>
SIMP_DEV bool simplify_run_sums(bool active, uint32_t c, long long (&v)[W]) {
    const int lane = (int)__lane_id();
    const uint32_t id = active ? c : kSimplifyEmpty;                            // (no cluster id reaches it: C <= V < 2^31)
    const uint32_t before = (uint32_t)__shfl_up((int)id, 1);
    const bool starts = lane == 0 || before != id || !active;
    const unsigned long long starts_mask = __ballot(starts);
    if (starts_mask != ~0ull) {                                                 // (wave-uniform) some run is longer than one lane
        const int run = __popcll(starts_mask & (~0ull >> (63 - lane)));         // the runs are contiguous: their numbers ascend
        for (int d = 1; d < 64; d <<= 1) {
            const int run_there = __shfl_down(run, d);                          // (every lane takes part: a lane that sat out would read as 0)
            const bool joins = lane + d < 64 && run_there == run;
            if (!__any(joins)) break;                                           // no run reaches d lanes: none reaches more
#pragma unroll
            for (int w = 0; w < W; w++) {
                const long long other = __shfl_down(v[w], d);
                if (joins) v[w] += other;
            }
        }
    }
    return starts && active;
}

template <bool RUNS>
__global__ __launch_bounds__(kSimplifyThreads) void simplify_vertex_sums_kernel(const SimplifyArgs a, const int words) {
    const uint32_t stride = gridDim.x * kSimplifyThreads;
    for (uint32_t base = blockIdx.x * kSimplifyThreads; base < a.n_vertices; base += stride) {      // (wave-uniform trips)
        const uint32_t v = base + threadIdx.x;
        const uint32_t key = v < a.n_vertices ? a.key[v] : kSimplifyOutside;
        const bool active = key != kSimplifyOutside;                            // outside: cnt stays 0 and the finish copies the vertex
        uint32_t c = 0;
        long long q[4] = {0, 0, 0, 1};                                          // r, and the member itself
        if (active) {
            c = (uint32_t)a.cluster[v];
            const f3 r = simplify_offset(a.grid, key, ld3(a.vertices + 3 * (size_t)v));
            q[0] = simplify_fixed(r.x); q[1] = simplify_fixed(r.y); q[2] = simplify_fixed(r.z);
        }
        if (RUNS ? simplify_run_sums(active, c, q) : active) {
            long long *acc = a.sums + (size_t)words * c;
            atomicAdd(&a.cnt[c], (uint32_t)q[3]);
            simplify_add(acc + 0, q[0]); simplify_add(acc + 1, q[1]); simplify_add(acc + 2, q[2]);
        }
    }
}

template <bool RUNS>
__global__ __launch_bounds__(kSimplifyThreads) void simplify_corner_sums_kernel(const SimplifyArgs a) {
    const uint32_t stride = gridDim.x * kSimplifyThreads;
    const uint32_t l_bits = *a.max_bits;
    if (l_bits == 0u) return;                                                   // no contributing triangle
    const double scale = weld_pow2(-(weld_exponent(l_bits) + 1));               // 2^-(e + 1), e = floor(log2 L)
    for (uint32_t base = blockIdx.x * kSimplifyThreads; base < a.n_tris; base += stride) {          // (wave-uniform trips)
        const uint32_t t = base + threadIdx.x;
        SimplifyTri tri;
        const bool ok = t < a.n_tris && simplify_triangle(a, t, tri);
        f3 u = mk3(0.0f, 0.0f, 0.0f), wu = u;
        long long qa[6] = {0, 0, 0, 0, 0, 0};
        if (ok) {
            u = mk3(tri.n.x / tri.l, tri.n.y / tri.l, tri.n.z / tri.l);         // three divisions
            const float w = (float)((double)tri.l * scale);                     // the power of two in float64 (exact), one rounding to fp32
            wu = mk3(w * u.x, w * u.y, w * u.z);
            qa[0] = simplify_fixed(wu.x * u.x); qa[1] = simplify_fixed(wu.x * u.y); qa[2] = simplify_fixed(wu.x * u.z);
            qa[3] = simplify_fixed(wu.y * u.y); qa[4] = simplify_fixed(wu.y * u.z); qa[5] = simplify_fixed(wu.z * u.z);
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            bool active = false;
            uint32_t c = 0;
            long long q[9] = {qa[0], qa[1], qa[2], qa[3], qa[4], qa[5], 0, 0, 0};
            if (ok) {
                const uint32_t key = a.key[tri.i[k]];
                if (key != kSimplifyOutside) {
                    c = (uint32_t)a.cluster[tri.i[k]];
                    active = a.cnt[c] > 1u;                                     // one member: its position is copied
                    if (active) {
                        const float s = dot(u, simplify_offset(a.grid, key, tri.v[k]));
                        q[6] = simplify_fixed(wu.x * s); q[7] = simplify_fixed(wu.y * s); q[8] = simplify_fixed(wu.z * s);
                    }
                }
            }
            if (RUNS ? simplify_run_sums(active, c, q) : active) {
                long long *dst = a.sums + (size_t)kSimplifyWords * c + kSimplifyMeanWords;
#pragma unroll
                for (int w = 0; w < 9; w++) simplify_add(dst + w, q[w]);
            }
        }
    }
}

template <bool QUADRIC>
__global__ __launch_bounds__(kSimplifyThreads) void simplify_finish_kernel(const SimplifyArgs a) {
    const uint32_t stride = gridDim.x * kSimplifyThreads;
    const uint32_t stored = min(a.counts[0], a.vertex_capacity);
    constexpr int words = QUADRIC ? kSimplifyWords : kSimplifyMeanWords;
    for (uint32_t c = blockIdx.x * kSimplifyThreads + threadIdx.x; c < stored; c += stride) {
        const uint32_t v = (uint32_t)a.first[c];
        const uint32_t key = a.key[v];
        const uint32_t cnt = a.cnt[c];
        const f3 p = ld3(a.vertices + 3 * (size_t)v);
        float *o = a.out_vertices + 3 * (size_t)c;
        if (key == kSimplifyOutside || cnt <= 1u) {                             // one member: its 12 bytes
            o[0] = p.x; o[1] = p.y; o[2] = p.z;
            continue;
        }
        const long long *S = a.sums + (size_t)words * c;
        const double den = (double)cnt * 0x1p30;
        const double m0 = (double)S[0] / den, m1 = (double)S[1] / den, m2 = (double)S[2] / den;   // m = (double)acc / ((double)cnt * 2^30)
        double x0 = m0, x1 = m1, x2 = m2;
        if (QUADRIC) {
            const double A00 = (double)S[3], A01 = (double)S[4], A02 = (double)S[5], A11 = (double)S[6], A12 = (double)S[7], A22 = (double)S[8];
            const double tr = (A00 + A11) + A22;
            const double lam = tr * 0x1p-10;
            const double a00 = A00 + lam, a11 = A11 + lam, a22 = A22 + lam, a01 = A01, a02 = A02, a12 = A12;
            const double d0 = (double)S[9] + lam * m0, d1 = (double)S[10] + lam * m1, d2 = (double)S[11] + lam * m2;
            const double c0 = a11 * a22 - a12 * a12;
            const double c1 = a01 * a22 - a12 * a02;
            const double c2 = a01 * a12 - a11 * a02;
            const double det = (a00 * c0 - a01 * c1) + a02 * c2;
            const double e0 = d1 * a22 - a12 * d2;
            const double e1 = d1 * a12 - a11 * d2;
            const double e2 = a01 * d2 - d1 * a02;
            const double q0 = ((d0 * c0 - a01 * e0) + a02 * e1) / det;
            const double q1 = ((a00 * e0 - d0 * c1) + a02 * e2) / det;
            const double q2 = ((d0 * c2 - a00 * e1) - a01 * e2) / det;
            // an optimum outside its cell is not trusted (a NaN or an infinity fails the comparisons)
            if (tr != 0.0 && __builtin_fabs(q0) <= 0.5 && __builtin_fabs(q1) <= 0.5 && __builtin_fabs(q2) <= 0.5) { x0 = q0; x1 = q1; x2 = q2; }
        }
        const f3 g = simplify_cell_centre(a.grid, key);
        o[0] = (float)((double)g.x + x0 * (double)a.grid.cell[0]);
        o[1] = (float)((double)g.y + x1 * (double)a.grid.cell[1]);
        o[2] = (float)((double)g.z + x2 * (double)a.grid.cell[2]);
    }
}

// ------------------------------------------------------------------ the triangles

// drt.h "triangles": t survives iff its three indices are in [0, V) and its three cluster ids differ pairwise
SIMP_DEV bool simplify_keep(const SimplifyArgs &a, uint32_t t, int32_t id[3]) {
    if (t >= a.n_tris) return false;
    bool ok = true;
    uint32_t i[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        i[k] = (uint32_t)a.faces[3 * (size_t)t + k];
        ok = ok && i[k] < a.n_vertices;
    }
    if (!ok) return false;
#pragma unroll
    for (int k = 0; k < 3; k++) id[k] = a.cluster[i[k]];
    return id[0] != id[1] && id[1] != id[2] && id[2] != id[0];
}

__global__ __launch_bounds__(kSimplifyThreads) void simplify_face_flags_kernel(const SimplifyArgs a) {
    __shared__ uint32_t s_wave[kSimplifyThreads / 64];
    int32_t id[3];
    const uint32_t flag = simplify_keep(a, blockIdx.x * kSimplifyScanBlock + threadIdx.x, id) ? 1u : 0u;
    const uint32_t incl = simplify_block_inclusive(flag, s_wave);
    if (threadIdx.x == kSimplifyScanBlock - 1) a.block_totals[blockIdx.x] = incl;
}

__global__ __launch_bounds__(kSimplifyThreads) void simplify_face_scatter_kernel(const SimplifyArgs a) {
    __shared__ uint32_t s_wave[kSimplifyThreads / 64];
    const uint32_t t = blockIdx.x * kSimplifyScanBlock + threadIdx.x;
    int32_t id[3];
    const bool keep = simplify_keep(a, t, id);
    const uint32_t incl = simplify_block_inclusive(keep ? 1u : 0u, s_wave);
    if (!keep) return;
    const uint32_t m = a.block_totals[blockIdx.x] + incl - 1u;                  // survivors keep input order
    if (m >= a.tri_capacity) return;                                            // a smaller capacity stores the first `capacity` triangles
    a.out_faces[3 * (size_t)m] = id[0]; a.out_faces[3 * (size_t)m + 1] = id[1]; a.out_faces[3 * (size_t)m + 2] = id[2];
    a.source[m] = (int32_t)t;
}

}  // namespace

hipError_t launch_simplify(SimplifyPlacement placement, const SimplifyArgs &args, int num_cus, hipStream_t stream) {
    static_assert(kSimplifyScanBlock == (uint32_t)kSimplifyThreads, "one item per thread");
    const bool quadric = placement == SimplifyPlacement::quadric;
    const int words = quadric ? kSimplifyWords : kSimplifyMeanWords;
    const uint32_t v_blocks = simplify_blocks(args.n_vertices);
    const dim3 block(kSimplifyThreads);
    hipError_t e = hipMemsetAsync(args.table, 0xFF, ((size_t)args.mask + 1) * sizeof(uint32_t), stream);         // kSimplifyEmpty
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(simplify_insert_kernel, dim3(v_blocks), block, 0, stream, args);
    hipLaunchKernelGGL(simplify_resolve_kernel, dim3(v_blocks), block, 0, stream, args);
    hipLaunchKernelGGL(simplify_offsets_kernel, dim3(1), block, 0, stream, args.block_totals, v_blocks, args.counts);
    hipLaunchKernelGGL(simplify_number_kernel, dim3(v_blocks), block, 0, stream, args);
    hipLaunchKernelGGL(simplify_gather_kernel, dim3(v_blocks), block, 0, stream, args);
    if (args.vertex_capacity) {                                                 // no stored vertex: no position is wanted
        if (quadric && args.n_tris) hipLaunchKernelGGL(simplify_maximum_kernel, dim3(grid_for(args.n_tris, num_cus)), block, 0, stream, args);
        const dim3 v_grid(grid_for(args.n_vertices, num_cus)), t_grid(grid_for(std::max(args.n_tris, 1u), num_cus));
        if (args.combine_runs) hipLaunchKernelGGL(simplify_vertex_sums_kernel<true>, v_grid, block, 0, stream, args, words);
        else hipLaunchKernelGGL(simplify_vertex_sums_kernel<false>, v_grid, block, 0, stream, args, words);
        if (quadric && args.n_tris) {
            if (args.combine_runs) hipLaunchKernelGGL(simplify_corner_sums_kernel<true>, t_grid, block, 0, stream, args);
            else hipLaunchKernelGGL(simplify_corner_sums_kernel<false>, t_grid, block, 0, stream, args);
        }
        const dim3 grid(grid_for(std::min(args.n_vertices, args.vertex_capacity), num_cus));
        if (quadric) hipLaunchKernelGGL(simplify_finish_kernel<true>, grid, block, 0, stream, args);
        else hipLaunchKernelGGL(simplify_finish_kernel<false>, grid, block, 0, stream, args);
    }
    if (args.n_tris) {
        const uint32_t t_blocks = simplify_blocks(args.n_tris);
        hipLaunchKernelGGL(simplify_face_flags_kernel, dim3(t_blocks), block, 0, stream, args);
        hipLaunchKernelGGL(simplify_offsets_kernel, dim3(1), block, 0, stream, args.block_totals, t_blocks, args.counts + 1);
        hipLaunchKernelGGL(simplify_face_scatter_kernel, dim3(t_blocks), block, 0, stream, args);
    } else {
        e = hipMemsetAsync(args.counts + 1, 0, sizeof(uint32_t), stream);
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

}  // namespace drt
