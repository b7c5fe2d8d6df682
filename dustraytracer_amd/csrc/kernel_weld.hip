// kernel_weld.hip -- vertex welding, vertex normals and Laplacian / Taubin smoothing for gfx950 (drt_renderer_weld,
// drt_renderer_vertex_normals, drt_renderer_smooth_vertices).  The reference has no such calls; include/drt.h states the rules, and
// every line below that computes a value cites the part of it that it implements.  None of the kernels reads a scene or a tree.
//
//   weld     insert   one lane per corner c = 3 t + k: an insert-only open-addressing table of corner indices, hashed by pcg_hash over
//                     the position's three words, linear probing.  A free slot is claimed with atomicCAS(slot, empty, c); a slot that
//                     holds a corner of the same bits takes atomicMin(slot, c); a slot of another position is passed.  Once claimed a
//                     slot's POSITION never changes (only the index in it falls), so every corner of one position ends in the same
//                     slot whatever the order, and that slot ends holding the smallest of them.  The table is at most half full, so
//                     a probe always ends; a lane waits for no other lane's progress.  The slot found is kept in rep[c].
//            resolve  rep[c] = table[rep[c]], the smallest corner with c's bits; the flag rep[c] == c marks the representatives, and
//                     workgroup b stores how many of its kWeldScanBlock corners are one
//            offsets  ONE workgroup turns the block totals into exclusive offsets, a block at a trip with a running carry, and stores V
//            number   workgroup b scans its flags again behind its offset: representative c is vertex id = offset + flags in front of
//                     it, which is ascending rep order; it writes faces[c], first[id] and vertices[id] (the last two while id < capacity)
//            gather   every other corner copies faces[rep[c]]
//            The three-launch scan is kernel_surface.hip's shape: no look-back, no flag, no spin.  Everything is integers, so the
//            result is the same bytes whatever the launch shape; the hash decides nothing that can be observed.
//   normals  maximum  (area weights) one atomicMax on the bits of the largest |n_j| of the contributing triangles
//            sums     one lane per triangle: nine 64-bit integer atomic adds of fixed-point terms -- integer sums are the same bytes in
//                     any order, float atomics are not
//            finish   one lane per vertex: x / sqrt(x x + y y + z z) in float64, rounded once
//   smooth   maximum  the largest finite |coordinate| of the first step's input, as above
//            sums     one lane per triangle: nine 64-bit adds of q(p) and three 32-bit adds of 2
//            update   one lane per vertex: p' from acc and cnt in float64, and the maximum of p' for the next step in the other word
//
// Registers: the compiler's resource remarks are recorded in DESIGN.md 5.33 (no scratch).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_math.hpp"
#include "weld.hpp"
#include "winding.hpp"

namespace drt {

namespace {

#define WELD_DEV __device__ __forceinline__

struct WeldKey { uint32_t x, y, z; };

// corner c = 3 t + k: the three words at tris + t * stride + 12 k
WELD_DEV WeldKey weld_key(const WeldArgs &a, uint32_t c) {
    const uint32_t t = c / 3u, k = c - 3u * t;
    const uint32_t *p = reinterpret_cast<const uint32_t *>(a.tris + (size_t)t * a.stride + 12u * k);
    WeldKey key;
    key.x = p[0]; key.y = p[1]; key.z = p[2];
    return key;
}

// drt.h "same vertex": the three 32-bit words equal as integers
WELD_DEV bool weld_same(WeldKey p, WeldKey q) { return p.x == q.x && p.y == q.y && p.z == q.z; }

__global__ __launch_bounds__(kWeldThreads) void weld_insert_kernel(const WeldArgs a) {
    const uint32_t c = blockIdx.x * kWeldThreads + threadIdx.x;
    if (c >= a.corners) return;
    const WeldKey key = weld_key(a, c);
    uint32_t slot = pcg_hash(key.x ^ pcg_hash(key.y ^ pcg_hash(key.z))) & a.mask;
    // at most mask + 1 probes: the table holds at most corners <= (mask + 1) / 2 positions, so a free or an equal slot comes first
    for (uint32_t tries = 0; tries <= a.mask; tries++) {
        const uint32_t held = atomicCAS(&a.table[slot], kWeldEmpty, c);
        if (held == kWeldEmpty) break;                                          // claimed
        if (weld_same(weld_key(a, held), key)) { atomicMin(&a.table[slot], c); break; }   // (held < corners: a corner index)
        slot = (slot + 1u) & a.mask;
    }
    a.rep[c] = slot;
}

// inclusive sum of v over the workgroup's kWeldScanBlock threads: a wave scan, then the four wave totals through LDS
WELD_DEV uint32_t weld_block_inclusive(uint32_t v, uint32_t *s_wave) {
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
    for (int w = 0; w < kWeldThreads / 64; w++) before += w < wave ? s_wave[w] : 0u;
    __syncthreads();                                                            // s_wave is free again
    return before + v;
}

__global__ __launch_bounds__(kWeldThreads) void weld_resolve_kernel(const WeldArgs a) {
    __shared__ uint32_t s_wave[kWeldThreads / 64];
    const uint32_t c = blockIdx.x * kWeldScanBlock + threadIdx.x;
    uint32_t flag = 0;
    if (c < a.corners) {
        const uint32_t rep = a.table[a.rep[c]];                                 // rep[c]: the smallest corner index with c's position
        a.rep[c] = rep;
        flag = rep == c ? 1u : 0u;
    }
    const uint32_t incl = weld_block_inclusive(flag, s_wave);
    if (threadIdx.x == kWeldScanBlock - 1) a.block_totals[blockIdx.x] = incl;
}

__global__ __launch_bounds__(kWeldThreads) void weld_offsets_kernel(uint32_t *block_totals, uint32_t n_blocks, uint32_t *vertex_count) {
    __shared__ uint32_t s_wave[kWeldThreads / 64];
    uint32_t carry = 0;                                                         // (the same in every thread)
    for (uint32_t base = 0; base < n_blocks; base += kWeldScanBlock) {
        const uint32_t b = base + threadIdx.x;
        const uint32_t v = b < n_blocks ? block_totals[b] : 0u;
        const uint32_t incl = weld_block_inclusive(v, s_wave);
        if (b < n_blocks) block_totals[b] = carry + (incl - v);                 // exclusive: the representatives in front of block b
        __shared__ uint32_t s_total;
        if (threadIdx.x == kWeldScanBlock - 1) s_total = incl;
        __syncthreads();
        carry += s_total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *vertex_count = carry;                                // V, stored or not
}

__global__ __launch_bounds__(kWeldThreads) void weld_number_kernel(const WeldArgs a) {
    __shared__ uint32_t s_wave[kWeldThreads / 64];
    const uint32_t c = blockIdx.x * kWeldScanBlock + threadIdx.x;
    const bool is_rep = c < a.corners && a.rep[c] == c;
    const uint32_t incl = weld_block_inclusive(is_rep ? 1u : 0u, s_wave);
    if (!is_rep) return;
    const uint32_t id = a.block_totals[blockIdx.x] + incl - 1u;                 // vertices are numbered in ascending rep
    a.faces[c] = (int32_t)id;
    if (id < a.capacity) {                                                      // a smaller capacity stores the first `capacity` vertices
        a.first[id] = (int32_t)c;
        if (a.vertices) {
            const WeldKey key = weld_key(a, c);                                 // copied bit for bit
            uint32_t *v = reinterpret_cast<uint32_t *>(a.vertices) + 3 * (size_t)id;
            v[0] = key.x; v[1] = key.y; v[2] = key.z;
        }
    }
}

__global__ __launch_bounds__(kWeldThreads) void weld_gather_kernel(const WeldArgs a) {
    const uint32_t c = blockIdx.x * kWeldThreads + threadIdx.x;
    if (c >= a.corners) return;
    const uint32_t rep = a.rep[c];
    if (rep != c) a.faces[c] = a.faces[rep];                                    // (faces[rep] is the launch before's; no lane writes it here)
}

// ------------------------------------------------------------------ normals and smoothing: what both read of a triangle

WELD_DEV bool weld_finite(float f) { return __builtin_fabsf(f) <= 3.402823466e+38f; }
WELD_DEV bool weld_finite3(f3 v) { return weld_finite(v.x) && weld_finite(v.y) && weld_finite(v.z); }
WELD_DEV void weld_add(long long *p, long long v) { atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v); }

// a triangle's indices and positions; false if an index is outside [0, V) (a bounds check) or a coordinate is not finite
struct WeldTri { uint32_t i[3]; f3 v[3]; };
WELD_DEV bool weld_triangle(const float *vertices, const int32_t *faces, uint32_t n_vertices, uint32_t t, WeldTri &tri) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        tri.i[k] = (uint32_t)faces[3 * (size_t)t + k];                          // (a negative index is a large unsigned one)
        ok = ok && tri.i[k] < n_vertices;
    }
    if (!ok) return false;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        tri.v[k] = ld3(vertices + 3 * (size_t)tri.i[k]);
        ok = ok && weld_finite3(tri.v[k]);
    }
    return ok;
}

// workgroup maximum of `best` into *word by one atomicMax on the bits (values >= +0: the bits order as the values do)
WELD_DEV void weld_fold_maximum(uint32_t best, uint32_t *word) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, d));
    if ((threadIdx.x & 63) == 0 && best) atomicMax(word, best);
}

// drt.h "normals": n = cross(v1 - v0, v2 - v0), l = sqrt(dot(n, n)); false if the triangle adds nothing
WELD_DEV bool weld_normal(const WeldTri &tri, f3 &n, float &l) {
    n = cross(tri.v[1] - tri.v[0], tri.v[2] - tri.v[0]);
    l = sqrtf(dot(n, n));
    return l != 0.0f && weld_finite(l);                                         // (a NaN fails the second test)
}

__global__ __launch_bounds__(kWeldThreads) void normals_maximum_kernel(const NormalsArgs a) {
    const uint32_t stride = gridDim.x * kWeldThreads;
    uint32_t best = 0;
    for (uint32_t t = blockIdx.x * kWeldThreads + threadIdx.x; t < a.n_tris; t += stride) {
        WeldTri tri;
        f3 n;
        float l;
        if (!weld_triangle(a.vertices, a.faces, a.n_vertices, t, tri) || !weld_normal(tri, n, l)) continue;
        const float m = fmaxf(fmaxf(__builtin_fabsf(n.x), __builtin_fabsf(n.y)), __builtin_fabsf(n.z));     // (l finite: so is every n_j)
        best = max(best, __float_as_uint(m));
    }
    weld_fold_maximum(best, a.max_bits);
}

template <bool AREA>
__global__ __launch_bounds__(kWeldThreads) void normals_sums_kernel(const NormalsArgs a) {
    const uint32_t stride = gridDim.x * kWeldThreads;
    double scale = 0.0;
    if (AREA) {
        const uint32_t m_bits = *a.max_bits;
        if (m_bits == 0u) return;                                               // M = 0: all zeros
        scale = weld_pow2(28 - weld_exponent(m_bits));                          // 2^(28 - e), e = floor(log2 M)
    }
    for (uint32_t t = blockIdx.x * kWeldThreads + threadIdx.x; t < a.n_tris; t += stride) {
        WeldTri tri;
        f3 n;
        float l;
        if (!weld_triangle(a.vertices, a.faces, a.n_vertices, t, tri) || !weld_normal(tri, n, l)) continue;
        if (AREA) {
            const long long qx = weld_fixed(n.x, scale), qy = weld_fixed(n.y, scale), qz = weld_fixed(n.z, scale);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                long long *acc = a.acc + 3 * (size_t)tri.i[k];
                weld_add(acc + 0, qx); weld_add(acc + 1, qy); weld_add(acc + 2, qz);
            }
        } else {
            const f3 u = mk3(n.x / l, n.y / l, n.z / l);                        // three divisions
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const f3 ea = tri.v[(k + 1) % 3] - tri.v[k], eb = tri.v[(k + 2) % 3] - tri.v[k];
                const float angle = wn_atan2(l, dot(ea, eb));                   // l > 0: the precondition y != 0 holds
                if (!weld_finite(angle)) continue;                              // dot(a, b) was a NaN: the corner adds nothing
                long long *acc = a.acc + 3 * (size_t)tri.i[k];
                weld_add(acc + 0, weld_fixed(angle * u.x, 0x1p28));
                weld_add(acc + 1, weld_fixed(angle * u.y, 0x1p28));
                weld_add(acc + 2, weld_fixed(angle * u.z, 0x1p28));
            }
        }
    }
}

__global__ __launch_bounds__(kWeldThreads) void normals_finish_kernel(const NormalsArgs a) {
    const uint32_t stride = gridDim.x * kWeldThreads;
    for (uint32_t v = blockIdx.x * kWeldThreads + threadIdx.x; v < a.n_vertices; v += stride) {
        const double x = (double)a.acc[3 * (size_t)v], y = (double)a.acc[3 * (size_t)v + 1], z = (double)a.acc[3 * (size_t)v + 2];
        const double len = sqrt(x * x + y * y + z * z);
        float *o = a.out + 3 * (size_t)v;
        o[0] = len > 0.0 ? (float)(x / len) : 0.0f;
        o[1] = len > 0.0 ? (float)(y / len) : 0.0f;
        o[2] = len > 0.0 ? (float)(z / len) : 0.0f;
    }
}

// the largest finite |coordinate| of a position as bits, 0 if none is finite
WELD_DEV uint32_t smooth_bits(f3 p) {
    uint32_t best = 0;
    if (weld_finite(p.x)) best = max(best, __float_as_uint(__builtin_fabsf(p.x)));
    if (weld_finite(p.y)) best = max(best, __float_as_uint(__builtin_fabsf(p.y)));
    if (weld_finite(p.z)) best = max(best, __float_as_uint(__builtin_fabsf(p.z)));
    return best;
}

// drt.h "smoothing": k = 27 - e, e = floor(log2 M); M = 0: k = 0 (every finite coordinate is then a zero)
WELD_DEV int smooth_shift(uint32_t m_bits) { return m_bits ? 27 - weld_exponent(m_bits) : 0; }

__global__ __launch_bounds__(kWeldThreads) void smooth_maximum_kernel(const SmoothArgs a) {
    const uint32_t stride = gridDim.x * kWeldThreads;
    uint32_t best = 0;
    for (uint32_t v = blockIdx.x * kWeldThreads + threadIdx.x; v < a.n_vertices; v += stride) best = max(best, smooth_bits(ld3(a.src + 3 * (size_t)v)));
    weld_fold_maximum(best, a.max_bits);
}

__global__ __launch_bounds__(kWeldThreads) void smooth_sums_kernel(const SmoothArgs a) {
    const uint32_t stride = gridDim.x * kWeldThreads;
    const double scale = weld_pow2(smooth_shift(a.max_bits[a.step & 1u]));
    if (blockIdx.x == 0 && threadIdx.x == 0) a.max_bits[(a.step + 1u) & 1u] = 0u;      // the update of this step folds into it
    for (uint32_t t = blockIdx.x * kWeldThreads + threadIdx.x; t < a.n_tris; t += stride) {
        WeldTri tri;
        if (!weld_triangle(a.src, a.faces, a.n_vertices, t, tri)) continue;
        long long q[3][3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            q[k][0] = weld_fixed(tri.v[k].x, scale); q[k][1] = weld_fixed(tri.v[k].y, scale); q[k][2] = weld_fixed(tri.v[k].z, scale);
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {                                           // acc[a] += q(p_b) + q(p_c), cyclically; cnt += 2
            long long *acc = a.acc + 3 * (size_t)tri.i[k];
#pragma unroll
            for (int j = 0; j < 3; j++) weld_add(acc + j, q[(k + 1) % 3][j] + q[(k + 2) % 3][j]);
            atomicAdd(&a.cnt[tri.i[k]], 2u);
        }
    }
}

__global__ __launch_bounds__(kWeldThreads) void smooth_update_kernel(const SmoothArgs a) {
    const uint32_t stride = gridDim.x * kWeldThreads;
    const double scale = weld_pow2(smooth_shift(a.max_bits[a.step & 1u]));
    const double f = (double)a.factor;
    uint32_t best = 0;
    for (uint32_t v = blockIdx.x * kWeldThreads + threadIdx.x; v < a.n_vertices; v += stride) {
        f3 p = ld3(a.src + 3 * (size_t)v);
        const uint32_t cnt = a.cnt[v];
        if (cnt != 0u && !(a.fixed && a.fixed[v]) && weld_finite3(p)) {
            const double den = (double)cnt * scale;
            // m = (double)acc / ((double)cnt * 2^k);  p' = (float)((double)p + (double)f * (m - (double)p))
            const double mx = (double)a.acc[3 * (size_t)v] / den, my = (double)a.acc[3 * (size_t)v + 1] / den, mz = (double)a.acc[3 * (size_t)v + 2] / den;
            p = mk3((float)((double)p.x + f * (mx - (double)p.x)), (float)((double)p.y + f * (my - (double)p.y)), (float)((double)p.z + f * (mz - (double)p.z)));
        }
        float *o = a.dst + 3 * (size_t)v;
        o[0] = p.x; o[1] = p.y; o[2] = p.z;
        best = max(best, smooth_bits(p));
    }
    weld_fold_maximum(best, &a.max_bits[(a.step + 1u) & 1u]);
}

// enough workgroups for every item, at most 8 per CU
uint32_t grid_for(uint32_t n, int num_cus) {
    const uint32_t want = (n + kWeldThreads - 1) / kWeldThreads;
    return std::max<uint32_t>(1, std::min<uint32_t>(want, (uint32_t)std::max(1, num_cus) * 8u));
}

}  // namespace

hipError_t launch_weld(const WeldArgs &args, hipStream_t stream) {
    if (args.corners == 0) return hipMemsetAsync(args.vertex_count, 0, sizeof(uint32_t), stream);
    static_assert(kWeldScanBlock == (uint32_t)kWeldThreads, "one corner per thread");
    const uint32_t n_blocks = weld_blocks(args.corners);
    hipError_t e = hipMemsetAsync(args.table, 0xFF, ((size_t)args.mask + 1) * sizeof(uint32_t), stream);     // kWeldEmpty
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(weld_insert_kernel, dim3(n_blocks), dim3(kWeldThreads), 0, stream, args);
    hipLaunchKernelGGL(weld_resolve_kernel, dim3(n_blocks), dim3(kWeldThreads), 0, stream, args);
    hipLaunchKernelGGL(weld_offsets_kernel, dim3(1), dim3(kWeldThreads), 0, stream, args.block_totals, n_blocks, args.vertex_count);
    hipLaunchKernelGGL(weld_number_kernel, dim3(n_blocks), dim3(kWeldThreads), 0, stream, args);
    hipLaunchKernelGGL(weld_gather_kernel, dim3(n_blocks), dim3(kWeldThreads), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_vertex_normals(NormalWeight weight, const NormalsArgs &args, int num_cus, hipStream_t stream) {
    if (args.n_vertices == 0) return hipSuccess;
    if (args.n_tris) {
        const dim3 grid(grid_for(args.n_tris, num_cus));
        if (weight == NormalWeight::area) {
            hipLaunchKernelGGL(normals_maximum_kernel, grid, dim3(kWeldThreads), 0, stream, args);
            hipLaunchKernelGGL(normals_sums_kernel<true>, grid, dim3(kWeldThreads), 0, stream, args);
        } else {
            hipLaunchKernelGGL(normals_sums_kernel<false>, grid, dim3(kWeldThreads), 0, stream, args);
        }
    }
    hipLaunchKernelGGL(normals_finish_kernel, dim3(grid_for(args.n_vertices, num_cus)), dim3(kWeldThreads), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_smooth_maximum(const SmoothArgs &args, int num_cus, hipStream_t stream) {
    if (args.n_vertices == 0) return hipSuccess;
    hipLaunchKernelGGL(smooth_maximum_kernel, dim3(grid_for(args.n_vertices, num_cus)), dim3(kWeldThreads), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_smooth_step(const SmoothArgs &args, int num_cus, hipStream_t stream) {
    if (args.n_vertices == 0) return hipSuccess;
    hipLaunchKernelGGL(smooth_sums_kernel, dim3(grid_for(std::max(args.n_tris, 1u), num_cus)), dim3(kWeldThreads), 0, stream, args);
    hipLaunchKernelGGL(smooth_update_kernel, dim3(grid_for(args.n_vertices, num_cus)), dim3(kWeldThreads), 0, stream, args);
    return hipGetLastError();
}

}  // namespace drt
