// kernel_adjacency.hip -- the edge adjacency of a triangle list for gfx950 (drt_renderer_tri_adjacency, drt_renderer_face_adjacency,
// the uploaded scene's table) and boundary vertices (drt_renderer_boundary_vertices).  The rule is edge_adjacency.hpp's, which
// include/drt.h states; the table is the host routine's bytes.  None of the kernels reads a scene or a tree.
//
// Half-edge h = 3 t + e runs from end e to end (e + 1) % 3 of triangle t.  An end is K words compared as integers: the three words of
// a position (K = 3) or one vertex index (K = 1).  A half-edge's key is the unordered pair of its ends.
//
//   insert    one lane per half-edge whose ends differ: kernel_weld.hip's insert-only open-addressing table, here of half-edge
//             indices, hashed over the unordered pair, linear probing.  A free slot is claimed with atomicCAS(slot, empty, h); a slot
//             that holds a half-edge of the same pair takes atomicMin(slot, h); a slot of another pair is passed.  Once claimed a
//             slot's PAIR never changes, so a group ends in one slot whatever the order, and that slot ends holding its smallest
//             member.  The table is at most half full, so a probe always ends; a lane waits for no other lane's progress.
//   resolve   rep[h] = table[slot of h], the smallest half-edge of h's group (kAdjNone for a zero-length one).  Every h != rep[h]
//             does old = atomicMin(other[rep], h) and, if there was a value already, atomicMin(other[rep], kAdjMany): other[rep] ends
//             as kAdjNone (a group of one), the second member (a group of two) or kAdjMany = 0 (three or more; no second member is
//             half-edge 0, which is the smallest of whatever group it is in).  Integer minima: the same word in any order.
//             With edges: the flag rep[h] == h marks the undirected edges, and workgroup b stores how many of its half-edges are one.
//   offsets   (edges) ONE workgroup turns the block totals into exclusive offsets and stores E
//   number    (edges) representative h is edge id = offset + flags in front of it, ascending h: edge[h], half_edge[id] while id < capacity
//   classify  adj[h]: -2 for zero length; -1 if other[rep] is kAdjNone; -2 if it is kAdjMany; otherwise the one other member if it
//             runs the other way -- the start of one is the end of the other, read from the keys -- and -2 if not.
//             With edges: edge[h] = edge[rep[h]], -1 for zero length.
// The flag scan is kernel_weld.hip's shape (kernel_surface.hip's): no look-back, no flag, no spin.  Everything is integers, so the
// result is the same bytes whatever the launch shape; the hash decides nothing that can be observed.
//
//   boundary  one lane per triangle: plain stores of 1 into a zeroed byte array, so no order is involved
//
// Registers: the compiler's resource remarks are recorded in DESIGN.md 5.35 (no scratch).  The kernels are latency-bound gathers.
#include <hip/hip_runtime.h>

#include "adjacency.hpp"
#include "device_math.hpp"

namespace drt {

namespace {

#define ADJ_DEV __device__ __forceinline__

template <int K>
struct AdjKey { uint32_t a[K], b[K]; };                 // the start and the end of a half-edge

// half-edge h = 3 t + e: end e and end (e + 1) % 3 of triangle t
template <int K>
ADJ_DEV AdjKey<K> adj_key(const AdjacencyArgs &a, uint32_t h) {
    const uint32_t t = h / 3u, e = h - 3u * t, e1 = e == 2u ? 0u : e + 1u;
    const unsigned char *tri = a.first + (size_t)t * a.tri_stride;
    const uint32_t *p = reinterpret_cast<const uint32_t *>(tri + e * a.vertex_stride);
    const uint32_t *q = reinterpret_cast<const uint32_t *>(tri + e1 * a.vertex_stride);
    AdjKey<K> key;
#pragma unroll
    for (int k = 0; k < K; k++) { key.a[k] = p[k]; key.b[k] = q[k]; }
    return key;
}

template <int K>
ADJ_DEV bool adj_words_equal(const uint32_t (&p)[K], const uint32_t (&q)[K]) {
    bool same = true;
#pragma unroll
    for (int k = 0; k < K; k++) same = same && p[k] == q[k];
    return same;
}

// both ends the same: drt.h "zero length"
template <int K>
ADJ_DEV bool adj_degenerate(const AdjKey<K> &x) { return adj_words_equal<K>(x.a, x.b); }
// x and y run between the same two ends, and the other way round (for ends that differ, exactly one of the two holds in a group)
template <int K>
ADJ_DEV bool adj_same_way(const AdjKey<K> &x, const AdjKey<K> &y) { return adj_words_equal<K>(x.a, y.a) && adj_words_equal<K>(x.b, y.b); }
template <int K>
ADJ_DEV bool adj_opposite(const AdjKey<K> &x, const AdjKey<K> &y) { return adj_words_equal<K>(x.a, y.b) && adj_words_equal<K>(x.b, y.a); }

template <int K>
ADJ_DEV uint32_t adj_end_hash(const uint32_t (&p)[K]) {
    uint32_t v = 0;
#pragma unroll
    for (int k = K - 1; k >= 0; k--) v = pcg_hash(p[k] ^ v);
    return v;
}
// the same for both directions: the two ends' hashes, the smaller first
template <int K>
ADJ_DEV uint32_t adj_hash(const AdjKey<K> &x) {
    const uint32_t ha = adj_end_hash<K>(x.a), hb = adj_end_hash<K>(x.b);
    return pcg_hash(min(ha, hb) ^ pcg_hash(max(ha, hb)));
}

template <int K>
__global__ __launch_bounds__(kWeldThreads) void adjacency_insert_kernel(const AdjacencyArgs a) {
    const uint32_t h = blockIdx.x * kWeldThreads + threadIdx.x;
    if (h >= a.half_edges) return;
    const AdjKey<K> key = adj_key<K>(a, h);
    if (adj_degenerate<K>(key)) return;                                         // (the resolve finds it again: rep[h] is not read)
    uint32_t slot = adj_hash<K>(key) & a.mask;
    // at most mask + 1 probes: the table holds at most half_edges <= (mask + 1) / 2 pairs, so a free or an equal slot comes first
    for (uint32_t tries = 0; tries <= a.mask; tries++) {
        const uint32_t held = atomicCAS(&a.table[slot], kWeldEmpty, h);
        if (held == kWeldEmpty) break;                                          // claimed
        const AdjKey<K> there = adj_key<K>(a, held);                            // (held < half_edges: a half-edge index)
        if (adj_same_way<K>(there, key) || adj_opposite<K>(there, key)) { atomicMin(&a.table[slot], h); break; }
        slot = (slot + 1u) & a.mask;
    }
    a.rep[h] = slot;
}

// inclusive sum of v over the workgroup's kWeldScanBlock threads: a wave scan, then the four wave totals through LDS
ADJ_DEV uint32_t adj_block_inclusive(uint32_t v, uint32_t *s_wave) {
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

template <int K>
__global__ __launch_bounds__(kWeldThreads) void adjacency_resolve_kernel(const AdjacencyArgs a) {
    __shared__ uint32_t s_wave[kWeldThreads / 64];
    const uint32_t h = blockIdx.x * kWeldScanBlock + threadIdx.x;
    uint32_t flag = 0;
    if (h < a.half_edges) {
        uint32_t rep = kAdjNone;
        if (!adj_degenerate<K>(adj_key<K>(a, h))) {
            rep = a.table[a.rep[h]];                                            // the smallest half-edge of h's group
            if (rep != h) {
                const uint32_t old = atomicMin(&a.other[rep], h);
                if (old != kAdjNone) atomicMin(&a.other[rep], kAdjMany);        // a second one beside the representative: three or more
            }
            flag = rep == h ? 1u : 0u;
        }
        a.rep[h] = rep;
    }
    if (a.edge == nullptr) return;                                              // (the same in every thread)
    const uint32_t incl = adj_block_inclusive(flag, s_wave);
    if (threadIdx.x == kWeldScanBlock - 1) a.block_totals[blockIdx.x] = incl;
}

__global__ __launch_bounds__(kWeldThreads) void adjacency_offsets_kernel(uint32_t *block_totals, uint32_t n_blocks, uint32_t *edge_count) {
    __shared__ uint32_t s_wave[kWeldThreads / 64];
    __shared__ uint32_t s_total;
    uint32_t carry = 0;                                                         // (the same in every thread)
    for (uint32_t base = 0; base < n_blocks; base += kWeldScanBlock) {
        const uint32_t b = base + threadIdx.x;
        const uint32_t v = b < n_blocks ? block_totals[b] : 0u;
        const uint32_t incl = adj_block_inclusive(v, s_wave);
        if (b < n_blocks) block_totals[b] = carry + (incl - v);                 // exclusive: the edges in front of block b
        if (threadIdx.x == kWeldScanBlock - 1) s_total = incl;
        __syncthreads();
        carry += s_total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *edge_count = carry;                                  // E, stored or not
}

__global__ __launch_bounds__(kWeldThreads) void adjacency_number_kernel(const AdjacencyArgs a) {
    __shared__ uint32_t s_wave[kWeldThreads / 64];
    const uint32_t h = blockIdx.x * kWeldScanBlock + threadIdx.x;
    const bool is_rep = h < a.half_edges && a.rep[h] == h;
    const uint32_t incl = adj_block_inclusive(is_rep ? 1u : 0u, s_wave);
    if (!is_rep) return;
    const uint32_t id = a.block_totals[blockIdx.x] + incl - 1u;                 // edges are numbered in ascending representative
    a.edge[h] = (int32_t)id;
    if (id < a.capacity) a.half_edge[id] = (int32_t)h;                          // a smaller capacity stores the first `capacity` edges
}

template <int K>
__global__ __launch_bounds__(kWeldThreads) void adjacency_classify_kernel(const AdjacencyArgs a) {
    const uint32_t h = blockIdx.x * kWeldThreads + threadIdx.x;
    if (h >= a.half_edges) return;
    const uint32_t rep = a.rep[h];
    int32_t adj = -2;                                                           // zero length, three or more, two the same way
    if (rep != kAdjNone) {
        const uint32_t second = a.other[rep];
        if (second == kAdjNone) adj = -1;                                       // a group of one (h is its representative)
        else if (second != kAdjMany) {
            const uint32_t twin = h == rep ? second : rep;                      // (h != rep: h is the second one)
            if (adj_opposite<K>(adj_key<K>(a, h), adj_key<K>(a, twin))) adj = (int32_t)twin;
        }
    }
    a.adj[h] = adj;
    if (a.edge && rep != h) a.edge[h] = rep == kAdjNone ? -1 : a.edge[rep];     // (edge[rep] is the launch before's; no lane writes it here)
}

__global__ __launch_bounds__(kWeldThreads) void boundary_vertices_kernel(const BoundaryArgs a) {
    const uint32_t t = blockIdx.x * kWeldThreads + threadIdx.x;
    if (t >= a.n_tris) return;
    uint32_t i[3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        i[k] = (uint32_t)a.faces[3 * (size_t)t + k];                            // (a negative index is a large unsigned one)
        ok = ok && i[k] < a.n_vertices;
    }
    if (!ok) return;                                                            // the bounds check: the triangle is skipped
#pragma unroll
    for (int e = 0; e < 3; e++) {
        const int32_t v = a.adj[3 * (size_t)t + e];
        if (v == -1 || ((a.flags & 1u) && v == -2)) { a.out[i[e]] = 1; a.out[i[(e + 1) % 3]] = 1; }
    }
}

template <int K>
hipError_t launch_adjacency_of(const AdjacencyArgs &args, hipStream_t stream) {
    static_assert(kWeldScanBlock == (uint32_t)kWeldThreads, "one half-edge per thread");
    const uint32_t n_blocks = weld_blocks(args.half_edges);
    hipError_t e = hipMemsetAsync(args.table, 0xFF, ((size_t)args.mask + 1) * sizeof(uint32_t), stream);     // kWeldEmpty
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(args.other, 0xFF, (size_t)args.half_edges * sizeof(uint32_t), stream);                // kAdjNone
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(adjacency_insert_kernel<K>, dim3(n_blocks), dim3(kWeldThreads), 0, stream, args);
    hipLaunchKernelGGL(adjacency_resolve_kernel<K>, dim3(n_blocks), dim3(kWeldThreads), 0, stream, args);
    if (args.edge) {
        hipLaunchKernelGGL(adjacency_offsets_kernel, dim3(1), dim3(kWeldThreads), 0, stream, args.block_totals, n_blocks, args.edge_count);
        hipLaunchKernelGGL(adjacency_number_kernel, dim3(n_blocks), dim3(kWeldThreads), 0, stream, args);
    }
    hipLaunchKernelGGL(adjacency_classify_kernel<K>, dim3(n_blocks), dim3(kWeldThreads), 0, stream, args);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_adjacency(AdjacencyKey key, const AdjacencyArgs &args, hipStream_t stream) {
    if (args.half_edges == 0) return hipSuccess;                                // drt.h: no triangles, nothing is touched
    return key == AdjacencyKey::position ? launch_adjacency_of<3>(args, stream) : launch_adjacency_of<1>(args, stream);
}

hipError_t launch_boundary_vertices(const BoundaryArgs &args, hipStream_t stream) {
    if (args.n_tris == 0) return hipSuccess;
    hipLaunchKernelGGL(boundary_vertices_kernel, dim3((args.n_tris + kWeldThreads - 1) / kWeldThreads), dim3(kWeldThreads), 0, stream, args);
    return hipGetLastError();
}

}  // namespace drt
