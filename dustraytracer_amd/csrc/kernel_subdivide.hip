// kernel_subdivide.hip -- one level of midpoint (1 -> 4) or Loop subdivision of an indexed mesh for gfx950 (drt_renderer_subdivide).
// The reference has no such call; include/drt.h states the rule, and every line below that computes a value cites the part of it that
// it implements.  None of the kernels reads a scene or a tree.  The connectivity -- adj, edge, half_edge and E -- is
// kernel_adjacency.hip's, made by the launches in front of these; the odd vertex of edge e is vertex V + e, so nothing is sorted,
// scanned or compacted here.
//
//   children  one lane per triangle: m(h) = V + edge[h], or faces[h] for a zero-length edge, and the four children, twelve words.
//             Reads no position, so an index out of range is copied as it is.  One lane stores V + E.
//   edges     one lane per undirected edge e < E (E is read from the device: the launch is sized for 3 N): the ends of the
//             representative half-edge are the parents of vertex V + e; its position is the midpoint, Loop's 3/8 3/8 1/8 1/8 on an
//             interior edge, or the NaN words where an end is out of range or not finite.  With Loop a usable edge adds q(p) of
//             each end to the other end's sums -- the interior or the crease set -- and 1 to the matching count: six 64-bit and two
//             32-bit integer atomic adds.  Integer sums are the same bytes in any order, float atomics are not.  An edge counts
//             once however many triangles share it, because the pass is over the edges.
//   finish    one lane per even vertex: the copy (midpoint), or Warren's weights on the interior sums / the 1/8 6/8 1/8 crease rule
//             in float64, rounded once.
// All three are grid-stride loops of 256-thread workgroups; a lane waits for no other lane.  Everything that decides a bit is an
// integer or one correctly rounded float64 operation (-ffp-contract=off), so the result is the same bytes whatever the launch shape.
//
// Registers: the compiler's resource remarks are recorded in DESIGN.md 5.36 (no scratch).  The kernels are streams with gathers: the
// limiter is memory latency on the indexed reads and, with Loop, the rate of the integer atomics.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "subdivide.hpp"

namespace drt {

namespace {

#define SUB_DEV __device__ __forceinline__

SUB_DEV bool sub_finite(float f) { return __builtin_fabsf(f) <= 3.402823466e+38f; }
SUB_DEV void sub_add(long long *p, long long v) { atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v); }

// the position of vertex `index`; ok is false if the index is outside [0, V) (a bounds check: nothing is read) or a coordinate is not finite
struct SubVertex { float x, y, z; bool ok; };
SUB_DEV SubVertex sub_vertex(const SubdivideArgs &a, int32_t index) {
    SubVertex p;
    p.x = p.y = p.z = 0.0f;
    p.ok = (uint32_t)index < a.n_vertices;                                      // (a negative index is a large unsigned one)
    if (p.ok) {
        const float *v = a.vertices + 3 * (size_t)(uint32_t)index;
        p.x = v[0]; p.y = v[1]; p.z = v[2];
        p.ok = sub_finite(p.x) && sub_finite(p.y) && sub_finite(p.z);
    }
    return p;
}

// drt.h "Loop": k = 27 - e, e = floor(log2 M); M = 0: k = 0 -- the smoothing's quantisation
SUB_DEV int sub_shift(uint32_t m_bits) { return m_bits ? 27 - weld_exponent(m_bits) : 0; }

// drt.h "midpoint": (float)(((double)pa + (double)pb) * 0.5)
SUB_DEV float sub_mid(float pa, float pb) { return (float)(((double)pa + (double)pb) * 0.5); }
// drt.h "interior odd vertex": (float)(((double)pa + (double)pb) * 0.375 + ((double)pc + (double)pd) * 0.125)
SUB_DEV float sub_odd(float pa, float pb, float pc, float pd) {
    return (float)(((double)pa + (double)pb) * 0.375 + ((double)pc + (double)pd) * 0.125);
}

__global__ __launch_bounds__(kWeldThreads) void subdivide_children_kernel(const SubdivideArgs a) {
    const uint32_t stride = gridDim.x * kWeldThreads;
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.vertex_count = a.n_vertices + (a.n_tris ? *a.edge_count : 0u);      // V + E, stored or not
    for (uint32_t t = blockIdx.x * kWeldThreads + threadIdx.x; t < a.n_tris; t += stride) {
        int32_t corner[3], mid[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            corner[k] = a.faces[3 * (size_t)t + k];
            const int32_t e = a.edge[3 * (size_t)t + k];
            mid[k] = e >= 0 ? (int32_t)(a.n_vertices + (uint32_t)e) : corner[k];      // a zero-length edge has no new vertex (V + E < 2^31)
        }
        int32_t *o = a.out_faces + 12 * (size_t)t;
        o[0] = corner[0]; o[1] = mid[0]; o[2] = mid[2];                         // child 4 t + 0 = (a, m0, m2)
        o[3] = corner[1]; o[4] = mid[1]; o[5] = mid[0];                         // child 4 t + 1 = (b, m1, m0)
        o[6] = corner[2]; o[7] = mid[2]; o[8] = mid[1];                         // child 4 t + 2 = (c, m2, m1)
        o[9] = mid[0]; o[10] = mid[1]; o[11] = mid[2];                          // child 4 t + 3 = (m0, m1, m2)
    }
}

template <bool LOOP>
__global__ __launch_bounds__(kWeldThreads) void subdivide_edges_kernel(const SubdivideArgs a) {
    const uint32_t stride = gridDim.x * kWeldThreads;
    const uint32_t n_edges = min(*a.edge_count, 3u * a.n_tris);                 // E <= 3 N: half_edge holds 3 N words
    double scale = 0.0;
    if (LOOP) scale = weld_pow2(sub_shift(*a.max_bits));
    for (uint32_t e = blockIdx.x * kWeldThreads + threadIdx.x; e < n_edges; e += stride) {
        const uint32_t h = (uint32_t)a.half_edge[e];                            // the representative: the edge's smallest half-edge
        const uint32_t t = h / 3u, k = h - 3u * t;
        const int32_t ia = a.faces[h], ib = a.faces[3 * (size_t)t + (k == 2u ? 0u : k + 1u)];
        const SubVertex pa = sub_vertex(a, ia), pb = sub_vertex(a, ib);
        const bool usable = pa.ok && pb.ok;
        const uint32_t id = a.n_vertices + e;                                   // the odd vertex of edge e
        uint32_t w[3] = {kSubdivideNaN, kSubdivideNaN, kSubdivideNaN};          // an unusable edge
        bool interior = false;
        if (LOOP) interior = a.adj[h] >= 0;                                     // every other edge (-1, -2) is a crease
        if (usable) {
            float x = sub_mid(pa.x, pb.x), y = sub_mid(pa.y, pb.y), z = sub_mid(pa.z, pb.z);
            if (LOOP && interior) {
                const uint32_t h2 = (uint32_t)a.adj[h], t2 = h2 / 3u, k2 = h2 - 3u * t2;
                const SubVertex pc = sub_vertex(a, a.faces[3 * (size_t)t + (k == 0u ? 2u : k - 1u)]);       // opposite h: corner (k + 2) % 3
                const SubVertex pd = sub_vertex(a, a.faces[3 * (size_t)t2 + (k2 == 0u ? 2u : k2 - 1u)]);    // opposite adj[h]
                if (pc.ok && pd.ok) {                                           // else the midpoint
                    x = sub_odd(pa.x, pb.x, pc.x, pd.x); y = sub_odd(pa.y, pb.y, pc.y, pd.y); z = sub_odd(pa.z, pb.z, pc.z, pd.z);
                }
            }
            w[0] = __float_as_uint(x); w[1] = __float_as_uint(y); w[2] = __float_as_uint(z);
            if (LOOP) {                                                         // acc[a] += q(pb), acc[b] += q(pa), one count each
                long long *acc = interior ? a.acc_int : a.acc_cr;
                uint32_t *cnt = interior ? a.n_int : a.n_cr;
                long long *sa = acc + 3 * (size_t)(uint32_t)ia, *sb = acc + 3 * (size_t)(uint32_t)ib;
                sub_add(sa + 0, weld_fixed(pb.x, scale)); sub_add(sa + 1, weld_fixed(pb.y, scale)); sub_add(sa + 2, weld_fixed(pb.z, scale));
                sub_add(sb + 0, weld_fixed(pa.x, scale)); sub_add(sb + 1, weld_fixed(pa.y, scale)); sub_add(sb + 2, weld_fixed(pa.z, scale));
                atomicAdd(&cnt[(uint32_t)ia], 1u);
                atomicAdd(&cnt[(uint32_t)ib], 1u);
            }
        }
        if (id < a.capacity) {                                                  // a smaller capacity stores the first `capacity` vertices
            uint32_t *o = reinterpret_cast<uint32_t *>(a.out_vertices) + 3 * (size_t)id;
            o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
            if (a.parents) { a.parents[2 * (size_t)id] = ia; a.parents[2 * (size_t)id + 1] = ib; }     // the ends of half_edge[e], in that order
        }
    }
}

// drt.h "finish": p' of one coordinate from its sum; S = (double)acc * 2^-k
SUB_DEV float sub_even_interior(float p, long long acc, double inverse, uint32_t n, double beta) {
    const double s = (double)acc * inverse;
    return (float)((double)p + beta * (s - (double)n * (double)p));
}
SUB_DEV float sub_even_crease(float p, long long acc, double inverse) {
    const double s = (double)acc * inverse;
    return (float)((double)p + 0.125 * (s - 2.0 * (double)p));
}

template <bool LOOP>
__global__ __launch_bounds__(kWeldThreads) void subdivide_finish_kernel(const SubdivideArgs a) {
    const uint32_t stride = gridDim.x * kWeldThreads;
    const uint32_t n_stored = min(a.n_vertices, a.capacity);
    double inverse = 0.0;
    if (LOOP) inverse = weld_pow2(-sub_shift(*a.max_bits));
    for (uint32_t v = blockIdx.x * kWeldThreads + threadIdx.x; v < n_stored; v += stride) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(a.vertices) + 3 * (size_t)v;
        uint32_t w[3] = {src[0], src[1], src[2]};                               // "keeps its bits"
        if (LOOP) {
            const uint32_t n_int = a.n_int[v], n_cr = a.n_cr[v];
            const float x = __uint_as_float(w[0]), y = __uint_as_float(w[1]), z = __uint_as_float(w[2]);
            // (a vertex with a coordinate that is not finite has no usable edge: both counts are 0)
            if (sub_finite(x) && sub_finite(y) && sub_finite(z)) {
                if (n_cr == 0u && n_int != 0u) {                                // Warren's weights
                    const double beta = n_int == 3u ? 0.1875 : 0.375 / (double)n_int;
                    const long long *acc = a.acc_int + 3 * (size_t)v;
                    w[0] = __float_as_uint(sub_even_interior(x, acc[0], inverse, n_int, beta));
                    w[1] = __float_as_uint(sub_even_interior(y, acc[1], inverse, n_int, beta));
                    w[2] = __float_as_uint(sub_even_interior(z, acc[2], inverse, n_int, beta));
                } else if (n_cr == 2u) {                                        // the crease rule: interior edges are ignored
                    const long long *acc = a.acc_cr + 3 * (size_t)v;
                    w[0] = __float_as_uint(sub_even_crease(x, acc[0], inverse));
                    w[1] = __float_as_uint(sub_even_crease(y, acc[1], inverse));
                    w[2] = __float_as_uint(sub_even_crease(z, acc[2], inverse));
                }                                                               // any other n_cr: a dart, a corner, a non-manifold vertex
            }
        }
        uint32_t *o = reinterpret_cast<uint32_t *>(a.out_vertices) + 3 * (size_t)v;
        o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
        if (a.parents) { a.parents[2 * (size_t)v] = (int32_t)v; a.parents[2 * (size_t)v + 1] = (int32_t)v; }
    }
}

// enough workgroups for every item, at most 8 per CU
uint32_t grid_for(uint32_t n, int num_cus) {
    const uint32_t want = (n + kWeldThreads - 1) / kWeldThreads;
    return std::max<uint32_t>(1, std::min<uint32_t>(want, (uint32_t)std::max(1, num_cus) * 8u));
}

}  // namespace

hipError_t launch_subdivide(SubdivideScheme scheme, const SubdivideArgs &args, int num_cus, hipStream_t stream) {
    const bool loop = scheme == SubdivideScheme::loop;
    hipLaunchKernelGGL(subdivide_children_kernel, dim3(grid_for(args.n_tris, num_cus)), dim3(kWeldThreads), 0, stream, args);
    if (args.capacity) {
        if (args.n_tris) {
            const dim3 grid(grid_for(3u * args.n_tris, num_cus));
            if (loop) hipLaunchKernelGGL(subdivide_edges_kernel<true>, grid, dim3(kWeldThreads), 0, stream, args);
            else hipLaunchKernelGGL(subdivide_edges_kernel<false>, grid, dim3(kWeldThreads), 0, stream, args);
        }
        if (args.n_vertices) {
            const dim3 grid(grid_for(std::min(args.n_vertices, args.capacity), num_cus));
            if (loop && args.n_tris) hipLaunchKernelGGL(subdivide_finish_kernel<true>, grid, dim3(kWeldThreads), 0, stream, args);
            else hipLaunchKernelGGL(subdivide_finish_kernel<false>, grid, dim3(kWeldThreads), 0, stream, args);
        }
    }
    return hipGetLastError();
}

}  // namespace drt
