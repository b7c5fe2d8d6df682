// kernel_curve.hip -- intersection curves (include/drt.h drt_renderer_chain_intersections): the segments of drt_renderer_intersect_triangles
// chained into open polylines and closed loops across scene triangles AND across queries, by two edge adjacency tables.  Integers only:
// no coordinate is read.
//
// One lane per record, two launches of its own in front of the phases it shares with the section contours (contour.hpp
// launch_chain_phases: init, the jumping rounds, tail, scan, scatter, here over the single range [0, total)):
//   keys      the query that owns the record (binary search in splits, then the clamped range is checked), a dense 4-byte array of
//             the records' prim, and whether the record is live, kept in the owner word: a record that is not live has no owner
//   link      drt.h "link": cq says which table the exit edge is looked up in.  A scene edge (cq < 4): adj[3 prim + cq], the twin's
//             triangle in the SAME query's range.  A query edge (cq >= 4): query_adj[3 owner + cq - 4], the SAME triangle in the twin
//             query's range.  Two dependent reads -- owner / code, then the table -- and a binary search over the 4-byte keys of
//             the target range (a miss record's prim -1 is the largest unsigned key, so a range is ascending); the 32-byte records are
//             touched once more, for the code of the one record found.  succ[j] = m and atomicMin(pred[m], j), as the contour link has
//             it: the shared init phase settles input on which the link is not injective.
//
// Bounds on any input: prim and both code digits are checked before they index a table (keys); a query_adj value is checked against n
// before it names a range; the search stays inside the clamped range of that query; the found record must be live and owned by it.
#include <hip/hip_runtime.h>

#include "contour.hpp"

namespace drt {

namespace {

#define CV_DEV static __device__ __forceinline__

// an endpoint's code: a scene edge 0..2 or 4 + a query edge
CV_DEV bool edge_code(uint32_t c) { return c < 7u && c != 3u; }

__global__ __launch_bounds__(kContourThreads) void curve_keys_kernel(const ContourArgs a) {
    const uint32_t j = blockIdx.x * kContourThreads + threadIdx.x;
    if (j >= a.total) return;
    const uint32_t prim = contour_seg_word(a.segs, j, 3), code = contour_seg_word(a.segs, j, 7);
    const bool live = prim < a.n_tris && edge_code(code & 15u) && edge_code(code >> 4);
    a.owner[j] = live ? contour_owner(a.splits, a.n, a.total, j) : kContourNone;
    a.key[j] = prim;
    a.pred[j] = kContourNone;
}

__global__ __launch_bounds__(kContourThreads) void curve_link_kernel(const ContourArgs a) {
    const uint32_t j = blockIdx.x * kContourThreads + threadIdx.x;
    uint32_t link = kContourFlag | 5u;                  // not live
    const uint32_t owner = j < a.total ? a.owner[j] : kContourNone;
    if (owner != kContourNone) {
        const uint32_t prim = a.key[j];
        const uint32_t cq = contour_seg_word(a.segs, j, 7) >> 4;
        const bool scene_edge = cq < 4u;
        const int32_t twin = scene_edge ? a.adj[3u * prim + cq] : a.query_adj[3u * owner + (cq - 4u)];
        if (twin == -1) link = kContourFlag | 1u;
        else if (twin < 0 || (!scene_edge && (uint32_t)twin / 3u >= a.n)) link = kContourFlag | 2u;
        else {
            const uint32_t across = (uint32_t)twin / 3u, edge = (uint32_t)twin - 3u * across;
            const uint32_t query = scene_edge ? owner : across;
            const uint32_t target = scene_edge ? across : prim;
            const uint32_t entry = scene_edge ? edge : 4u + edge;
            const ContourRange r = contour_range(a.splits, query, a.total);
            uint32_t lo = r.lo, hi = r.hi;
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (a.key[mid] < target) lo = mid + 1;
                else hi = mid;
            }
            link = kContourFlag | 3u;
            if (lo < r.hi && a.key[lo] == target && a.owner[lo] == query) {
                if ((contour_seg_word(a.segs, lo, 7) & 15u) == entry) {
                    link = lo;
                    atomicMin(&a.pred[lo], j);
                } else link = kContourFlag | 4u;
            }
        }
    }
    if (j < a.total) a.succ[j] = link;
    // counts[2]: the records that are not live, one atomic per workgroup that has any
    if (a.chains) {
        const int dead = __syncthreads_count(j < a.total && owner == kContourNone);
        if (dead && threadIdx.x == 0) atomicAdd(&a.chains[2], (uint32_t)dead);
    }
}

}  // namespace

hipError_t launch_curves(const ContourArgs &a, hipStream_t stream) {
    const dim3 block(kContourThreads);
    const dim3 lanes((a.total + kContourThreads - 1) / kContourThreads);
    hipError_t e = hipMemsetAsync(a.moved, 0, (kContourMaxRounds + 1) * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    if (a.chains) {
        e = hipMemsetAsync(a.chains, 0, 3 * sizeof(uint32_t), stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(curve_keys_kernel, lanes, block, 0, stream, a);
    hipLaunchKernelGGL(curve_link_kernel, lanes, block, 0, stream, a);
    return launch_chain_phases(a, true, stream);
}

}  // namespace drt
