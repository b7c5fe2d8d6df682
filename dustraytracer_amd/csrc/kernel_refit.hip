// kernel_refit.hip -- drt_renderer_refit: a renderer's device copy of the scene refitted in place to new vertex positions.
//
// What comes out is what HostScene::refit followed by pack() makes (scene_host.cpp), bit for bit:
//   leaf pass   one thread per leaf: every triangle of the leaf is assembled from positions[order[k]] with make_triangle's
//               fp32 operations (-ffp-contract=off, correctly rounded / and sqrtf: the Makefile's flags) into its TriHot record,
//               and the leaf's exact extent (min / max over its vertices) is kept in the extent array
//   heights     one thread per interior node, the nodes of one height (distance to the deepest leaf below) per launch: the
//               node's extent = min / max of its children's exact extents.  A kernel boundary orders the heights.
//   top         the few-thousand-node top of the tree in one workgroup, __syncthreads() between heights
// Every node stores its extent into its parent's InnerNode record as set_bounds does: bmin = lo, bmax = lo + (hi - lo).
// Min and max take -0 < +0 (min_zero_ordered / max_zero_ordered of scene_host.hpp), so the order of reduction does not matter.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "refit.hpp"

namespace drt {
namespace {

__device__ __forceinline__ float min_zo(float a, float b) { return a < b ? a : b < a ? b : signbit(a) ? a : b; }
__device__ __forceinline__ float max_zo(float a, float b) { return a > b ? a : b > a ? b : signbit(a) ? b : a; }

struct Ext { float lo[3], hi[3]; };

// the extent into the extent array and, as a box, into the parent's record (or the root box)
__device__ __forceinline__ void store_extent(const RefitArgs &a, int32_t node, uint32_t dest, const Ext &e) {
    float *x = a.ext + 6 * (size_t)node;
    for (int c = 0; c < 3; c++) { x[c] = e.lo[c]; x[3 + c] = e.hi[c]; }
    float *box = dest == kRefitRootDest ? a.root_box : reinterpret_cast<float *>(a.inner + (dest >> 1)) + 6 * (dest & 1u);
    for (int c = 0; c < 3; c++) { box[c] = e.lo[c]; box[3 + c] = e.lo[c] + (e.hi[c] - e.lo[c]); }
}

__global__ __launch_bounds__(kRefitThreads) void refit_leaf_kernel(RefitArgs a) {
    const uint32_t i = blockIdx.x * kRefitThreads + threadIdx.x;
    if (i >= a.n_leaves) return;
    const RefitLeaf leaf = a.leaves[i];
    Ext e;
    for (int c = 0; c < 3; c++) { e.lo[c] = FLT_MAX; e.hi[c] = -FLT_MAX; }
    bool finite = true;
    for (int32_t k = leaf.start; k < leaf.start + leaf.count; k++) {
        const size_t src = 9 * (size_t)a.order[k];
        float p[9];
        for (int j = 0; j < 9; j++) { p[j] = a.pos[src + j]; finite = finite && isfinite(p[j]); }
        float4 avg;
        if (a.nrm) {
            float q[9];
            for (int j = 0; j < 9; j++) { q[j] = a.nrm[src + j]; finite = finite && isfinite(q[j]); }
            avg.x = (q[0] + q[3] + q[6]) / 3.0f;             // (N0 + N1 + N2) / 3 (Scene.cu:279)
            avg.y = (q[1] + q[4] + q[7]) / 3.0f;
            avg.z = (q[2] + q[5] + q[8]) / 3.0f;
            avg.w = 0.f;
            a.avg_normal[k] = avg;
        } else {
            avg = a.avg_normal[k];
        }
        const float e1[3] = { p[3] - p[0], p[4] - p[1], p[5] - p[2] }, e2[3] = { p[6] - p[0], p[7] - p[1], p[8] - p[2] };
        float f[3] = { e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0] };
        const float ndot = f[0] * avg.x + f[1] * avg.y + f[2] * avg.z;
        if (ndot < 0.0f) for (int c = 0; c < 3; c++) f[c] = -f[c];
        const float inv_len = 1.0f / sqrtf(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);      // normalize, helper_math.cuh:1325-1328
        TriHot h;
        for (int c = 0; c < 3; c++) {
            h.v0[c] = p[c]; h.e1[c] = e1[c]; h.e2[c] = e2[c]; h.fn[c] = f[c] * inv_len;
            for (int v = 0; v < 3; v++) { e.lo[c] = min_zo(e.lo[c], p[3 * v + c]); e.hi[c] = max_zo(e.hi[c], p[3 * v + c]); }
        }
        a.hot[k] = h;
    }
    if (!finite) atomicOr(a.error, 1u);
    store_extent(a, leaf.node, leaf.dest, e);
}

__device__ __forceinline__ void refit_inner(const RefitArgs &a, const RefitInner &n) {
    const float *x = a.ext + 6 * (size_t)n.c1, *y = a.ext + 6 * (size_t)n.c2;
    Ext e;
    for (int c = 0; c < 3; c++) { e.lo[c] = min_zo(x[c], y[c]); e.hi[c] = max_zo(x[3 + c], y[3 + c]); }
    store_extent(a, n.node, n.dest, e);
}

__global__ __launch_bounds__(kRefitThreads) void refit_height_kernel(RefitArgs a, uint32_t first, uint32_t count) {
    const uint32_t i = blockIdx.x * kRefitThreads + threadIdx.x;
    if (i < count) refit_inner(a, a.levels[first + i]);
}

// heights h_first .. h_last (1-based) of the tree, one after the other, in one workgroup
__global__ __launch_bounds__(kRefitTopThreads) void refit_top_kernel(RefitArgs a, uint32_t h_first, uint32_t h_last) {
    for (uint32_t h = h_first; h <= h_last; h++) {
        const uint32_t first = a.height_begin[h - 1], end = a.height_begin[h];
        for (uint32_t i = first + threadIdx.x; i < end; i += kRefitTopThreads) refit_inner(a, a.levels[i]);
        __syncthreads();
    }
}

}  // namespace

hipError_t launch_refit(const RefitArgs &args, const std::vector<uint32_t> &height_begin, int top_nodes, hipStream_t stream,
                        int *launches) {
    int n = 0;
    if (args.n_leaves) {
        hipLaunchKernelGGL(refit_leaf_kernel, dim3((args.n_leaves + kRefitThreads - 1) / kRefitThreads), dim3(kRefitThreads), 0, stream, args);
        n++;
    }
    const uint32_t heights = height_begin.empty() ? 0u : (uint32_t)height_begin.size() - 1;
    // the lowest height from which every height up to the root has at most top_nodes nodes
    uint32_t top = heights + 1;
    if (top_nodes > 0)
        while (top > 1 && height_begin[top - 1] - height_begin[top - 2] <= (uint32_t)top_nodes) top--;
    for (uint32_t h = 1; h < top; h++) {
        const uint32_t first = height_begin[h - 1], count = height_begin[h] - first;
        hipLaunchKernelGGL(refit_height_kernel, dim3((count + kRefitThreads - 1) / kRefitThreads), dim3(kRefitThreads), 0, stream, args, first, count);
        n++;
    }
    if (top <= heights) {
        hipLaunchKernelGGL(refit_top_kernel, dim3(1), dim3(kRefitTopThreads), 0, stream, args, top, heights);
        n++;
    }
    if (launches) *launches = n;
    return hipGetLastError();
}

}  // namespace drt
