// refit.hpp -- launch seam of kernel_refit.hip: the in-place refit of a renderer's device copy of the scene
// (include/drt.h drt_renderer_refit).  The tree's topology, node order and triangle order stay; the triangles' TriHot
// records, the child boxes of every InnerNode and the root box are recomputed from new vertex positions.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "device_scene.hpp"

namespace drt {

constexpr uint32_t kRefitRootDest = 0xFFFFFFFFu;   // the node's box is the root box (SceneView::root_min / root_max)
constexpr int kRefitThreads = 256;
constexpr int kRefitTopThreads = 1024;             // the single-workgroup launch over the top of the tree
constexpr int kRefitTopNodes = 4096;               // heights whose node counts stay at or below this (and all above) go into it

// `node` and the children are slots of the exact-extent array (the host scene's node indices); dest = InnerNode record << 1 |
// child slot of the box this node's extent is stored into, or kRefitRootDest.
struct RefitLeaf { int32_t start, count, node; uint32_t dest; };
struct RefitInner { int32_t c1, c2, node; uint32_t dest; };

// Host image of the per-scene metadata (built once per upload, drt_capi.cpp refit_plan)
struct RefitPlan {
    std::vector<int32_t> order;                    // load index of triangle k
    std::vector<float4> avg_normal;                // (N0 + N1 + N2) / 3 of the stored normals, as make_triangle computes it
    std::vector<RefitLeaf> leaves;
    std::vector<RefitInner> inner;                 // interior nodes grouped by height (distance to the deepest leaf below), 1 first
    std::vector<uint32_t> height_begin;            // inner[height_begin[h - 1] .. height_begin[h]) have height h; size = heights + 1
    uint32_t n_nodes = 0;
};

struct RefitArgs {
    const float *pos;            // float[n][3][3], load order
    const float *nrm;            // same shape, or nullptr: use avg_normal as it stands
    const int32_t *order;
    float4 *avg_normal;          // rewritten when nrm is given
    TriHot *hot;
    InnerNode *inner;
    float *ext;                  // 6 floats per node: exact lo[3], hi[3]
    const RefitLeaf *leaves;
    uint32_t n_leaves;
    const RefitInner *levels;
    const uint32_t *height_begin;   // device copy of RefitPlan::height_begin
    float *root_box;             // 6 floats: bmin, bmax of the root
    unsigned int *error;         // bit 0: a non-finite input value
};

// Enqueues the leaf pass, one launch per height that has more than kRefitTopNodes nodes (or one under it that does), and one
// single-workgroup launch over the heights above (top_nodes = 0: one launch per height throughout).
hipError_t launch_refit(const RefitArgs &args, const std::vector<uint32_t> &height_begin, int top_nodes, hipStream_t stream,
                        int *launches);

}  // namespace drt
