// winding.hpp -- launch seam of kernel_winding.hip (generalised winding numbers of points: include/drt.h
// drt_renderer_winding_numbers / drt_renderer_winding_inside / drt_renderer_winding_signed_distance), the node moment's layout, and
// the rule's arithmetic: the project's own atan2 and the solid angle of a triangle, digit for digit as drt.h states them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "device_scene.hpp"
#ifdef __HIP__
#include "device_math.hpp"
#endif
#include "ray_query.hpp"
#include "refit.hpp"

namespace drt {

// drt.h "node moment": 32 bytes per tree node.  The array holds the interior nodes at their InnerNode record index and leaf l at
// n_inner + l, so a node reference finds its moment without a table.
struct alignas(16) WindingMoment { float N[3]; float r2; float p[3]; float pad; };
static_assert(sizeof(WindingMoment) == 32, "WindingMoment layout");

constexpr int kWnThreads = 256;                // the moment passes
constexpr int kWnTopThreads = 1024;            // the single-workgroup launch over the top of the tree ...
constexpr int kWnTopNodes = 4096;              // ... takes the heights whose node counts stay at or below this (and all above)

enum class WindingOut : uint32_t {
    number = 0,                  // float[n]: w
    inside = 1,                  // uint8_t[n]: w >= threshold
    side = 2,                    // the 4-byte `side` word at byte 28 of drt_nearest[n]: -1 if w >= threshold, else +1
};

// The moment passes read the refit plan's leaves and interior nodes by height (refit.hpp), the device's TriHot records and boxes.
struct WindingMomentArgs {
    const RefitLeaf *leaves;
    uint32_t n_leaves;
    const RefitInner *levels;        // interior nodes grouped by height, 1 first
    WindingMoment *moments;          // n_inner + n_leaves records
    float4 *sums;                    // per node {S[3], A}: the weighted centroid sum and the area a parent adds up
};

// Enqueues the leaf pass, one launch per height that has more than kWnTopNodes nodes (or one under it that does), and one
// single-workgroup launch over the heights above.
hipError_t launch_winding_moments(const SceneView &scene, const WindingMomentArgs &args, const std::vector<uint32_t> &height_begin,
                                  hipStream_t stream);

// The grid, the claim heads and the HBM stack are the occlusion ray query's (ray_query.hpp), as crossings.hpp's are.
struct WindingArgs {
    const void *points;          // drt_point[n] (16 B, 16-B aligned); max_dist is not read
    void *out;                   // what `kind` says
    QueryFrame frame;            // n, tree depth, refill threshold, claim heads, HBM stack: 4 B stack entries
    float beta2;                 // beta * beta in fp32 (+inf: never approximate)
    float threshold;
    const WindingMoment *moments;
};

hipError_t launch_winding(const SceneView &scene, WindingOut kind, const WindingArgs &args, int num_cus, hipStream_t stream);

#ifdef __HIP__                                      // device code: the .hip translation units only
// drt.h "atan2": one division and a fixed polynomial, plain fp32 + * / in the order written.  y != 0 is the caller's.
//   ax = |x|, ay = |y|; swap = ay > ax; mx = swap ? ay : ax; mn = swap ? ax : ay
//   big = mn > 0.414213562f * mx; t = big ? (mn - mx) / (mn + mx) : mn / mx; s = t * t
//   r = (((8.05374449538e-2f * s - 1.38776856032e-1f) * s + 1.99777106478e-1f) * s - 3.33329491539e-1f) * s * t + t
//   big: r = 0.785398163f + r;  swap: r = 1.57079633f - r;  x < 0: r = 3.14159265f - r;  y < 0: r = -r
DRT_DEV float wn_atan2(float y, float x) {
    const float ax = __builtin_fabsf(x), ay = __builtin_fabsf(y);
    const bool swap = ay > ax;
    const float mx = swap ? ay : ax, mn = swap ? ax : ay;
    const bool big = mn > 0.414213562f * mx;
    const float num = big ? mn - mx : mn, den = big ? mn + mx : mx;
    const float t = num / den;
    const float s = t * t;
    float r = (((8.05374449538e-2f * s - 1.38776856032e-1f) * s + 1.99777106478e-1f) * s - 3.33329491539e-1f) * s * t + t;
    if (big) r = 0.785398163f + r;
    if (swap) r = 1.57079633f - r;
    if (x < 0.0f) r = 3.14159265f - r;
    if (y < 0.0f) r = -r;
    return r;
}

// drt.h "triangle term": the signed solid angle of (v0, e1, e2) seen from q, in steradians; exactly 0 when det == 0.
DRT_DEV float wn_solid_angle(f3 q, f3 v0, f3 e1, f3 e2) {
    const f3 a = v0 - q, b = a + e1, c = a + e2;
    const float det = dot(a, cross(e1, e2));
    if (det == 0.0f) return 0.0f;
    const float la = sqrtf(dot(a, a)), lb = sqrtf(dot(b, b)), lc = sqrtf(dot(c, c));
    const float den = la * lb * lc + dot(a, b) * lc + dot(b, c) * la + dot(c, a) * lb;
    return 2.0f * wn_atan2(det, den);
}
#endif

}  // namespace drt
