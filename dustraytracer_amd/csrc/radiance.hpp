// radiance.hpp -- launch seam of kernel_radiance.hip: primary camera rays for many cameras (drt_renderer_camera_rays) and
// path-traced radiance of caller-chosen rays (drt_renderer_radiance).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_scene.hpp"
#include "ray_query.hpp"

namespace drt {

// Camera::GetRay's per-frame constants of one camera (FrameParams' camera fields, Camera.cu:84-103, for width x height)
struct CamConst {
    float cam_pos[3], fwd_focus[3], horizontal[3], vertical[3], disk_u[3], disk_v[3];
    int32_t defocus;
    float exposure;
};
constexpr int kCamsPerLaunch = 32;              // cameras carried in one launch's arguments (2.5 KiB)

struct CameraRaysArgs {
    void *rays;                  // drt_path_ray[n_cams * width * height], 16-B aligned, entry c * width * height + x + y * width
    uint32_t width, height, n_cams, frame;
    CamConst cams[kCamsPerLaunch];
};
hipError_t launch_camera_rays(const CameraRaysArgs &args, hipStream_t stream);

struct RadianceArgs {
    const void *rays;            // drt_path_ray[n] (32 B, 16-B aligned)
    float4 *out;                 // float4[n]
    QueryFrame frame;            // n, tree depth, refill threshold, claim heads, HBM stack: the closest-hit ray query's 8 B stack entries
    int32_t accumulate;          // 0: out = (c, 1); else out.rgb += c, alpha kept
};
// The path loop of RayGen for every ray, with the renderer's settings and material model in `frame` (FrameParams: sun, sky,
// bounce limit, tone curve, gamma, ext_*; its camera and framebuffer fields are not read).  `alpha`: the scene has an RGBA
// texture (AnyHit may reject hits).  The grid is at most the ray query's resident grid, so its HBM stack serves here too.
hipError_t launch_radiance(const SceneView &scene, const FrameParams &frame, bool alpha, const RadianceArgs &args, int num_cus,
                           hipStream_t stream);

}  // namespace drt
