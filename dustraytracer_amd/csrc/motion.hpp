// motion.hpp -- launch seam of kernel_motion.hip: the temporal reprojection through geometry that a device refit moved, and the
// screen-space motion-vector buffer (drt_renderer_track_motion / _motion_vectors, include/drt.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "temporal.hpp"

namespace drt {

// The current TriHot records and the snapshot the first refit since the last temporal call took of them (48 B each, read as
// three float4); the kernels compare the nine words v0, e1, e2 of the two themselves.
struct MotionGeometry {
    const float4 *hot;           // TriHot[n_tris] as it is now
    const float4 *snapshot;      // TriHot[n_tris] of the previous call's geometry, NULL = nothing moved (every pixel static)
};

// Stage (b) with the moved rule: temporal_reproject_kernel restated with P' and n' of include/drt.h, then kernel_temporal.hip's own
// variance pass (launch_temporal_variance).
hipError_t launch_motion_reproject(const ReprojectArgs &args, const MotionGeometry &geo, hipStream_t stream);

// out[x + y * width] = (fx - x, fy - y, z, flag) of P' in the camera args.pc; reads args.guides, the cameras, width and height only.
hipError_t launch_motion_vectors(const ReprojectArgs &args, const MotionGeometry &geo, float4 *out, hipStream_t stream);

}  // namespace drt
