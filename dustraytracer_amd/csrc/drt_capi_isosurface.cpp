// drt_capi_isosurface.cpp -- the isosurface entry point of include/drt.h (drt_renderer_isosurface, kernel_isosurface.hip): every
// argument check before any device work, in drt_renderer_plane_sections' order and style, then device memory and the launch.  The call
// reads no scene and no tree and shares no scratch with the queries, so it uploads nothing and orders itself by its stream alone.
#include "renderer_state.hpp"

#include <cmath>

#include "isosurface.hpp"

using namespace drt;

extern "C" {

int drt_renderer_isosurface(drt_renderer *r, const float *field, const drt_grid *grid, float level, float border, int32_t flip,
                            const uint32_t *offsets, drt_iso_tri *out, uint32_t out_capacity, uint32_t *counts, void *hip_stream) {
    if (!r || !field || !grid) return fail(DRT_ERR_INVALID, "null argument");
    if (flip != 0 && flip != 1) return fail(DRT_ERR_INVALID, "flip " + std::to_string(flip) + ": 0 or 1 expected");
    if (!out && !counts) return fail(DRT_ERR_INVALID, "out and counts are both null: nothing to write");
    if ((out == nullptr) != (out_capacity == 0)) return fail(DRT_ERR_INVALID, "out must be null if and only if out_capacity is 0");
    if (out && !offsets) return fail(DRT_ERR_INVALID, "null offset pointer: a fill needs the rows' segments");
    if (((uintptr_t)out & 15u) != 0 || ((uintptr_t)field & 3u) != 0 || ((uintptr_t)offsets & 3u) != 0 || ((uintptr_t)counts & 3u) != 0)
        return fail(DRT_ERR_INVALID, "out must be 16-byte aligned, field, offsets and counts 4-byte aligned");
    const bool has_border = !std::isnan(border);
    if (has_border && !std::isfinite(border)) return fail(DRT_ERR_INVALID, "border: a finite value, or NaN for none, expected");
    const uint32_t least = has_border ? 1u : 2u;
    uint64_t samples = 1, cubes = 1;
    for (int k = 0; k < 3; k++) {
        if (grid->dims[k] < least)
            return fail(DRT_ERR_INVALID, "dims[" + std::to_string(k) + "] = " + std::to_string(grid->dims[k]) + ": at least " +
                                             std::to_string(least) + " samples per axis expected (1 with a border, else 2)");
        if (grid->dims[k] > 0x7fffffffu) return fail(DRT_ERR_INVALID, "fewer than 2^31 samples expected");
        samples *= grid->dims[k];
        cubes *= has_border ? (uint64_t)grid->dims[k] + 1 : (uint64_t)grid->dims[k] - 1;
        if (samples > 0x7fffffffu || cubes > 0x7fffffffu) return fail(DRT_ERR_INVALID, "fewer than 2^31 samples and fewer than 2^31 cubes expected");
    }
    if (!std::isfinite(level)) return fail(DRT_ERR_INVALID, "level: a finite value expected");
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(grid->lo[k]) || !std::isfinite(grid->cell[k])) return fail(DRT_ERR_INVALID, "lo and cell: finite values expected");
    if (r->pending) return fail(DRT_ERR_INVALID, "an asynchronous render batch is pending: drt_renderer_wait first");
    HIP_TRY(hipSetDevice(r->device));
    (void)hipGetLastError();                   // (see render_batch_impl: only this call's own errors count)
    if (!on_renderer_device(r, field) || (offsets && !on_renderer_device(r, offsets)) || (out && !on_renderer_device(r, out)) ||
        (counts && !on_renderer_device(r, counts)))
        return fail(DRT_ERR_INVALID, "field, offsets, out and counts must be device memory on the renderer's device");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : r->stream;
    IsoArgs a;
    a.field = field; a.offsets = offsets; a.out = out; a.counts = counts; a.out_capacity = out_capacity;
    for (int k = 0; k < 3; k++) {
        a.dims[k] = grid->dims[k];
        a.cubes[k] = has_border ? grid->dims[k] + 1 : grid->dims[k] - 1;
        a.lo[k] = grid->lo[k]; a.cell[k] = grid->cell[k];
    }
    a.rows = a.cubes[1] * a.cubes[2];
    a.waves = iso_waves(a.rows, r->num_cus, out != nullptr);
    a.pad = has_border ? 1 : 0;
    a.swap = flip;
    a.level = level; a.border = border;
    HIP_TRY(launch_isosurface(out != nullptr, a, s));
    return DRT_OK;
}

}  // extern "C"
