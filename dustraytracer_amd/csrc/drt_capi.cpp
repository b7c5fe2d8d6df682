// drt_capi.cpp -- the C ABI of include/drt.h: scene handles, the renderer's lifecycle (device buffers, per-call constants, launches,
// read-back), render batches, ray and radiance queries, refit, the debug entry points and error reporting.  The guide pass and the
// filter stages (denoise, temporal, motion vectors, upscale) are in drt_capi_filters.cpp, adaptive sampling is in
// drt_capi_adaptive.cpp, what they share in renderer_state.hpp.
//
// Replaces class Renderer (Core/Renderer.hpp:14-47, Core/Renderer.cu) and InvokeRenderKernel
// (Core/Kernel/RenderKernel.cu:37-58).  No GL interop: the framebuffer is a device float4 array.
#include "renderer_state.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <stdexcept>

#include "ray_query.hpp"
#include "nearest.hpp"
#include "sphere_cast.hpp"
#include "crossings.hpp"
#include "list_hits.hpp"
#include "near_list.hpp"
#include "overlap.hpp"
#include "tri_overlap.hpp"
#include "section.hpp"
#include "bvh_build_device.hpp"
#include "png_decode.hpp"
#include "pool_index.hpp"

using namespace drt;

namespace {

thread_local std::string g_error;

int from_exception() {
    try {
        throw;
    } catch (const UnsupportedError &e) { return fail(DRT_ERR_UNSUPPORTED, e.what());
    } catch (const IoError &e) { return fail(DRT_ERR_IO, e.what());
    } catch (const BvhError &e) { return fail(DRT_ERR_BVH, e.what());
    } catch (const DeviceError &e) { return fail(DRT_ERR_DEVICE, e.what());
    } catch (const std::invalid_argument &e) { return fail(DRT_ERR_INVALID, e.what());
    } catch (const std::bad_alloc &) { return fail(DRT_ERR_INVALID, "out of host memory");
    } catch (const std::exception &e) { return fail(DRT_ERR_PARSE, e.what());
    } catch (...) { return fail(DRT_ERR_INVALID, "unknown error"); }
}

}  // namespace

int drt::fail(int code, const std::string &msg) {
    g_error = msg;
    return code;
}

// ------------------------------------------------------------------ steps that several entry points take (renderer_state.hpp)
static int copy_scene(drt_renderer *r, const drt_scene *scene) {
    if (r->uploaded_scene == scene && r->uploaded_revision == scene->host.revision) return DRT_OK;
    PackedScene ps;
    try { ps = scene->host.pack(); } catch (...) { return from_exception(); }
    if (r->query_recorded) HIP_TRY(hipEventSynchronize(r->ev_query));     // a query launch in flight reads the old buffers
    r->free_scene();
    HIP_TRY(r->d_inner.upload(ps.inner));
    HIP_TRY(r->d_leaves.upload(ps.leaves));
    HIP_TRY(r->d_hot.upload(ps.tri_hot));
    HIP_TRY(r->d_cold.upload(ps.tri_cold));
    HIP_TRY(r->d_mats.upload(ps.mats));
    HIP_TRY(r->d_mats_ext.upload(ps.mats_ext));
    HIP_TRY(r->d_texs.upload(ps.texs));
    HIP_TRY(r->d_texels.upload(ps.texels));
    SceneView &v = r->view;
    v.inner = r->d_inner.ptr; v.leaves = r->d_leaves.ptr; v.tri_hot = r->d_hot.ptr; v.tri_cold = r->d_cold.ptr;
    v.mats = r->d_mats.ptr; v.mats_ext = r->d_mats_ext.ptr; v.texs = r->d_texs.ptr; v.texels = r->d_texels.ptr;
    v.n_inner = (uint32_t)ps.inner.size(); v.n_leaves = (uint32_t)ps.leaves.size();
    v.n_tris = (uint32_t)ps.tri_hot.size(); v.n_mats = (uint32_t)ps.mats.size(); v.n_texs = (uint32_t)ps.texs.size();
    v.root_ref = ps.root_ref;
    std::memcpy(v.root_min, ps.root_min, 12);
    std::memcpy(v.root_max, ps.root_max, 12);
    r->bvh_depth = ps.depth;
    r->scene_has_alpha = ps.any_alpha_texture;
    r->leaves_ascending = section_leaves_ascending(ps);
    path_pool_leaf_classes(ps.leaves, r->pool_t_class);
    {   // the T step's reciprocal guard is decided per batch from the largest |edge component| (pool_index.hpp); NaN must not hide in a max
        float max_edge = 0.0f;
        bool finite = true;
        for (const TriHot &t : ps.tri_hot)
            for (int c = 0; c < 3; c++)
                for (const float e : { t.e1[c], t.e2[c] }) { finite = finite && std::isfinite(e); max_edge = std::max(max_edge, std::fabs(e)); }
        r->pool_safe_dir = finite ? pool_safe_dir(max_edge) : 0.0f;
    }
    if (r->tune.t_class_set) std::memcpy(r->pool_t_class, r->tune.t_class, sizeof r->pool_t_class);
    if (r->tune.pool_verbose) std::fprintf(stderr, "path_pool leaf classes: %u %u %u\n", r->pool_t_class[0], r->pool_t_class[1], r->pool_t_class[2]);
    r->uploaded_scene = scene;
    r->uploaded_revision = scene->host.revision;
    return DRT_OK;
}

int drt::upload_scene(drt_renderer *r, const drt_scene *scene) {
    if (int rc = copy_scene(r, scene)) return rc;
    if (r->bvh_depth > 64) return fail(DRT_ERR_UNSUPPORTED, "BVH deeper than 64 levels (the reference's traversal stack, BVHTraversal.cuh:17)");
    return DRT_OK;
}

// Camera::GetRay's per-frame constants (Camera.cu:84-103) for a width x height image, computed on the host with the same fp32
// operations in the same order (host libm for tan).
CamConst drt::camera_const(const drt_camera *cam, float width, float height) {      // Camera.cu:82 takes floats
    float theta = cam->vfov_rad / 2;
    float fov_factor = tanf(theta / 2.0f);
    float aspect_ratio = width / height;
    float plane_h = 2.0f * fov_factor * cam->focus_dist;
    float plane_w = plane_h * aspect_ratio;
    V3 forward_dir = normalize(V3{ cam->forward[0], cam->forward[1], cam->forward[2] });
    V3 right_dir = normalize(cross(forward_dir, V3{ 0, 1, 0 }));
    V3 up_dir = cross(right_dir, forward_dir);
    V3 horizontal = plane_w * right_dir, vertical = plane_h * up_dir;
    const float PI = 3.14159265359f;
    float defocus_radius = cam->focus_dist * tanf((cam->defocus_angle * (PI / 180.f)) / 2.0f);
    V3 disk_u = defocus_radius * right_dir, disk_v = defocus_radius * up_dir;
    V3 fwd_focus = forward_dir * cam->focus_dist;
    auto put = [](float *dst, V3 v) { dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; };
    CamConst c;
    std::memcpy(c.cam_pos, cam->position, 12);
    put(c.fwd_focus, fwd_focus); put(c.horizontal, horizontal); put(c.vertical, vertical);
    put(c.disk_u, disk_u); put(c.disk_v, disk_v);
    c.defocus = !(cam->defocus_angle <= 0);
    c.exposure = cam->exposure;
    return c;
}

// Per-frame constants of Camera::GetRay (Camera.cu:84-103) and RayGen (RayGen.cuh:68-72), computed on the
// host with the same fp32 operations in the same order (host libm for tan/sin/cos).
// width, height: the frame the constants are for; 0 = the renderer's (a guide pass at another size: drt_renderer_upscale).
void drt::fill_frame_params(const drt_renderer *r, const drt_camera *cam, FrameParams &fp, uint32_t width, uint32_t height) {
    const drt_settings &s = r->settings;
    if (width == 0 || height == 0) { width = r->width; height = r->height; }
    auto put = [](float *dst, V3 v) { dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; };
    if (cam) {                                 // (radiance queries have no camera: their rays carry what it would give)
        const CamConst c = camera_const(cam, (float)width, (float)height);
        std::memcpy(fp.cam_pos, c.cam_pos, 12);
        std::memcpy(fp.fwd_focus, c.fwd_focus, 12); std::memcpy(fp.horizontal, c.horizontal, 12); std::memcpy(fp.vertical, c.vertical, 12);
        std::memcpy(fp.disk_u, c.disk_u, 12); std::memcpy(fp.disk_v, c.disk_v, 12);
        fp.defocus = c.defocus;
        fp.exposure = c.exposure;
    }

    float sx = sinf(s.sunlight_dir[0]), sy = sinf(s.sunlight_dir[1]), cx = cosf(s.sunlight_dir[0]);
    put(fp.sunpos, V3{ sx * (1 - sy), sy, cx * (1 - sy) } * 100.0f);
    put(fp.suncol, V3{ s.sunlight_color[0], s.sunlight_color[1], s.sunlight_color[2] } * s.sunlight_intensity);
    std::memcpy(fp.sky_color, s.sky_color, 12);
    fp.sky_intensity = s.sky_intensity;
    fp.gamma_correction = s.gamma_correction != 0; fp.tone_mapping = s.tone_mapping != 0;
    fp.enable_sunlight = s.enable_sunlight != 0;
    fp.bounce_limit = s.ray_bounce_limit;
    fp.render_mode = s.render_mode; fp.debug_mode = s.debug_mode;
    fp.ext_emissive = r->material_model.emissive != 0; fp.ext_specular = r->material_model.specular != 0;
    fp.ext_emissive_scale = r->material_model.emissive_scale;
    fp.ext_transmission = r->material_model.transmission != 0;
    fp.width = width; fp.height = height;
    fp.stripe_rows = r->stripe_rows; fp.rank = r->rank; fp.world = r->world; fp.local_rows = r->local_rows;
    fp.accum = r->cur_accum(); fp.rgba = r->cur_rgba();
    fp.counters = r->counting ? r->counters.ptr : nullptr;
    fp.vote_node = r->vote_node; fp.vote_shade = r->vote_shade; fp.vote_dir = r->vote_dir; fp.vote_spec = r->vote_spec; fp.frames_in_flight = r->frames_in_flight; fp.vote_tail_node = r->vote_tail_node; fp.vote_tail_shade = r->vote_tail_shade;
    {   // tile rows are visited with a golden-ratio stride (kernel_wave_queue.hip, DRT_CHUNK_ORDER)
        const uint32_t tiles_y = (r->local_rows + 7) / 8;
        uint32_t step = 1;
        if (tiles_y > 2 && tiles_y < 65536) {
            step = std::max<uint32_t>(1, (uint32_t)(0.6180339887 * tiles_y + 0.5));
            auto gcd = [](uint32_t a, uint32_t b) { while (b) { uint32_t t = a % b; a = b; b = t; } return a; };
            while (gcd(step, tiles_y) != 1) step++;
        }
        fp.row_step = step;
    }
    fp.leaf_chain = r->leaf_chain < 0 ? (r->bvh_depth <= 4 ? 1 : 0) : (r->leaf_chain != 0);
}

bool drt::on_renderer_device(const drt_renderer *r, const void *p) {
    hipPointerAttribute_t at;
    std::memset(&at, 0, sizeof at);
    const hipError_t e = hipPointerGetAttributes(&at, p);
    (void)hipGetLastError();
    return e == hipSuccess && (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged) && at.device == r->device;
}

int drt::query_order(drt_renderer *r, hipStream_t s) {
    if (r->query_recorded && r->query_stream != s) HIP_TRY(hipStreamWaitEvent(s, r->ev_query, 0));
    return DRT_OK;
}
int drt::query_recorded(drt_renderer *r, hipStream_t s) {
    HIP_TRY(hipEventRecord(r->ev_query, s));
    r->query_stream = s;
    r->query_recorded = true;
    return DRT_OK;
}

int drt::traversal_scratch(drt_renderer *r, hipStream_t s, bool occluded, bool heads) {
    if (heads && !r->rq_heads.ptr) HIP_TRY(r->rq_heads.alloc(kRqHeadWords));
    const size_t stack_bytes = ray_query_stack_bytes(r->num_cus, r->bvh_depth, occluded);
    if (stack_bytes > r->rq_stack.bytes()) {
        if (r->query_recorded) HIP_TRY(hipEventSynchronize(r->ev_query));      // the launch in flight uses the one that goes
        HIP_TRY(r->rq_stack.alloc(stack_bytes / sizeof(uint32_t)));
    }
    if (heads) HIP_TRY(hipMemsetAsync(r->rq_heads.ptr, 0, r->rq_heads.bytes(), s));
    return DRT_OK;
}

// operands: [first, last) with ptr_of(*it) the pointer; null ones are absent optional operands
template <class It, class PtrOf>
static int query_open_impl(drt_renderer *r, const drt_scene *scene, uint32_t n, It first, It last, PtrOf ptr_of, const char *noun,
                           const char *names, void *hip_stream, bool occluded, hipStream_t *s) {
    if (n > 0x7fffffffu) return fail(DRT_ERR_INVALID, std::string("at most 2^31 - 1 ") + noun + " per call");
    if (r->pending) return fail(DRT_ERR_INVALID, "an asynchronous render batch is pending: drt_renderer_wait first");
    HIP_TRY(hipSetDevice(r->device));
    (void)hipGetLastError();                   // (see render_batch_impl: only this call's own errors count)
    for (It it = first; it != last; ++it)
        if (ptr_of(*it) && !on_renderer_device(r, ptr_of(*it)))
            return fail(DRT_ERR_INVALID, std::string(names) + " must be device memory on the renderer's device");
    if (int rc = upload_scene(r, scene)) return rc;
    *s = hip_stream ? (hipStream_t)hip_stream : r->stream;
    if (int rc = query_order(r, *s)) return rc;
    return traversal_scratch(r, *s, occluded, true);
}

int drt::query_open(drt_renderer *r, const drt_scene *scene, uint32_t n, std::initializer_list<const void *> operands, const char *noun,
                    const char *names, void *hip_stream, bool occluded, hipStream_t *s) {
    return query_open_impl(r, scene, n, operands.begin(), operands.end(), [](const void *p) { return p; }, noun, names, hip_stream, occluded, s);
}

bool drt::query_begin(drt_renderer *r, const drt_scene *scene, uint32_t n, std::initializer_list<QueryOperand> ops, const QueryWords &w,
                      void *hip_stream, bool occluded, hipStream_t *s, int *rc) {
    const auto stop = [rc](int code) { *rc = code; return false; };
    if (!r || !scene) return stop(fail(DRT_ERR_INVALID, "null argument"));
    if (n == 0) return stop(DRT_OK);
    for (const QueryOperand &o : ops)
        if (!o.p) return stop(fail(DRT_ERR_INVALID, w.null_msg));
    for (const QueryOperand &o : ops)
        if (((uintptr_t)o.p & (o.align - 1)) != 0) return stop(fail(DRT_ERR_INVALID, w.align_msg));
    *rc = query_open_impl(r, scene, n, ops.begin(), ops.end(), [](const QueryOperand &o) { return o.p; }, w.noun, w.names, hip_stream, occluded, s);
    return *rc == DRT_OK;
}

uint32_t drt::query_stack_levels(const drt_renderer *r) { return (uint32_t)std::max(1, r->bvh_depth); }

QueryFrame drt::query_frame(const drt_renderer *r, uint32_t n) {
    QueryFrame f;
    f.n = n;
    f.stack_levels = query_stack_levels(r);
    f.refill_min = (uint32_t)r->rq_refill_min;
    f.heads = r->rq_heads.ptr;
    f.stack_hbm = r->rq_stack.ptr;
    return f;
}

int drt::whole_frame(const drt_renderer *r, const char *who) {
    if (r->world > 1) return fail(DRT_ERR_UNSUPPORTED, std::string(who) + " the whole frame: a sharded renderer (world > 1) holds only its stripes");
    return DRT_OK;
}

int drt::stage_open(drt_renderer *r, const char *who) {
    if (r->width == 0 || r->height == 0) return fail(DRT_ERR_INVALID, "ResizeBuffer has not been called");
    if (r->pending) return fail(DRT_ERR_INVALID, "an asynchronous render batch is pending: drt_renderer_wait first");
    if (int rc = who ? whole_frame(r, who) : DRT_OK) return rc;
    HIP_TRY(hipSetDevice(r->device));
    (void)hipGetLastError();                   // (see render_batch_impl: only this call's own errors count)
    return DRT_OK;
}

int drt::read_back(drt_renderer *r, const float *src, int comps, float *dst, size_t dst_floats) {
    if (!r || !dst) return fail(DRT_ERR_INVALID, "null argument");
    size_t need = (size_t)r->width * r->local_rows * (size_t)comps;
    if (dst_floats < need) return fail(DRT_ERR_INVALID, "destination too small");
    if (need == 0) return DRT_OK;
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipStreamSynchronize(r->stream));
    HIP_TRY(hipMemcpy(dst, src, need * sizeof(float), hipMemcpyDeviceToHost));
    return DRT_OK;
}

extern "C" {

int drt_abi_version(void) { return DRT_ABI_VERSION; }
int drt_internal_fail(int code, const char *msg) { return fail(code, msg ? msg : ""); }      // for the library's other translation units
const char *drt_last_error(void) { return g_error.c_str(); }

int drt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void drt_default_settings(drt_settings *s) {
    if (!s) return;
    std::memset(s, 0, sizeof *s);
    s->gamma_correction = 1; s->tone_mapping = 1; s->enable_sunlight = 0;
    s->max_samples = 500; s->ray_bounce_limit = 2; s->render_mode = 0; s->debug_mode = 0;
    s->sunlight_dir[0] = -0.803f; s->sunlight_dir[1] = 0.681f;
    s->sunlight_color[0] = 1.000f; s->sunlight_color[1] = 0.944f; s->sunlight_color[2] = 0.917f;
    s->sunlight_intensity = 30;
    s->sky_color[0] = 0.25f; s->sky_color[1] = 0.498f; s->sky_color[2] = 0.80f;
    s->sky_intensity = 20;
}

void drt_default_camera(drt_camera *c) {
    if (!c) return;
    const float PI = 3.14159265359f;             // deg2rad, Camera.cu:125-129
    c->exposure = 1;
    c->vfov_rad = 60 * (PI / 180.f);
    c->defocus_angle = 0;
    c->focus_dist = 10;
    c->position[0] = 0; c->position[1] = 2; c->position[2] = 5;
    c->forward[0] = 0; c->forward[1] = 0; c->forward[2] = -1;
}

// ------------------------------------------------------------------ scene
drt_scene *drt_scene_create(void) {
    try { return new drt_scene(); } catch (...) { from_exception(); return nullptr; }
}
void drt_scene_destroy(drt_scene *s) { delete s; }

int drt_scene_load_gltf(drt_scene *s, const char *path) {
    if (!s || !path) return fail(DRT_ERR_INVALID, "null argument");
    try { s->host.load_gltf(path); return DRT_OK; } catch (...) { return from_exception(); }
}

int drt_scene_load_gltf_ex(drt_scene *s, const char *path, uint32_t flags) {
    if (!s || !path) return fail(DRT_ERR_INVALID, "null argument");
    if (flags & ~DRT_LOAD_STRICT) return fail(DRT_ERR_INVALID, "unknown load flag");
    try { s->host.load_gltf(path, (flags & DRT_LOAD_STRICT) != 0); return DRT_OK; } catch (...) { return from_exception(); }
}

int drt_scene_set_geometry(drt_scene *s, const float *positions, const float *normals, const float *uvs,
                           const int32_t *material_ids, int32_t n_tris) {
    if (!s || n_tris < 0 || (n_tris > 0 && (!positions || !normals || !uvs || !material_ids)))
        return fail(DRT_ERR_INVALID, "null argument");
    try {
        s->host.triangles.clear(); s->host.meshes.clear();
        s->host.set_geometry(positions, normals, uvs, material_ids, n_tris);
        return DRT_OK;
    } catch (...) { return from_exception(); }
}

int drt_scene_add_material(drt_scene *s, const float albedo[3], int32_t albedo_tex) {
    if (!s || !albedo) return fail(DRT_ERR_INVALID, "null argument");
    try {
        drt_material m;
        std::memset(&m, 0, sizeof m);
        std::memcpy(m.albedo, albedo, 12);
        m.albedo_tex = albedo_tex;
        m.refractive_index = 1.45f;
        s->host.materials.push_back(m);
        s->host.revision = HostScene::next_revision();
        return (int)s->host.materials.size() - 1;
    } catch (...) { return from_exception(); }
}

int drt_scene_add_material_ex(drt_scene *s, const drt_material *m) {
    if (!s || !m) return fail(DRT_ERR_INVALID, "null argument");
    try {
        s->host.materials.push_back(*m);
        s->host.revision = HostScene::next_revision();
        return (int)s->host.materials.size() - 1;
    } catch (...) { return from_exception(); }
}

// CudaMath/Random.cu:6-17 on the host (integer hash; the float conversion is exact arithmetic): what a host-side Sampler draws from
uint32_t drt_pcg_hash(uint32_t input) {
    uint32_t state = input * 747796405u + 2891336453u;
    uint32_t word = ((state >> ((state >> 28u) + 4u)) ^ state) * 277803737u;
    return (word >> 22u) ^ word;
}
float drt_random_float(uint32_t *seed) {
    if (!seed) return 0.f;
    *seed = drt_pcg_hash(*seed);
    return (float)*seed / 4294967296.0f;
}

int drt_scene_add_texture(drt_scene *s, const uint8_t *texels, int32_t width, int32_t height, int32_t components) {
    if (!s || !texels || width <= 0 || height <= 0 || components < 1 || components > 4)
        return fail(DRT_ERR_INVALID, "bad texture");
    try {
        HostTexture t;
        t.width = width; t.height = height; t.components = components;
        t.texels.assign(texels, texels + (size_t)width * height * components);
        s->host.textures.push_back(std::move(t));
        s->host.revision = HostScene::next_revision();
        return (int)s->host.textures.size() - 1;
    } catch (...) { return from_exception(); }
}

int drt_scene_build_bvh(drt_scene *s, int32_t target_leaf_prims, int32_t bin_count) {
    if (!s) return fail(DRT_ERR_INVALID, "null scene");
    try { s->host.build_bvh(target_leaf_prims, bin_count); return DRT_OK; } catch (...) { return from_exception(); }
}

int drt_scene_build_bvh_recursive(drt_scene *s, int32_t target_leaf_prims, int32_t bin_count) {
    if (!s) return fail(DRT_ERR_INVALID, "null scene");
    try { s->host.build_bvh(target_leaf_prims, bin_count); s->host.renumber_as_recursive_build(); return DRT_OK; } catch (...) { return from_exception(); }
}

int drt_scene_build_bvh_device(drt_scene *s, int32_t target_leaf_prims, int32_t bin_count, int32_t device, float *build_ms) {
    if (!s) return fail(DRT_ERR_INVALID, "null scene");
    if (build_ms) *build_ms = 0.f;
    try {
        const float ms = s->host.build_bvh_on_device(target_leaf_prims, bin_count, device);
        if (build_ms) *build_ms = ms;
        return DRT_OK;
    } catch (...) { return from_exception(); }
}

int drt_scene_validate(const drt_scene *s) {
    if (!s) return fail(DRT_ERR_INVALID, "null scene");
    try { (void)s->host.pack(); return DRT_OK; } catch (...) { return from_exception(); }
}

int32_t drt_scene_triangle_count(const drt_scene *s) { return s ? (int32_t)s->host.triangles.size() : 0; }
int32_t drt_scene_node_count(const drt_scene *s) { return s ? (int32_t)s->host.nodes.size() : 0; }
int32_t drt_scene_material_count(const drt_scene *s) { return s ? (int32_t)s->host.materials.size() : 0; }
int32_t drt_scene_texture_count(const drt_scene *s) { return s ? (int32_t)s->host.textures.size() : 0; }
int32_t drt_scene_mesh_count(const drt_scene *s) { return s ? (int32_t)s->host.meshes.size() : 0; }
int32_t drt_scene_bvh_depth(const drt_scene *s) { return s ? s->host.bvh_depth() : 0; }

#define DRT_COPY_OUT(vec)                                                                          \
    if (!s || (!out && cap > 0) || cap < 0) return fail(DRT_ERR_INVALID, "bad argument");          \
    {                                                                                              \
        size_t n = std::min<size_t>((size_t)cap, s->host.vec.size());                              \
        if (n) std::memcpy(out, s->host.vec.data(), n * sizeof(s->host.vec[0]));                   \
        return (int)n;                                                                             \
    }

int drt_scene_get_triangles(const drt_scene *s, drt_triangle *out, int32_t cap) { DRT_COPY_OUT(triangles) }
int drt_scene_get_nodes(const drt_scene *s, drt_bvh_node *out, int32_t cap) { DRT_COPY_OUT(nodes) }
int drt_scene_get_materials(const drt_scene *s, drt_material *out, int32_t cap) { DRT_COPY_OUT(materials) }
int drt_scene_get_meshes(const drt_scene *s, drt_mesh *out, int32_t cap) { DRT_COPY_OUT(meshes) }
int drt_scene_get_triangle_order(const drt_scene *s, int32_t *out, int32_t cap) { DRT_COPY_OUT(load_index) }

int drt_scene_refit(drt_scene *s, const float *positions, const float *normals) {
    if (!s) return fail(DRT_ERR_INVALID, "null scene");
    try { s->host.refit(positions, normals); return DRT_OK; } catch (...) { return from_exception(); }
}

int drt_scene_get_texture_info(const drt_scene *s, int32_t index, drt_texture_info *out) {
    if (!s || !out || index < 0 || (size_t)index >= s->host.textures.size()) return fail(DRT_ERR_INVALID, "bad texture index");
    const HostTexture &t = s->host.textures[(size_t)index];
    out->width = t.width; out->height = t.height; out->components = t.components;
    return DRT_OK;
}

int drt_scene_get_texture_texels(const drt_scene *s, int32_t index, uint8_t *out, size_t cap) {
    if (!s || !out || index < 0 || (size_t)index >= s->host.textures.size()) return fail(DRT_ERR_INVALID, "bad texture index");
    const HostTexture &t = s->host.textures[(size_t)index];
    if (cap < t.texels.size()) return fail(DRT_ERR_INVALID, "destination too small");
    std::memcpy(out, t.texels.data(), t.texels.size());
    return DRT_OK;
}

// ------------------------------------------------------------------ renderer
uint32_t drt_shard_rows(uint32_t height, uint32_t stripe_rows, uint32_t rank, uint32_t world) {
    if (stripe_rows == 0 || world == 0 || rank >= world) return 0;
    uint32_t stripes = (height + stripe_rows - 1) / stripe_rows, rows = 0;
    for (uint32_t s = rank; s < stripes; s += world)
        rows += std::min(stripe_rows, height - s * stripe_rows);
    return rows;
}

static int realloc_buffers(drt_renderer *r) {
    HIP_TRY(hipSetDevice(r->device));
    r->accum.release();
    r->rgba.release();
    r->free_stages();
    r->local_rows = drt_shard_rows(r->height, r->stripe_rows, r->rank, r->world);
    size_t px = std::max<size_t>((size_t)r->width * r->local_rows, 1);
    HIP_TRY(r->accum.alloc(px * 3));
    HIP_TRY(r->rgba.alloc_zeroed(px * 4));
    return drt_renderer_reset(r);
}

drt_renderer *drt_renderer_create(int32_t device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        fail(DRT_ERR_DEVICE, "no usable HIP device: this library has no CPU fallback");
        return nullptr;
    }
    if (device < 0 || device >= n) { fail(DRT_ERR_INVALID, "device index out of range"); return nullptr; }
    if (hipSetDevice(device) != hipSuccess) { fail(DRT_ERR_DEVICE, "hipSetDevice failed"); return nullptr; }
    drt_renderer *r = nullptr;
    try { r = new drt_renderer(); } catch (...) { from_exception(); return nullptr; }
    r->device = device;
    drt_default_settings(&r->settings);
    Tuning &t = r->tune;
    const char *which = std::getenv("DRT_KERNEL");
    if (which && std::strcmp(which, "pixel_walk") == 0) t.kernel = Tracer::pixel_walk;
    if (which && std::strcmp(which, "wave_queue") == 0) t.kernel = Tracer::wave_queue;
    if (t.kernel == Tracer::pixel_walk && !pixel_walk_built_in()) {
        fail(DRT_ERR_UNSUPPORTED, "DRT_KERNEL=pixel_walk: that kernel is not part of this library (the tests build libdrt_hip_pixel_walk.so: make pixel-walk)");
        delete r;
        return nullptr;
    }
    const char *filter = std::getenv("DRT_FILTER_KERNEL");
    if (filter && std::strcmp(filter, "lds") == 0) r->filter_kernel = FilterKernel::lds;
    if (filter && std::strcmp(filter, "taps") == 0) r->filter_kernel = FilterKernel::taps;
    auto env_int = [](const char *name, int dflt) { const char *v = std::getenv(name); return (v && *v) ? std::atoi(v) : dflt; };
    r->vote_node = std::max(1, env_int("DRT_VOTE_N", r->vote_node));
    r->vote_shade = std::max(1, env_int("DRT_VOTE_S", r->vote_shade));
    r->vote_dir = std::max(1, env_int("DRT_VOTE_R", r->vote_dir));
    r->vote_spec = std::max(1, env_int("DRT_VOTE_P", r->vote_spec));
    r->vote_tail_node = std::max(1, env_int("DRT_VOTE_TN", r->vote_tail_node));
    r->vote_tail_shade = std::max(1, env_int("DRT_VOTE_TS", r->vote_tail_shade));
    r->leaf_chain = env_int("DRT_LEAF_CHAIN", r->leaf_chain);
    r->sample_budget = (size_t)std::max(1, env_int("DRT_SAMPLE_MB", 1024)) << 20;
    t.pool_scene_bytes = (size_t)env_int("DRT_POOL_SCENE_KB", (int)(kLdsSceneBytes / 1024)) * 1024;
    t.lds_scene_bytes = (size_t)env_int("DRT_LDS_SCENE_KB", (int)(kLdsSceneBytes / 1024)) * 1024;
    t.pool_hbm = env_int("DRT_POOL_HBM", 1) != 0;
    t.pool_verbose = std::getenv("DRT_POOL_VERBOSE") != nullptr;
    if (const char *e = std::getenv("DRT_POOL_T_CLASSES")) t.t_class_set = std::sscanf(e, "%u,%u,%u", &t.t_class[0], &t.t_class[1], &t.t_class[2]) == 3;
    t.threads = env_int("DRT_POOL_THREADS", 0); t.paths = env_int("DRT_POOL_PATHS", 0); t.stack_lds = env_int("DRT_POOL_STACK_LDS", t.stack_lds);
    t.min_fill = env_int("DRT_POOL_MIN_FILL", t.min_fill); t.patience = env_int("DRT_POOL_PATIENCE", t.patience);
    t.n_loop = env_int("DRT_POOL_N_LOOP", t.n_loop); t.n_min_lanes = env_int("DRT_POOL_N_MIN", t.n_min_lanes);
    t.n_fuse_loop = env_int("DRT_POOL_N_FUSE_LOOP", t.n_fuse_loop); t.n_fuse_min = env_int("DRT_POOL_N_FUSE_MIN", t.n_fuse_min);
    t.cold_lds_kb = env_int("DRT_POOL_COLD_KB", t.cold_lds_kb); t.share_grid = env_int("DRT_POOL_SHARE_GRID", t.share_grid);
    t.dir_tries = env_int("DRT_POOL_DIR_TRIES", t.dir_tries);
    // launches of different streams that reliably run side by side (pool_share.hpp): the HIP runtime spreads a process's streams over
    // GPU_MAX_HW_QUEUES hardware queues (4 unless the environment says otherwise) and reads that variable once, when it starts -- so
    // it is read once per process here too, by the first renderer (the device count above has started the runtime by then): a change
    // made later reaches neither.  DRT_POOL_HW_QUEUES (tests) stands in for it per renderer; DRT_POOL_SHARE_MAX sets the result itself.
    static const int process_hw_queues = env_int("GPU_MAX_HW_QUEUES", 0);
    t.hw_queues = env_int("DRT_POOL_HW_QUEUES", process_hw_queues);
    t.share_max = std::max(0, env_int("DRT_POOL_SHARE_MAX", 0));
    if (env_int("DRT_POOL_STATS", 0) != 0 && hipMalloc((void **)&t.stats, 40 * sizeof(unsigned long long)) == hipSuccess)
        (void)hipMemset(t.stats, 0, 40 * sizeof(unsigned long long));
    t.wq_only_small = env_int("DRT_WG_THREADS", 0) == 256; t.wq_only_wide = env_int("DRT_STACK_REF16", 1) == 0; t.wq_tris_wide = env_int("DRT_TRIS_WIDE", 1) != 0;
    if (std::getenv("DRT_MAX_BLOCKS_PER_CU")) t.max_blocks_per_cu = std::max(1, env_int("DRT_MAX_BLOCKS_PER_CU", 1));
    if (std::getenv("DRT_CHUNKS_PER_WG")) t.chunks_per_wg = std::max(1, env_int("DRT_CHUNKS_PER_WG", 1));
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) r->num_cus = cus;
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz > 0) r->wall_clock_khz = khz;
    r->rq_refill_min = std::min(64, std::max(1, env_int("DRT_RQ_REFILL", r->rq_refill_min)));
    r->rf_top_nodes = std::max(0, env_int("DRT_REFIT_TOP", r->rf_top_nodes));
    r->section_waves = std::max(0, env_int("DRT_SECTION_WAVES", r->section_waves));
    if (const char *route = std::getenv("DRT_ADJACENCY")) r->adjacency_host = std::strcmp(route, "host") == 0;
    if (r->ev_start.create() != hipSuccess || r->ev_stop.create() != hipSuccess ||
        r->ev_query.create(hipEventDisableTiming) != hipSuccess ||
        r->counters.alloc(sizeof(drt_counters) / sizeof(unsigned long long)) != hipSuccess ||
        r->records.alloc_zeroed(4 * (size_t)drt_renderer::kRecords) != hipSuccess ||
        r->records_host.alloc(4 * (size_t)drt_renderer::kMaxSpans) != hipSuccess ||
        r->tile_counter.alloc_zeroed((size_t)drt_renderer::kCounters * kQueueHeadBlockWords) != hipSuccess) {
        fail(DRT_ERR_DEVICE, "cannot create HIP events / counter buffer");
        drt_renderer_destroy(r);
        return nullptr;
    }
    return r;
}

void drt_renderer_destroy(drt_renderer *r) { delete r; }         // (~drt_renderer selects the device; the members release)

int drt_renderer_reset(drt_renderer *r) {                      // Renderer.cu:132-136
    if (!r) return fail(DRT_ERR_INVALID, "null renderer");
    HIP_TRY(hipSetDevice(r->device));
    if (r->cur_accum() && r->width && r->local_rows)
        HIP_TRY(hipMemsetAsync(r->cur_accum(), 0, (size_t)r->width * r->local_rows * 3 * sizeof(float), r->stream));
    r->frame_index = 1;
    r->free_adaptive();                        // (adaptive calls are blocking: nothing in flight reads the state; no state, no work)
    return DRT_OK;
}

int drt_renderer_resize(drt_renderer *r, uint32_t width, uint32_t height) {   // Renderer.cu:29-78
    if (!r) return fail(DRT_ERR_INVALID, "null renderer");
    if (width == r->width && height == r->height) return DRT_OK;
    if ((uint64_t)width * height > (1ull << 31)) return fail(DRT_ERR_INVALID, "framebuffer too large (pixel index is 32-bit, RayGen.cuh:74)");
    if (r->ext_accum || r->ext_rgba) return fail(DRT_ERR_INVALID, "unbind external buffers before resizing");
    r->width = width; r->height = height;
    return realloc_buffers(r);
}

int drt_renderer_set_shard(drt_renderer *r, uint32_t stripe_rows, uint32_t rank, uint32_t world) {
    if (!r || stripe_rows == 0 || world == 0 || rank >= world) return fail(DRT_ERR_INVALID, "bad shard description");
    if (r->ext_accum || r->ext_rgba) return fail(DRT_ERR_INVALID, "unbind external buffers before re-sharding");
    r->stripe_rows = stripe_rows; r->rank = rank; r->world = world;
    return r->width && r->height ? realloc_buffers(r) : DRT_OK;
}

int drt_renderer_bind_buffers(drt_renderer *r, void *device_accum, void *device_rgba) {
    if (!r) return fail(DRT_ERR_INVALID, "null renderer");
    if ((device_accum == nullptr) != (device_rgba == nullptr)) return fail(DRT_ERR_INVALID, "bind both buffers or neither");
    r->ext_accum = (float *)device_accum;
    r->ext_rgba = (float *)device_rgba;
    return DRT_OK;
}

int drt_renderer_set_stream(drt_renderer *r, void *hip_stream) {
    if (!r) return fail(DRT_ERR_INVALID, "null renderer");
    if (r->stream != (hipStream_t)hip_stream) {
        // launches still running on the old stream own queue-head counters that the new stream's bulk re-zero must not touch
        HIP_TRY(hipSetDevice(r->device));
        HIP_TRY(hipStreamSynchronize(r->stream));
    }
    r->stream = (hipStream_t)hip_stream;
    return DRT_OK;
}

int drt_renderer_set_settings(drt_renderer *r, const drt_settings *s) {
    if (!r || !s) return fail(DRT_ERR_INVALID, "null argument");
    r->settings = *s;
    return DRT_OK;
}
int drt_renderer_set_material_model(drt_renderer *r, const drt_material_model *m) {
    if (!r || !m) return fail(DRT_ERR_INVALID, "null argument");
    r->material_model = *m;
    return DRT_OK;
}
int drt_renderer_get_material_model(const drt_renderer *r, drt_material_model *out) {
    if (!r || !out) return fail(DRT_ERR_INVALID, "null argument");
    *out = r->material_model;
    return DRT_OK;
}
int drt_renderer_get_settings(const drt_renderer *r, drt_settings *out) {
    if (!r || !out) return fail(DRT_ERR_INVALID, "null argument");
    *out = r->settings;
    return DRT_OK;
}

uint32_t drt_renderer_width(const drt_renderer *r) { return r ? r->width : 0; }
uint32_t drt_renderer_height(const drt_renderer *r) { return r ? r->height : 0; }
uint32_t drt_renderer_sample_count(const drt_renderer *r) { return r ? r->frame_index : 0; }
uint32_t drt_renderer_local_rows(const drt_renderer *r) { return r ? r->local_rows : 0; }
void *drt_renderer_device_rgba(drt_renderer *r) { return r ? r->cur_rgba() : nullptr; }
void *drt_renderer_device_accum(drt_renderer *r) { return r ? r->cur_accum() : nullptr; }

int drt_renderer_set_counting(drt_renderer *r, int32_t enable) {
    if (!r) return fail(DRT_ERR_INVALID, "null renderer");
    r->counting = enable != 0;
    return DRT_OK;
}

int drt_renderer_get_counters(drt_renderer *r, drt_counters *out) {
    if (!r || !out) return fail(DRT_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipStreamSynchronize(r->stream));
    HIP_TRY(hipMemcpy(out, r->counters.ptr, sizeof *out, hipMemcpyDeviceToHost));
    return DRT_OK;
}

// Camera.cu:61-80.  helper_math.cuh: cross(a,b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x),
// dot = a.x*b.x + a.y*b.y + a.z*b.z; every product and sum rounds on its own (-ffp-contract=off).
static void rotate_about(float v[3], const float k[3], float s, float c) {
    const float kxv[3] = { k[1] * v[2] - k[2] * v[1], k[2] * v[0] - k[0] * v[2], k[0] * v[1] - k[1] * v[0] };
    const float d = k[0] * v[0] + k[1] * v[1] + k[2] * v[2];
    const float one_minus_c = 1 - c;
    float r[3];
    for (int i = 0; i < 3; i++) r[i] = ((v[i] * c) + (kxv[i] * s)) + ((k[i] * d) * one_minus_c);
    for (int i = 0; i < 3; i++) v[i] = r[i];
}

void drt_camera_rotate(float forward[3], float right[3], const float up[3], const float delta[4]) {
    if (!forward || !right || !up || !delta) return;
    rotate_about(forward, up, delta[0], delta[1]);
    rotate_about(forward, right, delta[2], delta[3]);
    const float r[3] = { forward[1] * up[2] - forward[2] * up[1], forward[2] * up[0] - forward[0] * up[2],
                         forward[0] * up[1] - forward[1] * up[0] };
    for (int i = 0; i < 3; i++) right[i] = r[i];
}

// Camera.cu:44-58 (glm::mat3 * vec3 = col0*v.x + col1*v.y + col2*v.z, then m_Position += speed * move * delta)
void drt_camera_move(float position[3], const float right[3], const float up[3], const float forward[3],
                     const float velocity[3], float speed, float delta) {
    if (!position || !right || !up || !forward || !velocity) return;
    for (int i = 0; i < 3; i++) {
        const float move = (right[i] * velocity[0] + up[i] * velocity[1]) + forward[i] * velocity[2];
        position[i] = position[i] + (speed * move) * delta;
    }
}

int drt_renderer_set_frames_in_flight(drt_renderer *r, int32_t n) {
    if (!r || n < 1) return fail(DRT_ERR_INVALID, "bad argument");
    r->frames_in_flight = n;
    return DRT_OK;
}

int drt_renderer_kernel_span(const drt_renderer *r, float *ms) {
    if (!r || !ms) return fail(DRT_ERR_INVALID, "bad argument");
    *ms = r->span_ms;
    return DRT_OK;
}

int32_t drt_renderer_launch_count(const drt_renderer *r) { return r ? r->launches_last : 0; }

// path_pool<lean|materials[+alpha][+sun],lds-scene|hbm-scene>, wave_queue<lean|general|counting[+alpha][+sun],...> or pixel_walk<stackN>,
// then the shape of the last launch
int drt_renderer_kernel_info(const drt_renderer *r, char *buf, size_t cap) {
    if (!r || !buf || cap == 0) return fail(DRT_ERR_INVALID, "bad argument");
    static const char *const wave_queue_builds[6] = { "lean", "general", "counting", "lean+alpha", "lean+sun", "lean+alpha+sun" };
    const TracerChoice &c = r->choice;
    const LaunchShape &s = r->shape;
    char stack[48];
    if (s.levels_in_lds < s.stack_levels) std::snprintf(stack, sizeof stack, "%d(%d in LDS)", s.stack_levels, s.levels_in_lds);
    else std::snprintf(stack, sizeof stack, "%d", s.stack_levels);
    if (c.family == Tracer::path_pool)
        std::snprintf(buf, cap, "path_pool<%s%s%s,%s> stack=%s wg/CU=%d threads=%d paths=%d lds=%dKiB", (c.pool_flags & 16) ? "materials" : "lean",
                      (c.pool_flags & 4) ? "+alpha" : "", (c.pool_flags & 2) ? "+sun" : "", (c.pool_flags & 8) ? "hbm-scene" : "lds-scene", stack,
                      s.groups_per_cu, s.threads, s.paths, s.lds_kib);
    else if (c.family == Tracer::wave_queue)
        std::snprintf(buf, cap, "wave_queue<%s,%s> stack=%s%s wg/CU=%d%s lds=%dKiB", wave_queue_builds[c.wq_mode], c.wq_lds_scene ? "lds-scene" : "hbm-scene",
                      stack, s.entry_bytes == 6 ? "x6B" : (s.tris == 3 ? " tris=3" : ""), s.groups_per_cu, s.threads >= 512 ? "x512" : "", s.lds_kib);
    else if (c.family == Tracer::pixel_walk)
        std::snprintf(buf, cap, "pixel_walk<stack%d>", c.stack);
    else
        buf[0] = 0;
    return DRT_OK;
}

// The tracing kernel of a batch and its build: every rule that chooses one is here.  Returns nullptr, or why the
// batch cannot be rendered (DRT_ERR_UNSUPPORTED).
static const char *choose_tracer(const Tuning &tune, const SceneView &sc, int bvh_depth, bool scene_has_alpha, const FrameParams &fp, TracerChoice &c) {
    const bool material = fp.ext_emissive || fp.ext_specular || fp.ext_transmission, counting = fp.counters != nullptr;
    c = TracerChoice{};
    if (tune.kernel == Tracer::pixel_walk && !material) {        // (round 1's kernel has no material model)
        c.family = Tracer::pixel_walk;
        c.stack = bvh_depth <= 8 ? 8 : (bvh_depth <= 16 ? 16 : (bvh_depth <= 32 ? 32 : 64));      // (a stack never holds more than `depth` entries)
        return nullptr;
    }
    // path_pool: no debug views, bounce index in 16 bits (15 in the material-model builds), stack height in 8, no statistics build of
    // the material model; the lds-scene build has 12-bit triangle indices, the hbm-scene build 16-bit node references on its stacks
    const size_t scene_bytes = wave_queue_scene_lds_bytes(sc);
    const bool pool = tune.kernel == Tracer::path_pool && fp.render_mode == 0 && fp.bounce_limit <= (material ? 30000 : 60000) && bvh_depth <= 200 &&
                      sc.root_ref != kNoNode && !(counting && material);
    const bool in_lds = pool && scene_bytes <= tune.pool_scene_bytes && sc.n_tris < 4095u && path_pool_fits(sc, bvh_depth, scene_bytes, false);
    if (in_lds || (pool && tune.pool_hbm && sc.n_inner < 32768u && sc.n_leaves < 32768u && path_pool_fits(sc, bvh_depth, 0, true))) {
        c.family = Tracer::path_pool;
        c.pool_flags = ((counting || tune.stats) && !material ? 1 : 0) | (fp.enable_sunlight ? 2 : 0) | (scene_has_alpha ? 4 : 0) | (in_lds ? 0 : 8) | (material ? 16 : 0);
        return nullptr;
    }
    if (fp.ext_transmission)
        return "the dielectric lobe of drt_material_model is rendered by path_pool only (not: debug views, counting, DRT_KERNEL=wave_queue or pixel_walk, "
               "trees beyond 32 767 nodes, bounce limits beyond 30 000)";
    // wave_queue: the counting build, the general one (debug views, the emissive term and mirror lobe), else lean
    c.family = Tracer::wave_queue;
    c.wq_mode = counting ? 2 : ((material || fp.render_mode != 0) ? 1 : (fp.enable_sunlight ? (scene_has_alpha ? 5 : 4) : (scene_has_alpha ? 3 : 0)));
    // (a small scene under a degenerate, very deep tree: the stacks of one 256-thread group, 8 bytes per level and lane, and the scene
    // copy must fit the CU's 160 KB together, else the tree is read from HBM and the stacks have the LDS to themselves)
    c.wq_lds_scene = scene_bytes <= tune.lds_scene_bytes && scene_bytes + (size_t)std::max(bvh_depth, 1) * 256 * 8 <= 160u * 1024u;
    return nullptr;
}

static int render_batch_impl(drt_renderer *r, const drt_camera *cam, const drt_scene *scene, uint32_t n_frames,
                             float *delta_ms, bool blocking) {
    if (!r || !cam || !scene) return fail(DRT_ERR_INVALID, "null argument");
    if (delta_ms) *delta_ms = 0.f;
    r->pending = false;
    if (r->width == 0 || r->height == 0) return fail(DRT_ERR_INVALID, "ResizeBuffer has not been called");
    // Renderer.cu:82: nothing happens once m_FrameIndex == max_samples, so at most max_samples-1 frames accumulate.
    if ((int64_t)r->frame_index == (int64_t)r->settings.max_samples) return DRT_OK;
    if (r->settings.max_samples > 0 && r->frame_index < (uint32_t)r->settings.max_samples)
        n_frames = std::min<uint32_t>(n_frames, (uint32_t)r->settings.max_samples - r->frame_index);
    if (n_frames == 0) return DRT_OK;
    HIP_TRY(hipSetDevice(r->device));
    // hipGetLastError() after a launch reports the last error of ANY earlier runtime call of this thread -- also one that another
    // library made and handled (RCCL probing peers answers "invalid device ordinal" on a one-GPU box): start from a clean slate
    (void)hipGetLastError();
    if (int rc = upload_scene(r, scene)) return rc;

    FrameParams fp;
    std::memset(&fp, 0, sizeof fp);
    fill_frame_params(r, cam, fp);
    fp.frame_first = r->frame_index;
    fp.n_frames = n_frames;
    if (const char *why = choose_tracer(r->tune, r->view, r->bvh_depth, r->scene_has_alpha, fp, r->choice)) return fail(DRT_ERR_UNSUPPORTED, why);
    const TracerChoice &choice = r->choice;
    r->shape = LaunchShape{};
    if (r->counting) HIP_TRY(hipMemsetAsync(r->counters.ptr, 0, sizeof(drt_counters), r->stream));

    r->spans_used = 0;
    HIP_TRY(hipEventRecord(r->ev_start, r->stream));                   // Renderer.cu:97
    if (choice.family == Tracer::pixel_walk) {
        HIP_TRY(launch_render(r->view, fp, choice, r->counting, r->stream));
        r->launches_last = 1;
    } else {
        // split the batch so that the per-sample colour buffer of one launch stays within the budget
        const size_t per_frame = (size_t)r->width * r->local_rows * 4 * sizeof(float);
        uint32_t frames_per_launch = (uint32_t)std::max<size_t>(1, std::min<size_t>(n_frames, r->sample_budget / std::max<size_t>(per_frame, 1)));
        const size_t need = per_frame * frames_per_launch;
        if (need > r->samples.bytes()) HIP_TRY(r->samples.alloc(need / sizeof(float4)));
        r->spans_used = 0;
        r->launches_last = 0;
        if (r->records_used + drt_renderer::kMaxSpans > drt_renderer::kRecords) {      // stream order: every launch that used them is over by then
            HIP_TRY(hipMemsetAsync(r->records.ptr, 0, r->records.bytes(), r->stream));
            r->records_used = 0;
        }
        r->batch_first_record = r->records_used;
        for (uint32_t done = 0; done < n_frames; done += frames_per_launch) {
            fp.frame_first = r->frame_index + done;
            fp.n_frames = std::min(frames_per_launch, n_frames - done);
            unsigned long long *const record = r->spans_used < drt_renderer::kMaxSpans ? r->records.ptr + 4 * (size_t)(r->batch_first_record + r->spans_used++) : nullptr;
            if (record) r->records_used++;
            fp.span = record;
            unsigned int *const launch_status = record ? reinterpret_cast<unsigned int *>(record + 2) : nullptr;     // (beyond kMaxSpans launches per batch: no status word, the kernel still aborts cleanly)
            r->launches_last++;
            if (r->counters_used == drt_renderer::kCounters) {      // stream order: every launch that used them is over by then
                HIP_TRY(hipMemsetAsync(r->tile_counter.ptr, 0, r->tile_counter.bytes(), r->stream));
                r->counters_used = 0;
            }
            unsigned int *const queue_head = r->tile_counter.ptr + (size_t)(r->counters_used++) * kQueueHeadBlockWords;
            if (choice.family == Tracer::path_pool)
                HIP_TRY(launch_path_pool(r->view, fp, r->bvh_depth, choice, r->pool_t_class, r->pool_safe_dir, r->tune, r->pool_scratch, queue_head, r->samples.ptr, launch_status,
                                         r->num_cus, r->stream, &r->shape));
            else
                HIP_TRY(launch_wave_queue(r->view, fp, r->bvh_depth, choice, r->tune, queue_head, r->samples.ptr, r->num_cus, r->stream, &r->shape, r->wq_cache));
        }
    }
    // the launches' records (execution span, status bits) travel to pinned host memory on the stream: drt_renderer_wait reads them
    // after the event, no second round trip to the device (a 1/8-shard step is 0.4 ms)
    if (r->spans_used > 0)
        HIP_TRY(hipMemcpyAsync(r->records_host.ptr, r->records.ptr + 4 * (size_t)r->batch_first_record, sizeof(unsigned long long) * 4 * (size_t)r->spans_used, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipEventRecord(r->ev_stop, r->stream));                    // Renderer.cu:105
    r->frame_index += n_frames;                                        // Renderer.cu:116
    r->pending = true;
    if (!blocking) return DRT_OK;
    return drt_renderer_wait(r, delta_ms);                             // blocking, Renderer.cu:106-108
}

int drt_renderer_render_batch(drt_renderer *r, const drt_camera *cam, const drt_scene *scene, uint32_t n_frames,
                              float *delta_ms) {
    return render_batch_impl(r, cam, scene, n_frames, delta_ms, true);
}

int drt_renderer_render_batch_async(drt_renderer *r, const drt_camera *cam, const drt_scene *scene, uint32_t n_frames) {
    return render_batch_impl(r, cam, scene, n_frames, nullptr, false);
}

int drt_renderer_wait(drt_renderer *r, float *delta_ms) {
    if (!r) return fail(DRT_ERR_INVALID, "null renderer");
    if (delta_ms) *delta_ms = 0.f;
    if (!r->pending) return DRT_OK;
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipEventSynchronize(r->ev_stop));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, r->ev_start, r->ev_stop));
    if (delta_ms) *delta_ms = ms;
    r->span_ms = 0.f;
    unsigned int status = 0;
    if (r->spans_used > 0) {
        const unsigned long long *host = r->records_host.ptr;          // (copied on the stream before ev_stop)
        double ticks = 0;
        for (int i = 0; i < r->spans_used; i++) {
            const unsigned long long start = ~host[4 * i], end = host[4 * i + 1];
            if (host[4 * i] != 0 && end > start) ticks += (double)(end - start);
            status |= (unsigned int)host[4 * i + 2];
        }
        r->span_ms = (float)(ticks / (double)r->wall_clock_khz);
    }
    wave_queue_report(r->wq_cache, r->span_ms);
    r->pending = false;
    if (r->choice.family == Tracer::path_pool && status != 0)
        return fail(DRT_ERR_DEVICE, "path_pool kernel: status " + std::to_string(status) + (status < 0x100u ? " (a queue wait exceeded its bound; the launch was abandoned)"
                                                                                             : " (bits 8..: an index out of range was caught and clamped -- 0x100 triangle, 0x200 node, 0x400 leaf, "
                                                                                               "0x800 / 0x1000 hit triangle, 0x2000 material, 0x4000 texture, 0x8000 sample slot, 0x10000 / 0x20000 stack level, "
                                                                                               "0x40000 path id from a queue, 0x80000 shading record)"));
    return DRT_OK;
}

// ------------------------------------------------------------------ batched ray queries (kernel_ray_query.hip)
static int ray_query_impl(drt_renderer *r, const drt_scene *scene, const drt_ray *rays, void *out, uint32_t n, void *hip_stream,
                          bool occluded) {
    static const QueryWords words = {"null ray or result pointer", "rays and hits must be 16-byte aligned", "rays", "rays and results"};
    hipStream_t s;
    int rc;
    if (!query_begin(r, scene, n, {{rays, 16}, {out, occluded ? 1u : 16u}}, words, hip_stream, occluded, &s, &rc)) return rc;
    RayQueryArgs a;
    a.rays = rays; a.out = out; a.frame = query_frame(r, n);
    const char *name = nullptr;                // (kernel_info names the last render kernel: queries leave it alone)
    HIP_TRY(launch_ray_query(r->view, occluded, a, r->num_cus, s, &name));
    return query_recorded(r, s);
}

int drt_renderer_trace_rays(drt_renderer *r, const drt_scene *scene, const drt_ray *rays, drt_hit *hits, uint32_t n, void *hip_stream) {
    return ray_query_impl(r, scene, rays, hits, n, hip_stream, false);
}

int drt_renderer_occluded(drt_renderer *r, const drt_scene *scene, const drt_ray *rays, uint8_t *occluded, uint32_t n, void *hip_stream) {
    return ray_query_impl(r, scene, rays, occluded, n, hip_stream, true);
}

// ------------------------------------------------------------------ nearest-surface queries (kernel_nearest.hip)
// The closest-hit HBM stack ({ref, box2} entries).
int drt_renderer_nearest(drt_renderer *r, const drt_scene *scene, const drt_point *points, drt_nearest *out, uint32_t n, void *hip_stream) {
    static const QueryWords words = {"null point or result pointer", "points and results must be 16-byte aligned", "points", "points and results"};
    hipStream_t s;
    int rc;
    if (!query_begin(r, scene, n, {{points, 16}, {out, 16}}, words, hip_stream, false, &s, &rc)) return rc;
    NearestArgs a;
    a.points = points; a.out = out; a.frame = query_frame(r, n);
    HIP_TRY(launch_nearest(r->view, a, r->num_cus, s));
    return query_recorded(r, s);
}

// ------------------------------------------------------------------ sphere casts (kernel_sphere_cast.hip)
// The closest-hit HBM stack ({ref, enter} entries).
int drt_renderer_sphere_cast(drt_renderer *r, const drt_scene *scene, const drt_ray *rays, const float *radii, drt_sweep_hit *out, uint32_t n,
                             void *hip_stream) {
    static const QueryWords words = {"null ray, radius or result pointer", "rays and results must be 16-byte aligned, radii 4-byte aligned", "casts",
                                     "rays, radii and results"};
    hipStream_t s;
    int rc;
    if (!query_begin(r, scene, n, {{rays, 16}, {radii, 4}, {out, 16}}, words, hip_stream, false, &s, &rc)) return rc;
    SphereCastArgs a;
    a.rays = rays; a.radii = radii; a.out = out; a.frame = query_frame(r, n);
    HIP_TRY(launch_sphere_cast(r->view, a, r->num_cus, s));
    return query_recorded(r, s);
}

// ------------------------------------------------------------------ crossing counts, inside votes, signed distance (kernel_crossings.hip)
// The occlusion query's HBM stack (ref entries).
static int bad_rule(int32_t rule) {
    return fail(DRT_ERR_INVALID, "rule " + std::to_string(rule) + ": 0 (parity) or 1 (winding) expected");
}

// in: rays or points (16-byte aligned); out: what `kind` says, aligned to out_align bytes
static int crossings_impl(drt_renderer *r, const drt_scene *scene, const void *in, void *out, size_t out_align, uint32_t n, int32_t rule,
                          void *hip_stream, drt::CrossingsOut kind) {
    if (!r || !scene) return fail(DRT_ERR_INVALID, "null argument");
    if (n == 0) return DRT_OK;
    if (!in || !out) return fail(DRT_ERR_INVALID, "null query or result pointer");
    if (((uintptr_t)in & 15u) != 0 || ((uintptr_t)out & (out_align - 1)) != 0)
        return fail(DRT_ERR_INVALID, "queries must be 16-byte aligned, results " + std::to_string(out_align) + "-byte aligned");
    hipStream_t s;
    if (int rc = query_open(r, scene, n, {in, out}, "queries", "queries and results", hip_stream, true, &s)) return rc;
    CrossingsArgs a;
    a.in = in; a.out = out; a.frame = query_frame(r, n);
    a.rule = (uint32_t)rule;
    HIP_TRY(launch_crossings(r->view, kind, a, r->num_cus, s));
    return query_recorded(r, s);
}

int drt_renderer_crossings(drt_renderer *r, const drt_scene *scene, const drt_ray *rays, drt_crossings *out, uint32_t n, void *hip_stream) {
    return crossings_impl(r, scene, rays, out, 8, n, 0, hip_stream, drt::CrossingsOut::crossings);
}

int drt_renderer_inside(drt_renderer *r, const drt_scene *scene, const drt_point *points, uint8_t *votes, uint32_t n, int32_t rule, void *hip_stream) {
    if (rule != 0 && rule != 1) return bad_rule(rule);
    return crossings_impl(r, scene, points, votes, 1, n, rule, hip_stream, drt::CrossingsOut::votes);
}

// The nearest kernel writes the records, then the point-mode kernel replaces their `side` words: two launches on one stream.
int drt_renderer_signed_distance(drt_renderer *r, const drt_scene *scene, const drt_point *points, drt_nearest *out, uint32_t n, int32_t rule,
                                 void *hip_stream) {
    if (rule != 0 && rule != 1) return bad_rule(rule);
    if (int rc = drt_renderer_nearest(r, scene, points, out, n, hip_stream)) return rc;
    return crossings_impl(r, scene, points, out, 16, n, rule, hip_stream, drt::CrossingsOut::side);
}

// ------------------------------------------------------------------ ordered hit lists of rays (kernel_list_hits.hip)
// The occlusion query's HBM stack (ref entries).  counts may be null; hits may be null iff hits_capacity == 0 (a pure count); not both.
int drt_renderer_list_hits(drt_renderer *r, const drt_scene *scene, const drt_ray *rays, const uint32_t *offsets, drt_hit *hits,
                           uint32_t hits_capacity, uint32_t *counts, uint32_t n, void *hip_stream) {
    if (!r || !scene) return fail(DRT_ERR_INVALID, "null argument");
    if (n == 0) return DRT_OK;
    if (!rays || !offsets) return fail(DRT_ERR_INVALID, "null ray or offset pointer");
    if (!hits && !counts) return fail(DRT_ERR_INVALID, "hits and counts are both null: nothing to write");
    if ((hits == nullptr) != (hits_capacity == 0)) return fail(DRT_ERR_INVALID, "hits must be null if and only if hits_capacity is 0");
    if (((uintptr_t)rays & 15u) != 0 || ((uintptr_t)hits & 15u) != 0 || ((uintptr_t)offsets & 3u) != 0 || ((uintptr_t)counts & 3u) != 0)
        return fail(DRT_ERR_INVALID, "rays and hits must be 16-byte aligned, offsets and counts 4-byte aligned");
    hipStream_t s;
    if (int rc = query_open(r, scene, n, {rays, offsets, hits, counts}, "rays", "rays, offsets, hits and counts", hip_stream, true, &s)) return rc;
    ListHitsArgs a;
    a.rays = rays; a.offsets = offsets; a.hits = hits; a.counts = counts;
    a.hits_capacity = hits_capacity; a.frame = query_frame(r, n);
    HIP_TRY(launch_list_hits(r->view, a, r->num_cus, s));
    return query_recorded(r, s);
}

// ------------------------------------------------------------------ nearest-triangle lists of points (kernel_near_list.hip)
// drt_renderer_list_hits' checks in its order with the mode first after the handles; the closest-hit HBM stack ({ref, box2} entries).
// counts and surf may be null; near may be null iff near_capacity == 0 (a pure count); near and counts not both.
int drt_renderer_nearest_list(drt_renderer *r, const drt_scene *scene, const drt_point *points, const uint32_t *offsets, drt_near *near,
                              drt_near_surf *surf, uint32_t near_capacity, uint32_t *counts, uint32_t n, int32_t mode, void *hip_stream) {
    if (!r || !scene) return fail(DRT_ERR_INVALID, "null argument");
    if (mode != DRT_NEAR_GATHER && mode != DRT_NEAR_K)
        return fail(DRT_ERR_INVALID, "mode " + std::to_string(mode) + ": 0 (gather) or 1 (k-nearest) expected");
    if (n == 0) return DRT_OK;
    if (!points || !offsets) return fail(DRT_ERR_INVALID, "null point or offset pointer");
    if (!near && !counts) return fail(DRT_ERR_INVALID, "near and counts are both null: nothing to write");
    if ((near == nullptr) != (near_capacity == 0)) return fail(DRT_ERR_INVALID, "near must be null if and only if near_capacity is 0");
    if (((uintptr_t)points & 15u) != 0 || ((uintptr_t)near & 15u) != 0 || ((uintptr_t)surf & 15u) != 0 || ((uintptr_t)offsets & 3u) != 0 ||
        ((uintptr_t)counts & 3u) != 0)
        return fail(DRT_ERR_INVALID, "points, near and surf must be 16-byte aligned, offsets and counts 4-byte aligned");
    hipStream_t s;
    if (int rc = query_open(r, scene, n, {points, offsets, near, surf, counts}, "points", "points, offsets, near, surf and counts", hip_stream, false, &s))
        return rc;
    NearListArgs a;
    a.points = points; a.offsets = offsets; a.near = near; a.surf = near_capacity ? surf : nullptr; a.counts = counts;
    a.near_capacity = near_capacity; a.frame = query_frame(r, n);
    HIP_TRY(launch_near_list(r->view, mode == DRT_NEAR_K, a, r->num_cus, s));
    return query_recorded(r, s);
}

// ------------------------------------------------------------------ box overlap queries (kernel_overlap.hip)
// drt_renderer_nearest_list's checks in its order with the mode first after the handles; the occlusion query's HBM stack (ref entries).
// Mode LIST: counts may be null, prims may be null iff prims_capacity == 0 (a pure count), not both.  Mode ANY: no prims, no
// capacity, offsets is not read.
int drt_renderer_overlap_boxes(drt_renderer *r, const drt_scene *scene, const drt_box *boxes, const uint32_t *offsets, int32_t *prims,
                               uint32_t prims_capacity, uint32_t *counts, uint32_t n, int32_t mode, void *hip_stream) {
    if (!r || !scene) return fail(DRT_ERR_INVALID, "null argument");
    if (mode != DRT_OVERLAP_LIST && mode != DRT_OVERLAP_ANY)
        return fail(DRT_ERR_INVALID, "mode " + std::to_string(mode) + ": 0 (list) or 1 (any) expected");
    if (n == 0) return DRT_OK;
    const bool any = mode == DRT_OVERLAP_ANY;
    if (!boxes || (!any && !offsets)) return fail(DRT_ERR_INVALID, "null box or offset pointer");
    if (any) {
        if (prims || prims_capacity != 0) return fail(DRT_ERR_INVALID, "mode any writes no list: prims must be null and prims_capacity 0");
        if (!counts) return fail(DRT_ERR_INVALID, "mode any: counts is null: nothing to write");
        offsets = nullptr;                     // (not read)
    } else {
        if (!prims && !counts) return fail(DRT_ERR_INVALID, "prims and counts are both null: nothing to write");
        if ((prims == nullptr) != (prims_capacity == 0)) return fail(DRT_ERR_INVALID, "prims must be null if and only if prims_capacity is 0");
    }
    if (((uintptr_t)boxes & 15u) != 0 || ((uintptr_t)prims & 3u) != 0 || ((uintptr_t)offsets & 3u) != 0 || ((uintptr_t)counts & 3u) != 0)
        return fail(DRT_ERR_INVALID, "boxes must be 16-byte aligned, offsets, prims and counts 4-byte aligned");
    hipStream_t s;
    if (int rc = query_open(r, scene, n, {boxes, offsets, prims, counts}, "boxes", "boxes, offsets, prims and counts", hip_stream, true, &s))
        return rc;
    OverlapArgs a;
    a.boxes = boxes; a.offsets = offsets; a.prims = prims; a.counts = counts;
    a.prims_capacity = prims_capacity; a.frame = query_frame(r, n);
    HIP_TRY(launch_overlap(r->view, any, a, r->num_cus, s));
    return query_recorded(r, s);
}

// ------------------------------------------------------------------ triangle overlap queries (kernel_tri_overlap.hip)
// drt_renderer_overlap_boxes' checks in its order, word for word; the occlusion query's HBM stack (ref entries).
int drt_renderer_overlap_triangles(drt_renderer *r, const drt_scene *scene, const drt_tri *tris, const uint32_t *offsets, int32_t *prims,
                                   uint32_t prims_capacity, uint32_t *counts, uint32_t n, int32_t mode, void *hip_stream) {
    if (!r || !scene) return fail(DRT_ERR_INVALID, "null argument");
    if (mode != DRT_OVERLAP_LIST && mode != DRT_OVERLAP_ANY)
        return fail(DRT_ERR_INVALID, "mode " + std::to_string(mode) + ": 0 (list) or 1 (any) expected");
    if (n == 0) return DRT_OK;
    const bool any = mode == DRT_OVERLAP_ANY;
    if (!tris || (!any && !offsets)) return fail(DRT_ERR_INVALID, "null triangle or offset pointer");
    if (any) {
        if (prims || prims_capacity != 0) return fail(DRT_ERR_INVALID, "mode any writes no list: prims must be null and prims_capacity 0");
        if (!counts) return fail(DRT_ERR_INVALID, "mode any: counts is null: nothing to write");
        offsets = nullptr;                     // (not read)
    } else {
        if (!prims && !counts) return fail(DRT_ERR_INVALID, "prims and counts are both null: nothing to write");
        if ((prims == nullptr) != (prims_capacity == 0)) return fail(DRT_ERR_INVALID, "prims must be null if and only if prims_capacity is 0");
    }
    if (((uintptr_t)tris & 15u) != 0 || ((uintptr_t)prims & 3u) != 0 || ((uintptr_t)offsets & 3u) != 0 || ((uintptr_t)counts & 3u) != 0)
        return fail(DRT_ERR_INVALID, "tris must be 16-byte aligned, offsets, prims and counts 4-byte aligned");
    hipStream_t s;
    if (int rc = query_open(r, scene, n, {tris, offsets, prims, counts}, "triangles", "tris, offsets, prims and counts", hip_stream, true, &s))
        return rc;
    TriOverlapArgs a;
    a.tris = tris; a.offsets = offsets; a.prims = prims; a.counts = counts;
    a.prims_capacity = prims_capacity; a.frame = query_frame(r, n);
    HIP_TRY(launch_tri_overlap(r->view, any, a, r->num_cus, s));
    return query_recorded(r, s);
}

// ------------------------------------------------------------------ camera rays and radiance queries (kernel_radiance.hip)
// Both share the ray queries' claim heads and HBM stack: they wait for the last query / guide pass of this renderer on another stream,
// and record the event the next one waits for.
int drt_renderer_camera_rays(drt_renderer *r, const drt_camera *cams, uint32_t n_cams, uint32_t width, uint32_t height,
                             uint32_t frame_index, drt_path_ray *rays, void *hip_stream) {
    if (!r || !cams || !rays) return fail(DRT_ERR_INVALID, "null argument");
    if (frame_index == 0) return fail(DRT_ERR_INVALID, "frame indices start at 1");
    if (n_cams == 0 || width == 0 || height == 0) return fail(DRT_ERR_INVALID, "zero cameras, width or height");
    if ((uint64_t)n_cams * width * height > 0x7fffffffull) return fail(DRT_ERR_INVALID, "at most 2^31 - 1 rays per call");
    if (((uintptr_t)rays & 15u) != 0) return fail(DRT_ERR_INVALID, "rays must be 16-byte aligned");
    if (r->pending) return fail(DRT_ERR_INVALID, "an asynchronous render batch is pending: drt_renderer_wait first");
    HIP_TRY(hipSetDevice(r->device));
    (void)hipGetLastError();                   // (see render_batch_impl: only this call's own errors count)
    if (!on_renderer_device(r, rays)) return fail(DRT_ERR_INVALID, "rays must be device memory on the renderer's device");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : r->stream;
    if (int rc = query_order(r, s)) return rc;
    const size_t per_cam = (size_t)width * height;
    for (uint32_t c0 = 0; c0 < n_cams; c0 += kCamsPerLaunch) {     // (one launch up to kCamsPerLaunch cameras)
        CameraRaysArgs a;
        a.n_cams = std::min<uint32_t>(kCamsPerLaunch, n_cams - c0);
        a.rays = rays + c0 * per_cam;
        a.width = width; a.height = height; a.frame = frame_index;
        for (uint32_t c = 0; c < a.n_cams; c++) a.cams[c] = camera_const(&cams[c0 + c], (float)width, (float)height);
        HIP_TRY(launch_camera_rays(a, s));
    }
    return query_recorded(r, s);
}

int drt_renderer_radiance(drt_renderer *r, const drt_scene *scene, const drt_path_ray *rays, float *out, uint32_t n, int32_t accumulate,
                          void *hip_stream) {
    if (!r || !scene) return fail(DRT_ERR_INVALID, "null argument");
    if (n == 0) return DRT_OK;
    if (!rays || !out) return fail(DRT_ERR_INVALID, "null ray or result pointer");
    if (((uintptr_t)rays & 15u) != 0 || ((uintptr_t)out & 15u) != 0) return fail(DRT_ERR_INVALID, "rays and results must be 16-byte aligned");
    if (n > 0x7fffffffu) return fail(DRT_ERR_INVALID, "at most 2^31 - 1 rays per call");
    if (r->pending) return fail(DRT_ERR_INVALID, "an asynchronous render batch is pending: drt_renderer_wait first");
    if (r->settings.render_mode == 1) return fail(DRT_ERR_UNSUPPORTED, "debug views are the framebuffer's: radiance needs render_mode 0");
    HIP_TRY(hipSetDevice(r->device));
    (void)hipGetLastError();                   // (see render_batch_impl: only this call's own errors count)
    if (!on_renderer_device(r, rays) || !on_renderer_device(r, out))
        return fail(DRT_ERR_INVALID, "rays and results must be device memory on the renderer's device");
    if (int rc = upload_scene(r, scene)) return rc;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : r->stream;
    if (int rc = query_order(r, s)) return rc;
    if (int rc = traversal_scratch(r, s, false, true)) return rc;
    FrameParams fp;
    std::memset(&fp, 0, sizeof fp);
    fill_frame_params(r, nullptr, fp);
    RadianceArgs a;
    a.rays = rays; a.out = reinterpret_cast<float4 *>(out); a.frame = query_frame(r, n);
    a.accumulate = accumulate != 0;
    HIP_TRY(launch_radiance(r->view, fp, r->scene_has_alpha, a, r->num_cus, s));
    return query_recorded(r, s);
}

// ------------------------------------------------------------------ refit of the device copy (kernel_refit.hip)
// The metadata of the uploaded scene: load order, stored normals' averages, the leaves and the interior nodes by height, every
// node's destination box in pack()'s numbering of the records.
static RefitPlan refit_plan(const HostScene &h) {
    RefitPlan p;
    const size_t n_nodes = h.nodes.size();
    p.n_nodes = (uint32_t)n_nodes;
    p.order = h.load_index;
    p.avg_normal.resize(h.triangles.size());
    for (size_t k = 0; k < h.triangles.size(); k++) {
        const drt_vertex *v = h.triangles[k].vertex;
        const V3 avg = (V3{ v[0].normal[0], v[0].normal[1], v[0].normal[2] } + V3{ v[1].normal[0], v[1].normal[1], v[1].normal[2] } +
                        V3{ v[2].normal[0], v[2].normal[1], v[2].normal[2] }) / 3;        // make_triangle (Scene.cu:279)
        p.avg_normal[k] = make_float4(avg.x, avg.y, avg.z, 0.f);
    }
    std::vector<uint32_t> rec(n_nodes, 0), dest(n_nodes, kRefitRootDest);
    uint32_t n_inner = 0;
    for (size_t i = 0; i < n_nodes; i++)
        if (!h.nodes[i].is_leaf) rec[i] = n_inner++;
    for (size_t i = 0; i < n_nodes; i++) {
        const drt_bvh_node &nd = h.nodes[i];
        if (nd.is_leaf) continue;
        dest[(size_t)nd.child1] = rec[i] << 1;
        dest[(size_t)nd.child2] = rec[i] << 1 | 1u;
    }
    std::vector<int32_t> pre, todo{ (int32_t)n_nodes - 1 }, height(n_nodes, 0);
    pre.reserve(n_nodes);
    while (!todo.empty()) {
        const int32_t i = todo.back();
        todo.pop_back();
        pre.push_back(i);
        const drt_bvh_node &nd = h.nodes[(size_t)i];
        if (!nd.is_leaf) { todo.push_back(nd.child1); todo.push_back(nd.child2); }
    }
    int32_t heights = 0;
    for (size_t j = pre.size(); j-- > 0;) {            // children before their parent
        const int32_t i = pre[j];
        const drt_bvh_node &nd = h.nodes[(size_t)i];
        if (nd.is_leaf) {
            p.leaves.push_back(RefitLeaf{ nd.prim_start, nd.prim_count, i, dest[(size_t)i] });
        } else {
            height[(size_t)i] = 1 + std::max(height[(size_t)nd.child1], height[(size_t)nd.child2]);
            heights = std::max(heights, height[(size_t)i]);
        }
    }
    p.height_begin.assign((size_t)heights + 1, 0);
    for (int32_t i : pre)
        if (height[(size_t)i] > 0) p.height_begin[(size_t)height[(size_t)i]]++;
    for (int32_t hh = 1; hh <= heights; hh++) p.height_begin[(size_t)hh] += p.height_begin[(size_t)hh - 1];
    std::vector<uint32_t> fill(p.height_begin.begin(), p.height_begin.end());
    p.inner.resize(n_inner);
    for (size_t i = 0; i < n_nodes; i++) {
        const drt_bvh_node &nd = h.nodes[i];
        if (!nd.is_leaf) p.inner[fill[(size_t)height[i] - 1]++] = RefitInner{ nd.child1, nd.child2, (int32_t)i, dest[i] };
    }
    return p;
}

}  // extern "C"

// The uploaded scene's plan on the device, made once per upload: the first refit needs it, and so does the first winding call.
int drt::refit_metadata(drt_renderer *r, const drt_scene *scene) {
    if (r->rf_built) return DRT_OK;
    RefitPlan plan;
    try { plan = refit_plan(scene->host); } catch (...) { return from_exception(); }
    HIP_TRY(r->rf_order.upload(plan.order));
    HIP_TRY(r->rf_avg.upload(plan.avg_normal));
    HIP_TRY(r->rf_ext.upload(std::vector<float>(6 * (size_t)plan.n_nodes, 0.f)));
    HIP_TRY(r->rf_leaves.upload(plan.leaves));
    HIP_TRY(r->rf_levels.upload(plan.inner));
    HIP_TRY(r->rf_height_begin.upload(plan.height_begin));
    HIP_TRY(r->rf_out.upload(std::vector<float>(8, 0.f)));
    r->rf_heights = plan.height_begin;
    r->rf_built = true;
    return DRT_OK;
}

extern "C" {

// device memory of the renderer's device that holds `bytes` bytes from p on (as far as the runtime can tell)
static bool device_range_on_renderer(const drt_renderer *r, const void *p, size_t bytes) {
    if (((uintptr_t)p & 3u) != 0 || !on_renderer_device(r, p)) return false;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return true; }
    return (const char *)p >= (const char *)base && bytes <= size - (size_t)((const char *)p - (const char *)base);
}

int drt_renderer_refit(drt_renderer *r, const drt_scene *scene, const float *positions, const float *normals, float *delta_ms,
                       void *hip_stream) {
    if (delta_ms) *delta_ms = 0.f;
    if (!r || !scene || !positions) return fail(DRT_ERR_INVALID, "null argument");
    if (r->pending) return fail(DRT_ERR_INVALID, "an asynchronous render batch is pending: drt_renderer_wait first");
    if (scene->host.nodes.empty()) return fail(DRT_ERR_INVALID, "scene has no BVH: refit keeps a tree, build one first");
    HIP_TRY(hipSetDevice(r->device));
    (void)hipGetLastError();
    const size_t bytes = 9 * sizeof(float) * scene->host.triangles.size();
    for (const float *p : { positions, normals })
        if (p && !device_range_on_renderer(r, p, bytes))
            return fail(DRT_ERR_INVALID, "positions and normals must be float[n][3][3] in device memory on the renderer's device");
    if (int rc = upload_scene(r, scene)) return rc;
    if (int rc = refit_metadata(r, scene)) return rc;
    r->wn_valid = false;                         // the winding moments are those of the positions that go
    HIP_TRY(r->ev_rf_start.create());
    HIP_TRY(r->ev_rf_stop.create());
    HIP_TRY(r->ev_rf_dep.create(hipEventDisableTiming));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : r->stream;
    // nothing is written before the renderer's queries / guide passes in flight and the work on its stream are done
    if (int rc = query_order(r, s)) return rc;
    if (s != r->stream) {
        HIP_TRY(hipEventRecord(r->ev_rf_dep, r->stream));
        HIP_TRY(hipStreamWaitEvent(s, r->ev_rf_dep, 0));
    }
    const bool take_snapshot = r->mv_track && !r->mv_armed && r->d_hot.count;      // the oldest state since the last temporal call / motion_advance is kept
    if (take_snapshot && r->mv_snap.count != r->d_hot.count) HIP_TRY(r->mv_snap.alloc(r->d_hot.count));       // (host time: not in *delta_ms)
    HIP_TRY(hipEventRecord(r->ev_rf_start, s));
    if (take_snapshot) {
        HIP_TRY(hipMemcpyAsync(r->mv_snap.ptr, r->d_hot.ptr, r->d_hot.count * sizeof(TriHot), hipMemcpyDeviceToDevice, s));
        r->mv_armed = true;
    }
    HIP_TRY(hipMemsetAsync(r->rf_out.ptr + 6, 0, sizeof(unsigned int), s));
    RefitArgs a;
    a.pos = positions; a.nrm = normals;
    a.order = r->rf_order.ptr; a.avg_normal = r->rf_avg.ptr;
    a.hot = r->d_hot.ptr; a.inner = r->d_inner.ptr; a.ext = r->rf_ext.ptr;
    a.leaves = r->rf_leaves.ptr; a.n_leaves = (uint32_t)r->rf_leaves.count;
    a.levels = r->rf_levels.ptr; a.height_begin = r->rf_height_begin.ptr;
    a.root_box = r->rf_out.ptr; a.error = reinterpret_cast<unsigned int *>(r->rf_out.ptr + 6);
    r->pool_safe_dir = 0.0f;                     // the edges are rewritten on the device: path_pool keeps its guarded T loop until the scene is uploaded again
    HIP_TRY(launch_refit(a, r->rf_heights, r->rf_top_nodes, s, &r->rf_launches));
    HIP_TRY(hipEventRecord(r->ev_rf_stop, s));
    float out[8];
    HIP_TRY(hipMemcpyAsync(out, r->rf_out.ptr, sizeof out, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    unsigned int err;
    std::memcpy(&err, out + 6, 4);
    if (err) {
        r->uploaded_scene = nullptr;             // the copy is half written: the next use uploads the host state again
        r->mv_armed = false;                     // ... and with it goes the snapshot
        return fail(DRT_ERR_INVALID, "non-finite coordinate in refit input");
    }
    std::memcpy(r->view.root_min, out, 12);
    std::memcpy(r->view.root_max, out + 3, 12);
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, r->ev_rf_start, r->ev_rf_stop));
    if (delta_ms) *delta_ms = ms;
    return DRT_OK;
}

int drt_debug_pack_scene(const drt_scene *s, void *inner, size_t inner_bytes, void *tri_hot, size_t hot_bytes, float root_box[6]) {
    if (!s) return fail(DRT_ERR_INVALID, "null scene");
    PackedScene ps;
    try { ps = s->host.pack(); } catch (...) { return from_exception(); }
    if ((inner && inner_bytes < ps.inner.size() * sizeof(InnerNode)) || (tri_hot && hot_bytes < ps.tri_hot.size() * sizeof(TriHot)))
        return fail(DRT_ERR_INVALID, "destination too small");
    if (inner && !ps.inner.empty()) std::memcpy(inner, ps.inner.data(), ps.inner.size() * sizeof(InnerNode));
    if (tri_hot && !ps.tri_hot.empty()) std::memcpy(tri_hot, ps.tri_hot.data(), ps.tri_hot.size() * sizeof(TriHot));
    if (root_box) { std::memcpy(root_box, ps.root_min, 12); std::memcpy(root_box + 3, ps.root_max, 12); }
    return DRT_OK;
}

int drt_debug_read_device_scene(drt_renderer *r, void *inner, size_t inner_bytes, void *tri_hot, size_t hot_bytes, float root_box[6]) {
    if (!r) return fail(DRT_ERR_INVALID, "null renderer");
    if (!r->uploaded_scene) return fail(DRT_ERR_INVALID, "the renderer holds no scene");
    if ((inner && inner_bytes < r->d_inner.count * sizeof(InnerNode)) || (tri_hot && hot_bytes < r->d_hot.count * sizeof(TriHot)))
        return fail(DRT_ERR_INVALID, "destination too small");
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipDeviceSynchronize());
    if (inner && r->d_inner.count) HIP_TRY(hipMemcpy(inner, r->d_inner.ptr, r->d_inner.count * sizeof(InnerNode), hipMemcpyDeviceToHost));
    if (tri_hot && r->d_hot.count) HIP_TRY(hipMemcpy(tri_hot, r->d_hot.ptr, r->d_hot.count * sizeof(TriHot), hipMemcpyDeviceToHost));
    if (root_box) { std::memcpy(root_box, r->view.root_min, 12); std::memcpy(root_box + 3, r->view.root_max, 12); }
    return DRT_OK;
}

int drt_renderer_render(drt_renderer *r, const drt_camera *cam, const drt_scene *scene, float *delta_ms) {
    return drt_renderer_render_batch(r, cam, scene, 1, delta_ms);
}

int drt_renderer_read_rgba32f(drt_renderer *r, float *dst, size_t dst_floats) {
    return read_back(r, r ? r->cur_rgba() : nullptr, 4, dst, dst_floats);
}
int drt_renderer_read_accum(drt_renderer *r, float *dst, size_t dst_floats) {
    return read_back(r, r ? r->cur_accum() : nullptr, 3, dst, dst_floats);
}

static int debug_check_exact(int32_t device, int which, uint64_t *mismatches, uint64_t *fast_path_count) {
    if (!mismatches || !fast_path_count) return fail(DRT_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(device));
    DeviceArray<unsigned long long> d;
    HIP_TRY(d.alloc_zeroed(2));
    HIP_TRY(launch_check_rcp(which, 0u, 1ull << 32, d.ptr, nullptr));
    unsigned long long h[2] = { 0, 0 };
    HIP_TRY(hipMemcpy(h, d.ptr, sizeof h, hipMemcpyDeviceToHost));
    *mismatches = h[0]; *fast_path_count = h[1];
    return DRT_OK;
}

int drt_debug_check_rcp(int32_t device, uint64_t *mismatches, uint64_t *fast_path_count) {
    return debug_check_exact(device, 0, mismatches, fast_path_count);
}
int drt_debug_check_sqrt(int32_t device, uint64_t *mismatches, uint64_t *fast_path_count) {
    return debug_check_exact(device, 1, mismatches, fast_path_count);
}

int drt_debug_decode_image(const uint8_t *file, size_t file_bytes, drt_texture_info *info, uint8_t *out, size_t cap) {
    if (!file || !info) return fail(DRT_ERR_INVALID, "null argument");
    try {
        DecodedImage img;
        if (looks_like_png(file, file_bytes)) img = decode_png(file, file_bytes);
        else if (looks_like_jpeg(file, file_bytes)) img = decode_jpeg(file, file_bytes);
        else return fail(DRT_ERR_UNSUPPORTED, "neither PNG nor JPEG");
        info->width = img.width; info->height = img.height; info->components = img.components;
        if (out) {
            if (cap < img.texels.size()) return fail(DRT_ERR_INVALID, "destination too small");
            std::memcpy(out, img.texels.data(), img.texels.size());
        }
    } catch (...) { return from_exception(); }
    return DRT_OK;
}

int drt_debug_kat(int32_t device, int32_t which, const void *in, size_t in_bytes, void *out, size_t out_bytes, uint32_t n,
                  const drt_camera *cam, uint32_t width, uint32_t height) {
    if (!in || !out || which < 0 || which > 8) return fail(DRT_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(device));
    FrameParams fp;
    std::memset(&fp, 0, sizeof fp);
    if (which == 4) {
        if (!cam || width == 0 || height == 0) return fail(DRT_ERR_INVALID, "camera KAT needs a camera and a frame size");
        drt_renderer tmp;
        tmp.device = device;
        drt_default_settings(&tmp.settings);
        tmp.width = width; tmp.height = height;
        fill_frame_params(&tmp, cam, fp);
    }
    DeviceArray<uint8_t> d_in, d_out;
    HIP_TRY(d_in.alloc(std::max<size_t>(in_bytes, 16)));
    HIP_TRY(d_out.alloc(std::max<size_t>(out_bytes, 16)));
    HIP_TRY(hipMemcpy(d_in.ptr, in, in_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_out.ptr, 0, out_bytes));
    HIP_TRY(launch_kat(which, d_in.ptr, d_out.ptr, n, fp, nullptr));
    HIP_TRY(hipMemcpy(out, d_out.ptr, out_bytes, hipMemcpyDeviceToHost));
    return DRT_OK;
}

int drt_debug_wave_queue_plans(const drt_renderer *r, char *buf, size_t cap) {
    if (!r || !buf || cap == 0) return fail(DRT_ERR_INVALID, "bad argument");
    std::string out = "[";
    for (const WqPlan &p : r->wq_cache.plans) {
        if (out.size() > 1) out += ", ";
        out += "{\"key\": " + std::to_string(p.key) + ", \"chosen\": " + std::to_string(p.chosen) + ", \"candidates\": [";
        for (size_t i = 0; i < p.cands.size(); i++) {
            char item[200];
            std::snprintf(item, sizeof item, "%s{\"threads\": %d, \"entry_bytes\": %d, \"tris\": %d, \"wg_per_cu\": %d, \"trials\": %d, \"ns_per_sample\": %.6f}",
                          i ? ", " : "", p.cands[i].threads, p.cands[i].entry_bytes, p.cands[i].tris, p.cands[i].per_cu, p.trials[i], p.ns_per_sample[i]);
            out += item;
        }
        out += "]}";
    }
    out += "]";
    if (out.size() + 1 > cap) return fail(DRT_ERR_INVALID, "destination too small");
    std::memcpy(buf, out.c_str(), out.size() + 1);
    return DRT_OK;
}

// (path_pool's statistics builds only: launches of the material-model builds gather no statistics)
int drt_debug_pool_stats(drt_renderer *r, uint64_t out[40], int32_t reset) {
    if (!r || !out) return fail(DRT_ERR_INVALID, "null argument");
    if (!r->tune.stats) return fail(DRT_ERR_INVALID, "renderer was not created with DRT_POOL_STATS=1");
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipStreamSynchronize(r->stream));
    HIP_TRY(hipMemcpy(out, r->tune.stats, 40 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset(r->tune.stats, 0, 40 * sizeof(uint64_t)));
    return DRT_OK;
}

int drt_debug_hash_cycles(int32_t device, uint32_t max_len, uint32_t *pairs_out, uint32_t cap_pairs, uint32_t *found) {
    if (!pairs_out || !found || cap_pairs == 0) return fail(DRT_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(device));
    DeviceArray<uint32_t> d;
    HIP_TRY(d.alloc_zeroed(1 + 2 * (size_t)cap_pairs));
    HIP_TRY(launch_hash_cycles(max_len, d.ptr, cap_pairs, nullptr));
    std::vector<uint32_t> h(d.count);
    HIP_TRY(hipMemcpy(h.data(), d.ptr, d.bytes(), hipMemcpyDeviceToHost));
    *found = h[0];
    std::memcpy(pairs_out, h.data() + 1, 2 * (size_t)std::min<uint32_t>(h[0], cap_pairs) * sizeof(uint32_t));
    return DRT_OK;
}

int drt_assemble_shards(const void *gathered, void *image, uint32_t width, uint32_t height, uint32_t stripe_rows,
                        uint32_t world, uint32_t padded_rows, void *hip_stream) {
    if (!gathered || !image || stripe_rows == 0 || world == 0) return fail(DRT_ERR_INVALID, "bad argument");
    if (padded_rows < drt_shard_rows(height, stripe_rows, 0, world)) return fail(DRT_ERR_INVALID, "padded_rows smaller than rank 0's shard");
    (void)hipGetLastError();                 // (see render_batch_impl: only this launch's own error counts)
    HIP_TRY(launch_assemble(gathered, image, width, height, stripe_rows, world, padded_rows, (hipStream_t)hip_stream));
    return DRT_OK;
}

}  // extern "C"
