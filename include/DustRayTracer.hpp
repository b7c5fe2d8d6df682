// DustRayTracer.hpp -- the reference's "intended library header" (DustRayTracer/include/DustRayTracer.hpp:1 is empty)
// filled in for the MI355X core: thin C++ classes with the reference's names and members over the C ABI of drt.h.
//
//   Renderer        Core/Renderer.hpp:14-47          ResizeBuffer / Render / resetAccumulationBuffer / getSampleCount /
//                                                    getBufferWidth / getBufferHeight / public m_RendererSettings
//   Scene           Core/Scene/Scene.cuh:41-57       loadGLTFmodel (+ counts the editor shows, EditorLayer.cpp:57-65)
//   BVHBuilder      Core/BVH/BVHBuilder.cuh:12-23    m_BinCount, m_TargetLeafPrimitivesCount, buildIterative, build
//   Camera          Core/Scene/Camera.cuh:14-48      public fields, OnUpdate, Rotate, GetPosition
//   RendererSettings Core/Scene/RendererSettings.h   same fields and enums
//
// Differences a caller sees (INTEGRATION.md lists the editor-side edits):
//   * no GL interop: GetRenderTargetImage_name() is replaced by ReadRenderTarget(float*) / DeviceRenderTarget();
//   * Camera is a plain host object (no cudaMallocManaged `Managed` base), copied by value at each Render;
//   * errors throw drt::Error instead of printing and exit(99) (Editor/Common/CudaCommon.cu:4-13).
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "drt.h"

namespace drt {
struct Error : std::runtime_error {
    int code;
    Error(int c, const char *msg) : std::runtime_error(msg ? msg : "drt error"), code(c) {}
};
inline void check(int rc) { if (rc < 0) throw Error(rc, drt_last_error()); }
}  // namespace drt

struct float2_ { float x, y; };         // stand-ins for CUDA's vector types in this header's public fields
struct float3_ { float x, y, z; };
struct float4_ { float x, y, z, w; };

// Core/Scene/RendererSettings.h:4-35
struct RendererSettings {
    enum class RenderModes { NORMALMODE = 0, DEBUGMODE = 1 };
    enum class DebugModes { ALBEDO_DEBUG = 0, NORMAL_DEBUG = 1, BARYCENTRIC_DEBUG = 2, UVS_DEBUG = 3, MESHBVH_DEBUG = 4, WORLDBVH_DEBUG = 5 };
    bool gamma_correction = true;
    bool tone_mapping = true;
    bool enableSunlight = false;
    int max_samples = 500;
    int ray_bounce_limit = 2;
    RenderModes RenderMode = RenderModes::NORMALMODE;
    DebugModes DebugMode = DebugModes::ALBEDO_DEBUG;
    float2_ sunlight_dir = { -0.803f, 0.681f };
    float3_ sunlight_color = { 1.000f, 0.944f, 0.917f };
    float sunlight_intensity = 30;
    float3_ sky_color = { 0.25f, 0.498f, 0.80f };
    float sky_intensity = 20;

    drt_settings pod() const {
        drt_settings s;
        s.gamma_correction = gamma_correction; s.tone_mapping = tone_mapping; s.enable_sunlight = enableSunlight;
        s.max_samples = max_samples; s.ray_bounce_limit = ray_bounce_limit;
        s.render_mode = (int)RenderMode; s.debug_mode = (int)DebugMode;
        s.sunlight_dir[0] = sunlight_dir.x; s.sunlight_dir[1] = sunlight_dir.y;
        s.sunlight_color[0] = sunlight_color.x; s.sunlight_color[1] = sunlight_color.y; s.sunlight_color[2] = sunlight_color.z;
        s.sunlight_intensity = sunlight_intensity;
        s.sky_color[0] = sky_color.x; s.sky_color[1] = sky_color.y; s.sky_color[2] = sky_color.z;
        s.sky_intensity = sky_intensity;
        return s;
    }
};

inline float deg2rad(float degree) { const float PI = 3.14159265359f; return degree * (PI / 180.f); }    // Camera.cu:125-129

// Core/Scene/Camera.cuh:14-48
class Camera {
public:
    explicit Camera(float3_ pos = { 0, 2, 5 }) : m_Position(pos) { m_Right_dir = cross(m_Forward_dir, m_Up_dir); }

    void OnUpdate(float3_ velocity, float delta) {                       // Camera.cu:44-58
        drt_camera_move(&m_Position.x, &m_Right_dir.x, &m_Up_dir.x, &m_Forward_dir.x, &velocity.x, m_movement_speed, delta);
    }
    void Rotate(float4_ d) {                                             // Camera.cu:61-80 (sin_x, cos_x, sin_y, cos_y)
        drt_camera_rotate(&m_Forward_dir.x, &m_Right_dir.x, &m_Up_dir.x, &d.x);
    }
    float3_ GetPosition() const { return m_Position; }
    void setMovementSpeed(float speed) { m_movement_speed = speed; }

    float exposure = 1;
    float vfov_rad = deg2rad(60);
    float zfar = 0, znear = 0, m_AspectRatio = 0;
    float defocus_angle = 0;
    float focus_dist = 10;
    float m_movement_speed = 10;
    float3_ m_Position = { 0, 2, 5 };
    float3_ m_Forward_dir = { 0, 0, -1 };
    float3_ m_Up_dir = { 0, 1, 0 };
    float3_ m_Right_dir = { 0, 1, 0 };

    drt_camera pod() const {
        drt_camera c;
        c.exposure = exposure; c.vfov_rad = vfov_rad; c.defocus_angle = defocus_angle; c.focus_dist = focus_dist;
        c.position[0] = m_Position.x; c.position[1] = m_Position.y; c.position[2] = m_Position.z;
        c.forward[0] = m_Forward_dir.x; c.forward[1] = m_Forward_dir.y; c.forward[2] = m_Forward_dir.z;
        return c;
    }

private:
    static float3_ cross(float3_ a, float3_ b) { return { a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
};

// Core/Scene/Mesh.cuh:8-18 (what the editor's metrics loop reads, EditorLayer.cpp:61-64)
struct Mesh { const char *name = ""; int m_primitives_offset = -1; size_t m_trisCount = 0; };

// Core/Scene/Scene.cuh:41-57
struct Scene {
    Scene() : m_PrimitivesBuffer{ this }, m_BVHNodes{ this }, handle(drt_scene_create()) {
        if (!handle) throw drt::Error(DRT_ERR_INVALID, drt_last_error());
    }
    ~Scene() { drt_scene_destroy(handle); }
    Scene(const Scene &) = delete;
    Scene &operator=(const Scene &) = delete;

    // strict = true: read the file as the glTF 2.0 specification defines it (drt.h DRT_LOAD_STRICT) instead of as Scene.cu does
    bool loadGLTFmodel(const char *filepath, bool strict = false) {
        drt::check(drt_scene_load_gltf_ex(handle, filepath, strict ? DRT_LOAD_STRICT : 0u));
        refresh();
        return true;
    }

    // host-side copies of what the reference keeps in thrust device vectors; enough for `.size()` and a range-for
    std::vector<Mesh> m_Meshes;
    std::vector<drt_material> m_Material;
    std::vector<drt_texture_info> m_Textures;
    // m_PrimitivesBuffer / m_BVHNodes live inside the scene handle; these members only name them, so that
    // `scene.d_BVHTreeRoot = builder.buildIterative(scene.m_PrimitivesBuffer, scene.m_BVHNodes)` (EditorLayer.cpp:55) compiles
    struct Part { Scene *scene; };
    Part m_PrimitivesBuffer, m_BVHNodes;
    const void *d_BVHTreeRoot = nullptr;              // non-null once a BVH has been built

    size_t meshCount() const { return (size_t)drt_scene_mesh_count(handle); }
    size_t trianglesCount() const { return (size_t)drt_scene_triangle_count(handle); }
    size_t materialsCount() const { return (size_t)drt_scene_material_count(handle); }
    size_t texturesCount() const { return (size_t)drt_scene_texture_count(handle); }
    std::vector<drt_triangle> primitives() const {                        // m_PrimitivesBuffer
        std::vector<drt_triangle> v(trianglesCount());
        if (!v.empty()) drt::check(drt_scene_get_triangles(handle, v.data(), (int32_t)v.size()));
        return v;
    }
    std::vector<drt_bvh_node> bvhNodes() const {                          // m_BVHNodes (root last)
        std::vector<drt_bvh_node> v((size_t)drt_scene_node_count(handle));
        if (!v.empty()) drt::check(drt_scene_get_nodes(handle, v.data(), (int32_t)v.size()));
        return v;
    }
    // new: load index of every triangle of primitives() (drt_scene_get_triangle_order)
    std::vector<int32_t> TriangleOrder() const {
        std::vector<int32_t> v(trianglesCount());
        if (!v.empty()) drt::check(drt_scene_get_triangle_order(handle, v.data(), (int32_t)v.size()));
        return v;
    }
    // new: the twin of every half-edge 3 t + e of primitives(), -1 on a boundary edge, -2 where the edge is non-manifold, flipped or
    // of zero length, by bit-equal positions (drt_scene_edge_adjacency); needs a BVH: the table is in tree order
    std::vector<int32_t> EdgeAdjacency() const {
        std::vector<int32_t> v(3 * trianglesCount());
        drt::check(drt_scene_edge_adjacency(handle, v.data(), (uint32_t)v.size()));
        return v;
    }
    // new: refit the BVH to moved vertices, float[n][3][3] in load order; normals nullptr = keep them (drt_scene_refit)
    void Refit(const float *positions, const float *normals = nullptr) { drt::check(drt_scene_refit(handle, positions, normals)); }
    void refresh() {                                                      // after anything that changes the scene
        std::vector<drt_mesh> meshes(meshCount());
        if (!meshes.empty()) drt::check(drt_scene_get_meshes(handle, meshes.data(), (int32_t)meshes.size()));
        m_Meshes.clear();
        for (const drt_mesh &m : meshes) { Mesh out; out.m_primitives_offset = m.primitives_offset; out.m_trisCount = (size_t)m.tris_count; m_Meshes.push_back(out); }
        m_Material.resize(materialsCount());
        if (!m_Material.empty()) drt::check(drt_scene_get_materials(handle, m_Material.data(), (int32_t)m_Material.size()));
        m_Textures.resize(texturesCount());
        for (size_t i = 0; i < m_Textures.size(); i++) drt::check(drt_scene_get_texture_info(handle, (int32_t)i, &m_Textures[i]));
    }

    drt_scene *handle;
};

// new: the edge adjacency of a query mesh, Scene::EdgeAdjacency's rule on the nine coordinates of each drt_tri in the caller's order
// (drt_tri_edge_adjacency): 3 values per triangle, host memory; what Renderer::ChainIntersections takes as query_adj
inline std::vector<int32_t> TriEdgeAdjacency(const drt_tri *tris, uint32_t n) {
    std::vector<int32_t> v(3 * (size_t)n);
    drt::check(drt_tri_edge_adjacency(tris, n, v.data(), (uint32_t)v.size()));
    return v;
}

// Core/BVH/BVHBuilder.cuh:12-23
class BVHBuilder {
public:
    int m_BinCount = 8;
    int m_TargetLeafPrimitivesCount = 6;
    int m_BuildDevice = -1;               // new: >= 0 runs the same build on that GPU (drt_scene_build_bvh_device)
    float m_LastBuildDeviceMs = 0;
    // the reference passes (scene.m_PrimitivesBuffer, scene.m_BVHNodes) and stores the returned root pointer
    // (EditorLayer.cpp:55); here the scene owns both, so the scene is the argument.
    void buildIterative(Scene &scene) {
        if (m_BuildDevice >= 0)
            drt::check(drt_scene_build_bvh_device(scene.handle, m_TargetLeafPrimitivesCount, m_BinCount, m_BuildDevice, &m_LastBuildDeviceMs));
        else
            drt::check(drt_scene_build_bvh(scene.handle, m_TargetLeafPrimitivesCount, m_BinCount));
        scene.d_BVHTreeRoot = scene.handle;
    }
    // BVHBuilder.cu:100-173: the same tree through recursion -- same nodes, same triangle order, node ARRAY in the recursion's
    // order (children after both of their subtrees); always on the host
    void build(Scene &scene) {
        drt::check(drt_scene_build_bvh_recursive(scene.handle, m_TargetLeafPrimitivesCount, m_BinCount));
        scene.d_BVHTreeRoot = scene.handle;
    }
    // the reference's spelling (EditorLayer.cpp:55): both arguments name parts of one scene; returns the root token
    const void *buildIterative(Scene::Part &primitives, Scene::Part &nodes) {
        if (primitives.scene != nodes.scene) throw drt::Error(DRT_ERR_INVALID, "primitives and nodes of different scenes");
        buildIterative(*primitives.scene);
        return primitives.scene->d_BVHTreeRoot;
    }
    const void *build(Scene::Part &primitives, Scene::Part &nodes) {
        if (primitives.scene != nodes.scene) throw drt::Error(DRT_ERR_INVALID, "primitives and nodes of different scenes");
        build(*primitives.scene);
        return primitives.scene->d_BVHTreeRoot;
    }
};

// Core/Sampler.cuh:5-13: the interface the reference declares and never implements (PCGSampler is an empty class there, RayGen.cuh
// seeds by hand).  Here PCGSampler is the RayGen recipe behind that interface, on the host: seed = (x + y * width) * sampleidx
// (RayGen.cuh:74-75), + dimension (the bounce index, :91), draws = randomFloat (Random.cu:13-17) -- the numbers a path of the
// kernels draws, for tools that want to follow one.
class Sampler {
public:
    virtual ~Sampler() = default;
    virtual void StartSampler(float2_ pixel, uint32_t sampleidx, int dimension) = 0;   // dim replaces bounces
    virtual float Get1DSample() = 0;
    virtual float2_ Get2DSample() = 0;
    virtual float2_ GetPixel2D() = 0;
};
class PCGSampler : public Sampler {
public:
    explicit PCGSampler(uint32_t image_width) : m_width(image_width) {}
    void StartSampler(float2_ pixel, uint32_t sampleidx, int dimension) override {
        m_pixel = pixel;
        m_seed = ((uint32_t)pixel.x + (uint32_t)pixel.y * m_width) * sampleidx + (uint32_t)dimension;
    }
    float Get1DSample() override { return drt_random_float(&m_seed); }
    float2_ Get2DSample() override { float2_ v; v.x = drt_random_float(&m_seed); v.y = drt_random_float(&m_seed); return v; }
    float2_ GetPixel2D() override { return m_pixel; }
    uint32_t seed() const { return m_seed; }
    void setSeed(uint32_t s) { m_seed = s; }
private:
    uint32_t m_width, m_seed = 0;
    float2_ m_pixel = { 0, 0 };
};

// Core/Renderer.hpp:14-47.  Renderer(device) renders on one GPU; Renderer({0, 1, ..., 7}) renders on several GPUs of the
// node (drt_group_*: framebuffer stripes per device, gathered into the first device's image over RCCL) behind the same calls.
class Renderer {
public:
    explicit Renderer(int device = 0) : handle(drt_renderer_create(device)) { if (!handle) throw drt::Error(DRT_ERR_DEVICE, drt_last_error()); }
    explicit Renderer(const std::vector<int> &devices) {
        std::vector<int32_t> d(devices.begin(), devices.end());
        group = drt_group_create(d.data(), (int32_t)d.size());
        if (!group) throw drt::Error(DRT_ERR_DEVICE, drt_last_error());
        handle = drt_group_renderer(group, 0);
    }
    ~Renderer() { if (group) drt_group_destroy(group); else drt_renderer_destroy(handle); }
    Renderer(const Renderer &) = delete;
    Renderer &operator=(const Renderer &) = delete;

    void ResizeBuffer(uint32_t width, uint32_t height) {
        drt::check(group ? drt_group_resize(group, width, height) : drt_renderer_resize(handle, width, height));
    }
    void Render(Camera *cam, const Scene &scene, float *delta) { RenderBatch(cam, scene, 1, delta); }
    // spp batch: frames getSampleCount() .. +n-1 in one launch, same image as n Render() calls
    void RenderBatch(Camera *cam, const Scene &scene, uint32_t n_frames, float *delta) {
        drt_settings s = m_RendererSettings.pod();
        drt_camera c = cam->pod();
        m_AdaptiveFrame = false;
        if (group) {
            drt::check(drt_group_set_settings(group, &s));
            drt::check(drt_group_render_batch(group, &c, scene.handle, n_frames, delta));
        } else {
            drt::check(drt_renderer_set_settings(handle, &s));
            drt::check(drt_renderer_render_batch(handle, &c, scene.handle, n_frames, delta));
        }
    }
    uint32_t getBufferWidth() const { return drt_renderer_width(handle); }
    uint32_t getBufferHeight() const { return drt_renderer_height(handle); }
    uint32_t getSampleCount() const { return drt_renderer_sample_count(handle); }
    void resetAccumulationBuffer() { drt::check(group ? drt_group_reset(group) : drt_renderer_reset(handle)); }
    int deviceCount() const { return group ? (int)drt_group_size(group) : 1; }
    // opt-in material model (drt.h drt_material_model; off = the reference's image): emissive term, metallic lobe, dielectric lobe
    void setMaterialModel(bool emissive, bool specular, float emissive_scale = 1.0f, bool transmission = false) {
        drt_material_model m = { emissive ? 1 : 0, specular ? 1 : 0, emissive_scale, transmission ? 1 : 0 };
        const int n = deviceCount();
        for (int i = 0; i < n; i++) drt::check(drt_renderer_set_material_model(group ? drt_group_renderer(group, i) : handle, &m));
    }

    // replaces GLuint& GetRenderTargetImage_name(): RGBA32F, row 0 = bottom, width*height*4 floats
    void ReadRenderTarget(float *dst) {
        const size_t n = (size_t)getBufferWidth() * getBufferHeight() * 4;
        drt::check(gathered() ? drt_group_read_rgba32f(group, dst, n) : drt_renderer_read_rgba32f(handle, dst, n));
    }
    void *DeviceRenderTarget() { return gathered() ? drt_group_device_rgba(group) : drt_renderer_device_rgba(handle); }
    // Batched ray queries (drt_renderer_trace_rays / _occluded: device arrays, enqueued on `stream`, NULL = the renderer's).
    // A multi-device renderer answers them on its first device (handle = drt_group_renderer(group, 0)).
    void TraceRays(const Scene &scene, const drt_ray *rays, drt_hit *hits, uint32_t n, void *stream = nullptr) {
        drt::check(drt_renderer_trace_rays(handle, scene.handle, rays, hits, n, stream));
    }
    void Occluded(const Scene &scene, const drt_ray *rays, uint8_t *occluded, uint32_t n, void *stream = nullptr) {
        drt::check(drt_renderer_occluded(handle, scene.handle, rays, occluded, n, stream));
    }
    // new: the closest point of the mesh for each of n points (drt_renderer_nearest: device arrays, enqueued on `stream`); after
    // Refit the moved geometry is the one queried
    void Nearest(const Scene &scene, const drt_point *points, drt_nearest *out, uint32_t n, void *stream = nullptr) {
        drt::check(drt_renderer_nearest(handle, scene.handle, points, out, n, stream));
    }
    // new: the first contact of a sphere of radius radii[i] moving along rays[i] with the mesh (drt_renderer_sphere_cast: device
    // arrays, enqueued on `stream`); after Refit the moved geometry is the one queried
    void SphereCast(const Scene &scene, const drt_ray *rays, const float *radii, drt_sweep_hit *out, uint32_t n, void *stream = nullptr) {
        drt::check(drt_renderer_sphere_cast(handle, scene.handle, rays, radii, out, n, stream));
    }
    // new: every triangle each ray passes through (drt_renderer_crossings), the inside vote of each point, 0..3 with 2 or more =
    // inside (drt_renderer_inside), and Nearest's records with side = -1 inside / +1 outside (drt_renderer_signed_distance);
    // rule = DRT_INSIDE_PARITY or DRT_INSIDE_WINDING.  Device arrays, enqueued on `stream`.
    void Crossings(const Scene &scene, const drt_ray *rays, drt_crossings *out, uint32_t n, void *stream = nullptr) {
        drt::check(drt_renderer_crossings(handle, scene.handle, rays, out, n, stream));
    }
    void Inside(const Scene &scene, const drt_point *points, uint8_t *votes, uint32_t n, int32_t rule = DRT_INSIDE_PARITY, void *stream = nullptr) {
        drt::check(drt_renderer_inside(handle, scene.handle, points, votes, n, rule, stream));
    }
    void SignedDistance(const Scene &scene, const drt_point *points, drt_nearest *out, uint32_t n, int32_t rule = DRT_INSIDE_PARITY,
                        void *stream = nullptr) {
        drt::check(drt_renderer_signed_distance(handle, scene.handle, points, out, n, rule, stream));
    }
    // new: generalised winding numbers, the inside test for meshes that are open or unevenly oriented -- w = the triangles' signed solid
    // angles at each point over 4 pi, on the tree with one dipole per far subtree (drt_renderer_winding_numbers); one byte w >= threshold
    // (drt_renderer_winding_inside); Nearest's records with side = -1 where w >= threshold, else +1
    // (drt_renderer_winding_signed_distance).  beta: a node is replaced by its dipole beyond beta radii, +inf = the exact sum; first
    // order only.  Device arrays, enqueued on `stream`.
    void WindingNumbers(const Scene &scene, const drt_point *points, float *out, uint32_t n, float beta = 2.0f, void *stream = nullptr) {
        drt::check(drt_renderer_winding_numbers(handle, scene.handle, points, n, beta, out, stream));
    }
    void WindingInside(const Scene &scene, const drt_point *points, uint8_t *out, uint32_t n, float beta = 2.0f, float threshold = 0.5f,
                       void *stream = nullptr) {
        drt::check(drt_renderer_winding_inside(handle, scene.handle, points, n, beta, threshold, out, stream));
    }
    void WindingSignedDistance(const Scene &scene, const drt_point *points, drt_nearest *out, uint32_t n, float beta = 2.0f,
                               float threshold = 0.5f, void *stream = nullptr) {
        drt::check(drt_renderer_winding_signed_distance(handle, scene.handle, points, n, beta, threshold, out, stream));
    }
    // new: a watertight triangle mesh from a float32 [Z][Y][X] field by marching tetrahedra (drt_renderer_isosurface): one drt_iso_tri
    // {v[3][3], cube, code, 0} per triangle in ascending cube, tetrahedron and table order, shared vertices bit-equal, normals towards
    // f >= level (flip = 1: away from it).  Rows are the cubes along x of one (y, z): row r's records go to out[offsets[r] ..
    // offsets[r + 1]), clamped to out_capacity, miss records (cube = 0xffffffff) behind them; counts[r] = all of them, stored or not.
    // out null iff out_capacity == 0 (a pure count; offsets may be null then); border NaN = none.  No scene and no tree; triangle soup,
    // no index buffer.  `grid` is host memory, the arrays are device arrays, out 16-byte aligned, enqueued on `stream`.
    void Isosurface(const float *field, const drt_grid &grid, float level, const uint32_t *offsets, drt_iso_tri *out, uint32_t out_capacity,
                    uint32_t *counts, bool flip = false, float border = std::numeric_limits<float>::quiet_NaN(), void *stream = nullptr) {
        drt::check(drt_renderer_isosurface(handle, field, &grid, level, border, flip ? 1 : 0, offsets, out, out_capacity, counts, stream));
    }
    // new: the index buffer of a triangle soup (drt_renderer_weld): n triangles `stride` bytes apart (36: float [N][3][3]; 48: drt_tri /
    // drt_iso_tri), corners with bit-equal positions become one vertex, numbered by first appearance.  faces int32 [n][3]; first [V] the
    // representative corner and vertices [V][3] its position, the first `capacity` of them (vertices may be null; first null iff
    // capacity == 0); vertex_count one word, always the total.  No scene and no tree; device arrays, enqueued on `stream`.
    void Weld(const void *tris, uint32_t n, uint32_t stride, int32_t *faces, int32_t *first, float *vertices, uint32_t capacity,
              uint32_t *vertex_count, void *stream = nullptr) {
        drt::check(drt_renderer_weld(handle, tris, n, stride, faces, first, vertices, capacity, vertex_count, stream));
    }
    // new: vertex normals of an indexed mesh (drt_renderer_vertex_normals): float [V][3], angle-weighted (DRT_NORMALS_ANGLE) or
    // area-weighted (DRT_NORMALS_AREA), summed in 64-bit fixed point so the bytes do not depend on the order; zeros for a vertex that no
    // triangle with an area names.
    void VertexNormals(const float *vertices, uint32_t n_vertices, const int32_t *faces, uint32_t n_tris, float *out,
                       int32_t weight = DRT_NORMALS_ANGLE, void *stream = nullptr) {
        drt::check(drt_renderer_vertex_normals(handle, vertices, n_vertices, faces, n_tris, weight, out, stream));
    }
    // new: Laplacian / Taubin smoothing of an indexed mesh (drt_renderer_smooth_vertices): one umbrella step per factor (host memory,
    // |f| <= 1; {0.5, -0.53, ...} is Taubin's), vertices with fixed[v] != 0 stay (fixed may be null).  out may not alias vertices.
    void SmoothVertices(const float *vertices, uint32_t n_vertices, const int32_t *faces, uint32_t n_tris, const float *factors,
                        uint32_t n_factors, float *out, const uint8_t *fixed = nullptr, void *stream = nullptr) {
        drt::check(drt_renderer_smooth_vertices(handle, vertices, n_vertices, faces, n_tris, factors, n_factors, fixed, out, stream));
    }
    // new: mesh simplification by vertex clustering (drt_renderer_simplify): the vertices of one cell of `grid` become one vertex, placed
    // at the cell's quadric optimum (DRT_SIMPLIFY_QUADRIC) or at the members' mean (DRT_SIMPLIFY_MEAN); vertices outside the grid stay.
    // cluster int32 [V] the new id of every vertex; out_vertices [C][3] and first [C], the first vertex_capacity of them; out_faces
    // [M][3] and source [M] (the input triangle), the first tri_capacity of them; counts two words, C then M, always the totals.
    // A pair of outputs is null iff its capacity is 0.  No scene and no tree; device arrays, enqueued on `stream`.
    void Simplify(const float *vertices, uint32_t n_vertices, const int32_t *faces, uint32_t n_tris, const drt_grid &grid, int32_t *cluster,
                  float *out_vertices, int32_t *first, uint32_t vertex_capacity, int32_t *out_faces, int32_t *source, uint32_t tri_capacity,
                  uint32_t *counts, int32_t placement = DRT_SIMPLIFY_QUADRIC, void *stream = nullptr) {
        drt::check(drt_renderer_simplify(handle, vertices, n_vertices, faces, n_tris, &grid, placement, cluster, out_vertices, first,
                                         vertex_capacity, out_faces, source, tri_capacity, counts, stream));
    }
    // new: the edge adjacency of a triangle list on the device, by bit-equal positions (drt_renderer_tri_adjacency; stride 36 or 48) or by
    // vertex index (drt_renderer_face_adjacency): adj[3 t + e] = the twin half-edge, -1 on a boundary edge, -2 on every other edge --
    // drt_tri_edge_adjacency's bytes.  With edge, half_edge and edge_count (null together): the undirected edges numbered by first
    // appearance.  Device arrays, enqueued on `stream`.
    void TriAdjacency(const void *tris, uint32_t n, uint32_t stride, int32_t *adj, int32_t *edge = nullptr, int32_t *half_edge = nullptr,
                      uint32_t capacity = 0, uint32_t *edge_count = nullptr, void *stream = nullptr) {
        drt::check(drt_renderer_tri_adjacency(handle, tris, n, stride, adj, edge, half_edge, capacity, edge_count, stream));
    }
    void FaceAdjacency(const int32_t *faces, uint32_t n, int32_t *adj, int32_t *edge = nullptr, int32_t *half_edge = nullptr,
                       uint32_t capacity = 0, uint32_t *edge_count = nullptr, void *stream = nullptr) {
        drt::check(drt_renderer_face_adjacency(handle, faces, n, adj, edge, half_edge, capacity, edge_count, stream));
    }
    // new: one level of subdivision of an indexed mesh (drt_renderer_subdivide): every triangle becomes four, out_faces int32 [4 N][3];
    // the even vertices keep their ids and the odd vertex of undirected edge e (drt_renderer_face_adjacency's numbering) is V + e.
    // DRT_SUBDIVIDE_LOOP smooths (Loop's weights, the open and non-manifold edges as creases), DRT_SUBDIVIDE_MIDPOINT only refines.
    // out_vertices [V'][3] and parents [V'][2] (the two ends an odd vertex lies between; may be null), the first vertex_capacity of
    // them (V + 3 N always suffices); vertex_count one word, always V' = V + E.  No scene and no tree; device arrays, enqueued on `stream`.
    void Subdivide(const float *vertices, uint32_t n_vertices, const int32_t *faces, uint32_t n_tris, float *out_vertices, int32_t *parents,
                   uint32_t vertex_capacity, int32_t *out_faces, uint32_t *vertex_count, int32_t scheme = DRT_SUBDIVIDE_LOOP,
                   void *stream = nullptr) {
        drt::check(drt_renderer_subdivide(handle, vertices, n_vertices, faces, n_tris, scheme, out_vertices, parents, vertex_capacity,
                                          out_faces, vertex_count, stream));
    }
    // new: out[v] = 1 iff a half-edge with adj == -1 (with DRT_BOUNDARY_BAD_EDGES also -2) starts or ends at vertex v
    // (drt_renderer_boundary_vertices); uint8 [V].
    void BoundaryVertices(const int32_t *faces, const int32_t *adj, uint32_t n_tris, uint32_t n_vertices, uint8_t *out, uint32_t flags = 0,
                          void *stream = nullptr) {
        drt::check(drt_renderer_boundary_vertices(handle, faces, adj, n_tris, n_vertices, flags, out, stream));
    }
    // new: the triangles each ray passes through, sorted by (t, prim) (drt_renderer_list_hits): ray i's records go to
    // hits[offsets[i] .. offsets[i+1]), clamped to hits_capacity, miss records behind them; counts[i] = all of them, stored or not.
    // counts may be null, hits may be null iff hits_capacity == 0.  Device arrays, enqueued on `stream`.
    void ListHits(const Scene &scene, const drt_ray *rays, const uint32_t *offsets, drt_hit *hits, uint32_t hits_capacity, uint32_t *counts,
                  uint32_t n, void *stream = nullptr) {
        drt::check(drt_renderer_list_hits(handle, scene.handle, rays, offsets, hits, hits_capacity, counts, n, stream));
    }
    // new: the triangles nearest each point within its max_dist, sorted by (d2, prim) (drt_renderer_nearest_list): point i's records go
    // to near[offsets[i] .. offsets[i+1]), clamped to near_capacity, miss records behind them.  mode DRT_NEAR_GATHER: every triangle
    // within the radius, counts[i] = all of them, stored or not; mode DRT_NEAR_K: the cap_i nearest, counts[i] = the stored ones.
    // surf (the closest points and sides, parallel to near) and counts may be null, near may be null iff near_capacity == 0.  Device
    // arrays, enqueued on `stream`.
    void NearestList(const Scene &scene, const drt_point *points, const uint32_t *offsets, drt_near *near, drt_near_surf *surf,
                     uint32_t near_capacity, uint32_t *counts, uint32_t n, int32_t mode, void *stream = nullptr) {
        drt::check(drt_renderer_nearest_list(handle, scene.handle, points, offsets, near, surf, near_capacity, counts, n, mode, stream));
    }
    // new: the triangles that touch each query box, an oriented box drt_box {center, half, axis[3]} (drt_renderer_overlap_boxes).  mode
    // DRT_OVERLAP_LIST: box i's triangle indices in ascending order go to prims[offsets[i] .. offsets[i+1]), clamped to prims_capacity,
    // -1 behind them, counts[i] = all listed, stored or not; counts may be null, prims may be null iff prims_capacity == 0.  mode
    // DRT_OVERLAP_ANY: counts[i] = 0 or 1, offsets is not read, prims must be null and prims_capacity 0.  Device arrays, enqueued on
    // `stream`.
    void OverlapBoxes(const Scene &scene, const drt_box *boxes, const uint32_t *offsets, int32_t *prims, uint32_t prims_capacity,
                      uint32_t *counts, uint32_t n, int32_t mode, void *stream = nullptr) {
        drt::check(drt_renderer_overlap_boxes(handle, scene.handle, boxes, offsets, prims, prims_capacity, counts, n, mode, stream));
    }
    // new: the mesh triangles that each query triangle touches, a drt_tri {v[3][3]} (drt_renderer_overlap_triangles).  Modes, segments,
    // counts and the null rules are OverlapBoxes'.  Device arrays, enqueued on `stream`.
    void OverlapTriangles(const Scene &scene, const drt_tri *tris, const uint32_t *offsets, int32_t *prims, uint32_t prims_capacity,
                          uint32_t *counts, uint32_t n, int32_t mode, void *stream = nullptr) {
        drt::check(drt_renderer_overlap_triangles(handle, scene.handle, tris, offsets, prims, prims_capacity, counts, n, mode, stream));
    }
    // new: the mesh triangle nearest each query triangle within max_dist[i] (null: infinite), a drt_tri_near {point_q[3], d2,
    // point_t[3], prim, u, v, feature} per query (drt_renderer_triangle_distance); d2 = 0 with feature | 16 where the overlap predicate
    // does not separate the pair; the miss record is zeros with d2 = max_dist^2 and prim = -1.  Mode DRT_TRIDIST_ANY ends a query at
    // the first pair within the distance.  Device arrays, tris and out 16-byte aligned, enqueued on `stream`.
    void TriangleDistance(const Scene &scene, const drt_tri *tris, const float *max_dist, drt_tri_near *out, uint32_t n,
                          int32_t mode = DRT_TRIDIST_NEAREST, void *stream = nullptr) {
        drt::check(drt_renderer_triangle_distance(handle, scene.handle, tris, max_dist, out, n, mode, stream));
    }
    // new: the first contact of each query triangle translating along motions[i].d with the mesh, the smallest t in [0, tmax), a
    // drt_tri_hit {point[3], t, normal[3], prim, u, v, feature} per cast (drt_renderer_triangle_cast); t = 0 with feature | 16 where
    // the overlap predicate does not separate the pair at the start; the miss record is zeros with t = tmax, prim = -1, feature = -1.
    // Mode DRT_TRICAST_ANY ends a cast at the first pair found.  No rotation, no thickness, no penetration depth.  Device arrays, all
    // three 16-byte aligned, enqueued on `stream`.
    void TriangleCast(const Scene &scene, const drt_tri *tris, const drt_motion *motions, drt_tri_hit *out, uint32_t n,
                      int32_t mode = DRT_TRICAST_FIRST, void *stream = nullptr) {
        drt::check(drt_renderer_triangle_cast(handle, scene.handle, tris, motions, out, n, mode, stream));
    }
    // new: what lies on the surface at each reference {t, prim, u, v} -- the output of TraceRays and the other queries as it stands --
    // a drt_surface per reference (drt_renderer_surface_lookup): position, the stored face normal, the interpolated vertex normals
    // (NOT normalised; `normals`: a device float[n_tris][3][3] in load order, nullptr = the host scene's), uv, albedo and alpha by the
    // reference's nearest-texel rule, the material's other fields, the load index.  prim outside [0, n_tris): the miss record, zeros
    // with material = load_index = texture = -1.  Device arrays, refs and out 16-byte aligned, enqueued on `stream`.
    void SurfaceLookup(const Scene &scene, const drt_hit *refs, drt_surface *out, uint32_t n, const float *normals = nullptr,
                       void *stream = nullptr) {
        drt::check(drt_renderer_surface_lookup(handle, scene.handle, refs, normals, out, n, stream));
    }
    // new: the inclusive table of integer area weights the samples are drawn from, a device uint64[n_tris] (drt_renderer_surface_weights)
    void SurfaceWeights(const Scene &scene, uint64_t *cdf, void *stream = nullptr) {
        drt::check(drt_renderer_surface_weights(handle, scene.handle, cdf, stream));
    }
    // new: n references {0, prim, u, v} drawn on the mesh with probability proportional to area, samples first .. first + n - 1 of the
    // stream `seed` (drt_renderer_sample_surface); they feed SurfaceLookup as they are.  Independent hashes: not stratified.
    void SampleSurface(const Scene &scene, uint32_t seed, drt_hit *out, uint32_t n, uint32_t first = 0, void *stream = nullptr) {
        drt::check(drt_renderer_sample_surface(handle, scene.handle, seed, first, out, n, stream));
    }
    // new: ambient occlusion -- for each drt_ao_point {p, max_dist, n, bias} `samples` occlusion rays from p + n * bias in the renderer's
    // bounce directions normalize(n + unit-sphere draw), none longer than max_dist, and per point a drt_ao_result {open, bent[3]}: the
    // number of open samples and the integer sum of their directions * 65536 (drt_renderer_ambient_occlusion).  Pass unit normals for a
    // cosine-weighted answer; max_dist < 0 or NaN skips a point ({-1, 0, 0, 0}).  Sample streams are (seed, first + index): `first`
    // continues a batch.  Device arrays, 16-byte aligned, enqueued on `stream`; no falloff, not stratified.
    void AmbientOcclusion(const Scene &scene, const drt_ao_point *points, drt_ao_result *out, uint32_t n, uint32_t samples = 64,
                          uint32_t seed = 0, uint32_t first = 0, void *stream = nullptr) {
        const drt_ao_params params = { samples, seed, first, 0u };
        drt::check(drt_renderer_ambient_occlusion(handle, scene.handle, points, n, &params, out, stream));
    }
    // new: the segments where each query plane dot(n, x) = d cuts the mesh, a drt_plane {n[3], d} (drt_renderer_plane_sections): one
    // drt_section {p[3], prim, q[3], code} per cut triangle in ascending triangle index, p -> q counter-clockwise about n on a closed
    // mesh with outward faces; the miss record is zeros with prim = -1.  Modes (DRT_SECTION_LIST / DRT_SECTION_ANY), segments, counts
    // and the null rules are OverlapBoxes', with 32-byte records.  Endpoints of neighbouring triangles agree only as far as their stored
    // vertices do: weld with a tolerance.  Device arrays, planes and out 16-byte aligned, enqueued on `stream`.
    void PlaneSections(const Scene &scene, const drt_plane *planes, const uint32_t *offsets, drt_section *out, uint32_t out_capacity,
                       uint32_t *counts, uint32_t n, int32_t mode, void *stream = nullptr) {
        drt::check(drt_renderer_plane_sections(handle, scene.handle, planes, offsets, out, out_capacity, counts, n, mode, stream));
    }
    // new: where each query triangle cuts the mesh, a drt_tri {v[3][3]} (drt_renderer_intersect_triangles): one drt_isect {p[3], prim,
    // q[3], code} per cutting pair in ascending triangle index, p -> q along cross(query normal, triangle normal), each endpoint one of
    // the pair's four edge cut points; code = cp + 16 * cq, an endpoint's code the scene triangle's edge 0..2 or 4 + the query's edge;
    // the miss record is zeros with prim = -1.  Coplanar pairs and zero-area triangles give nothing.  Segments, counts and the null rules
    // are PlaneSections' in mode DRT_SECTION_LIST; there is no mode.  Device arrays, tris and out 16-byte aligned, enqueued on `stream`.
    void IntersectTriangles(const Scene &scene, const drt_tri *tris, const uint32_t *offsets, drt_isect *out, uint32_t out_capacity,
                            uint32_t *counts, uint32_t n, void *stream = nullptr) {
        drt::check(drt_renderer_intersect_triangles(handle, scene.handle, tris, offsets, out, out_capacity, counts, n, stream));
    }
    // new: the records of PlaneSections chained into contours by the mesh's edge adjacency, integers only (drt_renderer_chain_sections):
    // plane i owns segs and slots [splits[i], splits[i + 1]); slots[pos] = {seg, first, length, flags} in canonical order -- a path from
    // its record without a predecessor, a cycle from its smallest record, chains by their first record, miss records last; flags bit 0 =
    // closed, bits 1..3 = the record's exit status.  chains (may be null) = per plane {chains, closed ones}.  Device arrays, segs and
    // slots 16-byte aligned, enqueued on `stream`.
    void ChainSections(const Scene &scene, const drt_section *segs, const uint32_t *splits, drt_chain_slot *slots, uint32_t *chains, uint32_t n,
                       uint32_t total, void *stream = nullptr) {
        drt::check(drt_renderer_chain_sections(handle, scene.handle, segs, splits, slots, chains, n, total, stream));
    }
    // new: the records of IntersectTriangles chained into curves across scene triangles and across queries, integers only
    // (drt_renderer_chain_intersections): query i owns segs [splits[i], splits[i + 1]); query_adj = TriEdgeAdjacency of the query mesh,
    // copied to the device (3 n values).  A record that leaves through a scene edge continues in the twin triangle with the same query,
    // one that leaves through a query edge in the same triangle with the twin query.  slots[pos] = {seg, first, length, flags} in one
    // canonical order over the whole list, as ChainSections; counts (may be null) = {chains, closed ones, records that are not live}.
    // Device arrays, segs and slots 16-byte aligned, enqueued on `stream`.
    void ChainIntersections(const Scene &scene, const drt_isect *segs, const uint32_t *splits, const int32_t *query_adj, drt_chain_slot *slots,
                            uint32_t *counts, uint32_t n, uint32_t total, void *stream = nullptr) {
        drt::check(drt_renderer_chain_intersections(handle, scene.handle, segs, splits, query_adj, slots, counts, n, total, stream));
    }
    // new: mesh topology (drt.h "mesh topology"), all in tree order and on device arrays, enqueued on `stream`.  ShellLabels: labels[t] =
    // the smallest triangle index of t's shell (triangles joined by twin half-edges), counts (may be null) = {shells, open half-edges,
    // bad half-edges}.  BoundaryLoops: the boundary half-edges chained into loops by rotation about their end vertices, one 16-byte
    // slot per record, truncated at `capacity` (slots null and capacity 0: a pure count); counts = {records, loops, closed loops}.
    // ShellTerms: per triangle {c.x, c.y, c.z, w} in float64 from the device's positions, c = cross(e1, e2) and w = dot(v0, c): the sum
    // of w / 6 over a shell is its volume, |c| / 2 a triangle's area.  terms and slots 16-byte aligned.
    void ShellLabels(const Scene &scene, int32_t *labels, uint32_t *counts = nullptr, void *stream = nullptr) {
        drt::check(drt_renderer_shell_labels(handle, scene.handle, labels, counts, stream));
    }
    void BoundaryLoops(const Scene &scene, drt_loop_slot *slots, uint32_t capacity, uint32_t *counts, void *stream = nullptr) {
        drt::check(drt_renderer_boundary_loops(handle, scene.handle, slots, capacity, counts, stream));
    }
    void ShellTerms(const Scene &scene, double *terms, void *stream = nullptr) {
        drt::check(drt_renderer_shell_terms(handle, scene.handle, terms, stream));
    }
    // new: RayGen's primary rays of n_cams cameras for a width x height image, frame `frame_index` (drt_renderer_camera_rays): a device
    // drt_path_ray[n_cams * width * height], enqueued on `stream`
    void CameraRays(const drt_camera *cams, uint32_t n_cams, uint32_t width, uint32_t height, uint32_t frame_index, drt_path_ray *rays,
                    void *stream = nullptr) {
        drt::check(drt_renderer_camera_rays(handle, cams, n_cams, width, height, frame_index, rays, stream));
    }
    // new: one path-traced sample per ray with the current settings (drt_renderer_radiance): device float4 out[n], (c, 1) or rgb += c
    void Radiance(const Scene &scene, const drt_path_ray *rays, float *out, uint32_t n, bool accumulate = false, void *stream = nullptr) {
        drt_settings s = m_RendererSettings.pod();
        drt::check(drt_renderer_set_settings(handle, &s));
        drt::check(drt_renderer_radiance(handle, scene.handle, rays, out, n, accumulate ? 1 : 0, stream));
    }
    // First-hit guide buffers of frame `frame_index` (drt_renderer_render_guides): a device drt_guide[width*height], enqueued on `stream`
    // new: refit this renderer's device copy of the scene to moved vertices (device pointers, load order; drt_renderer_refit).
    // Blocking; returns the device ms.  Reset the accumulation afterwards, as after a camera move.
    float Refit(const Scene &scene, const float *positions, const float *normals = nullptr, void *stream = nullptr) {
        float ms = 0.f;
        drt::check(drt_renderer_refit(handle, scene.handle, positions, normals, &ms, stream));
        return ms;
    }
    void RenderGuides(Camera *cam, const Scene &scene, uint32_t frame_index, drt_guide *guides, void *stream = nullptr) {
        drt_settings s = m_RendererSettings.pod();
        drt_camera c = cam->pod();
        drt::check(drt_renderer_set_settings(handle, &s));
        drt::check(drt_renderer_render_guides(handle, &c, scene.handle, frame_index, guides, stream));
    }
    // Edge-avoiding a-trous filter of the current frame, guided by frame 1's albedo and normal (drt_renderer_denoise; blocking).
    // A multi-device renderer is refused (DRT_ERR_UNSUPPORTED): the filter needs the whole frame on one device.
    void Denoise(Camera *cam, const Scene &scene, float *delta, int iterations = 5, float sigma_color = 0.5f, float sigma_normal = 0.1f,
                 float sigma_albedo = 0.1f) {
        drt_denoise_params p = { iterations, sigma_color, sigma_normal, sigma_albedo };
        drt_settings s = m_RendererSettings.pod();
        drt_camera c = cam->pod();
        drt::check(drt_renderer_set_settings(handle, &s));
        drt::check(drt_renderer_denoise(handle, &c, scene.handle, &p, delta));
    }
    // the last Denoise result: RGBA32F, row 0 = bottom, width*height*4 floats (what a "denoise" toggle shows instead of ReadRenderTarget)
    void ReadDenoisedTarget(float *dst) {
        drt::check(drt_renderer_read_denoised_rgba32f(handle, dst, (size_t)getBufferWidth() * getBufferHeight() * 4));
    }
    void *DeviceDenoisedTarget() { return drt_renderer_device_denoised(handle); }
    // Temporal reprojection + variance-guided a-trous filter of the current frame (drt_renderer_temporal_denoise; blocking): call
    // once per rendered pose, the history travels from call to call.  params NULL = drt_default_temporal_params.  The result is
    // read with ReadDenoisedTarget / DeviceDenoisedTarget.  A multi-device renderer is refused (DRT_ERR_UNSUPPORTED).
    void TemporalDenoise(Camera *cam, const Scene &scene, float *delta, const drt_temporal_params *params = nullptr) {
        drt_temporal_params p;
        drt_default_temporal_params(&p);
        if (params) p = *params;
        drt_settings s = m_RendererSettings.pod();
        drt_camera c = cam->pod();
        drt::check(drt_renderer_set_settings(handle, &s));
        drt::check(drt_renderer_temporal_denoise(handle, &c, scene.handle, &p, delta));
    }
    void ResetTemporalHistory() { drt::check(drt_renderer_temporal_reset(handle)); }      // after a cut or untracked moved geometry: N = 1 again
    // Follow geometry that Refit moves: TemporalDenoise then reprojects every moved triangle through the state it had at the last
    // call (drt_renderer_track_motion).  AdvanceMotion makes the current geometry the previous one without a TemporalDenoise.
    void TrackMotion(bool enable = true) { drt::check(drt_renderer_track_motion(handle, enable ? 1 : 0)); }
    void AdvanceMotion() { drt::check(drt_renderer_motion_advance(handle)); }
    // (fx - x, fy - y, z, flag) per pixel into the device buffer out (float4[width*height]); prev_cam NULL = the camera of the
    // last TemporalDenoise (drt_renderer_motion_vectors; enqueues only)
    void MotionVectors(Camera *cam, const Scene &scene, float *out, Camera *prev_cam = nullptr, void *stream = nullptr) {
        drt_settings s = m_RendererSettings.pod();
        drt_camera c = cam->pod(), pc;
        if (prev_cam) pc = prev_cam->pod();
        drt::check(drt_renderer_set_settings(handle, &s));
        drt::check(drt_renderer_motion_vectors(handle, &c, prev_cam ? &pc : nullptr, scene.handle, out, stream));
    }
    // Guide-driven upscaling of the frame to out_width x out_height (drt_renderer_upscale; blocking): the framebuffer, or with
    // params->source == 1 the last Denoise / TemporalDenoise result, rebuilt at full size from full-size first-hit guides.
    // params NULL = drt_default_upscale_params.  A multi-device renderer is refused (DRT_ERR_UNSUPPORTED).
    void Upscale(Camera *cam, const Scene &scene, uint32_t out_width, uint32_t out_height, float *delta, const drt_upscale_params *params = nullptr) {
        drt_upscale_params p;
        drt_default_upscale_params(&p);
        if (params) p = *params;
        drt_settings s = m_RendererSettings.pod();
        drt_camera c = cam->pod();
        drt::check(drt_renderer_set_settings(handle, &s));
        drt::check(drt_renderer_upscale(handle, &c, scene.handle, out_width, out_height, &p, delta));
        m_UpscaledWidth = out_width; m_UpscaledHeight = out_height;
    }
    // the last Upscale result: RGBA32F, row 0 = bottom, out_width*out_height*4 floats
    void ReadUpscaledTarget(float *dst) {
        drt::check(drt_renderer_read_upscaled_rgba32f(handle, dst, (size_t)m_UpscaledWidth * m_UpscaledHeight * 4));
    }
    void *DeviceUpscaledTarget() { return drt_renderer_device_upscaled(handle); }
    // Adaptive sampling (drt_renderer_render_adaptive; blocking): one call spends params->budget samples (0 = 4 per pixel) where the
    // per-pixel state says the noise is and leaves sum / n in the framebuffer (ReadRenderTarget and the filters read it).  The first
    // call after a reset or resize is uniform.  params NULL = drt_default_adaptive_params.  A multi-device renderer is refused.
    drt_adaptive_info RenderAdaptive(Camera *cam, const Scene &scene, const drt_adaptive_params *params = nullptr) {
        drt_adaptive_params p;
        drt_default_adaptive_params(&p);
        if (params) p = *params;
        drt_adaptive_info info;
        drt_settings s = m_RendererSettings.pod();
        drt_camera c = cam->pod();
        drt::check(drt_renderer_set_settings(handle, &s));
        drt::check(drt_renderer_render_adaptive(handle, &c, scene.handle, &p, &info));
        m_AdaptiveFrame = true;
        return info;
    }
    void ResetAdaptive() { drt::check(drt_renderer_adaptive_reset(handle)); }
    // the adaptive state, width*height*4 words: which 0 = (sum rgb, n as uint32), 1 = (m1, m2, the last call's q and count as uint32)
    void ReadAdaptiveState(int which, void *dst) {
        drt::check(drt_renderer_read_adaptive(handle, which, dst, (size_t)getBufferWidth() * getBufferHeight() * 16));
    }
    // the history of the last TemporalDenoise, width*height*4 floats: which 0 = (colour rgb, N), 1 = (m1, m2, variance, weight sum)
    void ReadTemporal(int which, float *dst) {
        drt::check(drt_renderer_read_temporal(handle, which, dst, (size_t)getBufferWidth() * getBufferHeight() * 4));
    }

    // A group's frame is the image its stripes were gathered into.  An adaptive call (a group of one device only: a sharded renderer
    // is refused) writes the device's own framebuffer instead, which then is the frame until the next RenderBatch.
    bool gathered() const { return group && !m_AdaptiveFrame; }

    RendererSettings m_RendererSettings;
    bool m_AdaptiveFrame = false;         // the last frame came from RenderAdaptive
    uint32_t m_UpscaledWidth = 0, m_UpscaledHeight = 0;      // the size of the last Upscale
    drt_renderer *handle = nullptr;       // the (first) device's renderer
    drt_group *group = nullptr;           // set when the renderer spans several devices
};
