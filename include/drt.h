/*
 * drt.h -- C ABI of the MI355X-native DustRayTracer path-tracing core.
 *
 * One shared library (dustraytracer_amd/libdrt_hip.so) exports exactly these
 * symbols.  They are what a binding for the reference's Renderer / Scene /
 * BVHBuilder / Camera classes needs (include/DustRayTracer.hpp is that binding
 * for C++; INTEGRATION.md shows the editor-side change).  Plain pointers and
 * sizes only.  Citations are relative to /root/reference/DustRayTracer/src/.
 *
 * Error model (replaces Editor/Common/CudaCommon.cu:4-13, which prints,
 * cudaDeviceReset()s and exit(99)s): every call returns DRT_OK (0) or a
 * negative drt_status; drt_last_error() returns a thread-local message.
 * Nothing in the library ever calls exit().
 *
 * There is NO CPU fallback: a call that needs the GPU fails with
 * DRT_ERR_DEVICE when no gfx950 device is usable.
 */
#ifndef DRT_H
#define DRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: drt_counters grew by sampler_tries; drt_group_* and drt_material_model entry points (round 2) are part of it; the ray-query
 * entry points (drt_renderer_trace_rays / _occluded), the guide / denoise entry points, the refit entry points and the camera-ray /
 * radiance entry points, the upscaling entry points, the adaptive-sampling entry points, the nearest-surface entry point
 * (drt_renderer_nearest), the crossing-count entry points (drt_renderer_crossings / _inside / _signed_distance), the hit-list entry
 * point (drt_renderer_list_hits), the sphere-cast entry point (drt_renderer_sphere_cast), the nearest-list entry point
 * (drt_renderer_nearest_list), the box-overlap entry point (drt_renderer_overlap_boxes), the triangle-overlap entry point
 * (drt_renderer_overlap_triangles), the plane-section entry point (drt_renderer_plane_sections), the intersection-segment entry
 * point (drt_renderer_intersect_triangles), the intersection-curve entry points (drt_tri_edge_adjacency,
 * drt_renderer_chain_intersections), the triangle-distance entry point (drt_renderer_triangle_distance), the triangle-cast entry
 * point (drt_renderer_triangle_cast), the surface entry points (drt_renderer_surface_lookup, drt_renderer_surface_weights,
 * drt_renderer_sample_surface), the ambient-occlusion entry point (drt_renderer_ambient_occlusion) and the winding-number entry
 * points (drt_renderer_winding_numbers / _winding_inside / _winding_signed_distance) are additions to it; so is the isosurface
 * entry point (drt_renderer_isosurface), and so are the welding entry points (drt_renderer_weld / _vertex_normals /
 * _smooth_vertices), and so is the simplification entry point (drt_renderer_simplify), and so are the device edge-adjacency entry
 * points (drt_renderer_tri_adjacency / _face_adjacency / _boundary_vertices / _adjacency_route), and so is the subdivision entry
 * point (drt_renderer_subdivide) */
#define DRT_ABI_VERSION 2

typedef enum {
    DRT_OK = 0,
    DRT_ERR_INVALID = -1,      /* bad argument / bad handle state */
    DRT_ERR_IO = -2,           /* file missing or unreadable */
    DRT_ERR_PARSE = -3,        /* glTF / PNG content not understood */
    DRT_ERR_UNSUPPORTED = -4,  /* valid input outside the reference loader's subset */
    DRT_ERR_DEVICE = -5,       /* HIP error, no device, out of device memory */
    DRT_ERR_BVH = -6           /* builder cannot terminate on this input (the reference hangs) */
} drt_status;

/* ---- PODs mirroring the reference's public data ---- */

/* Core/Scene/RendererSettings.h:4-35 (bools widened to int32 for a stable ABI). */
typedef struct drt_settings {
    int32_t gamma_correction;      /* :22 default 1 */
    int32_t tone_mapping;          /* :23 default 1 */
    int32_t enable_sunlight;       /* :24 default 0 */
    int32_t max_samples;           /* :25 default 500; Render is a no-op once sample_count == max_samples */
    int32_t ray_bounce_limit;      /* :26 default 2; the path loop runs i = 0..limit inclusive */
    int32_t render_mode;           /* :27 0 NORMALMODE, 1 DEBUGMODE */
    int32_t debug_mode;            /* :28 0 ALBEDO 1 NORMAL 2 BARYCENTRIC 3 UVS 4 MESHBVH 5 WORLDBVH */
    float   sunlight_dir[2];       /* :29 */
    float   sunlight_color[3];     /* :30 */
    float   sunlight_intensity;    /* :31 */
    float   sky_color[3];          /* :32 */
    float   sky_intensity;         /* :34 */
} drt_settings;

/* Opt-in material model -- NOT reference behaviour.  The reference loads emissiveFactor, roughnessFactor and
 * metallicFactor (Scene.cu:71-75, Material.cuh:9,17,20) and its kernel reads none of them (RayGen.cuh:111-134).  With everything
 * zero (the default) the image is the reference's, bit for bit.  emissive != 0: a hit adds  EmmisiveFactor * emissive_scale *
 * throughput  (the throughput before that hit's albedo).  specular != 0: a hit on a Metallic material continues along
 * reflect(normalize(ray.dir), N) + Roughness * randomUnitSphereVec3(seed)  -- the same random draws as the diffuse bounce -- and the
 * path ends if that direction points into the surface.  transmission != 0: a hit on a Transmission material (Material.cuh:20-21; the
 * reference's loader never sets it: drt_scene_add_material_ex does) is a dielectric interface, computed with the reference's own
 * unused helpers refract / reflectance (CudaMath/Random.cu:26-40):  v = normalize(ray.dir), cos = fminf(dot(-v, N), 1), ri = front face ?
 * 1 / refractive_index : refractive_index;  total internal reflection (ri * sqrtf(1 - cos^2) > 1) or reflectance(cos, ri) >
 * randomFloat(seed)  ->  continue along reflect(v, N) from P + 0.001 N, else along refract(v, N, ri) from P - 0.001 N.  That one
 * randomFloat replaces the bounce's randomUnitSphereVec3; pow(x, 5) is ((x x)(x x)) x; takes precedence over the metallic lobe.
 * The rule is this library's (the reference has none): oracle/drt_oracle.c states it first, tests/test_material_model.py checks
 * cases that can be derived by hand -- "parity unpinned" by construction.
 * Rendered by path_pool (every lobe) and by the general wave_queue kernel (emissive, specular). */
typedef struct drt_material_model {
    int32_t emissive;
    int32_t specular;
    float   emissive_scale;        /* default 1 */
    int32_t transmission;
} drt_material_model;

/* Core/Scene/Camera.cuh:30-47: the fields the kernel reads (Camera.cu:82-123). */
typedef struct drt_camera {
    float exposure;                /* :32 */
    float vfov_rad;                /* :33 */
    float defocus_angle;           /* :37 */
    float focus_dist;              /* :38 */
    float position[3];             /* :43 m_Position */
    float forward[3];              /* :44 m_Forward_dir */
} drt_camera;

/* Core/Scene/Vertex.cuh:4-12 (32 bytes) */
typedef struct drt_vertex { float position[3]; float normal[3]; float uv[2]; } drt_vertex;

/* Core/Scene/Triangle.cuh:7-19 (128 bytes, same field offsets as the reference struct) */
typedef struct drt_triangle {
    float centroid[3]; float _pad0;
    drt_vertex vertex[3];
    float face_normal[3];
    int32_t material;
} drt_triangle;

/* Core/BVH/BVHNode.cuh:14-44 (44 bytes). The root is the LAST node (BVHBuilder.cu:85). */
typedef struct drt_bvh_node {
    uint8_t is_leaf; uint8_t _pad0[3];
    float bmin[3], bmax[3];
    int32_t child1, child2;
    int32_t prim_count, prim_start;
} drt_bvh_node;

/* Core/Scene/Material.cuh:4-23 (44 bytes); the kernel reads albedo + albedo_tex only (RayGen.cuh:112-117). */
typedef struct drt_material {
    float albedo[3];
    float emissive[3];
    int32_t albedo_tex;
    float roughness;
    uint8_t transmission; uint8_t _pad0[3];
    float refractive_index;
    uint8_t metallic; uint8_t _pad1[3];
} drt_material;

/* Core/Scene/Mesh.cuh:8-18 */
typedef struct drt_mesh { int32_t primitives_offset; int32_t tris_count; } drt_mesh;

typedef struct drt_texture_info { int32_t width, height, components; } drt_texture_info;

/* Exact device-side work counters for one render call (drt_renderer_set_counting). */
typedef struct drt_counters {
    uint64_t samples, rays, node_visits, inner_visits, tri_tests, hits_textured, hits_flat,
             shadow_rays, inner_visits_shadow, tri_tests_shadow;
    /* wave_queue kernel only: executions of the T / N / S / R phase (per wave) and lanes served by them */
    uint64_t phase_execs[4], phase_lanes[4];
    uint64_t phase_ticks[4], wave_ticks;   /* counting build: shader-clock ticks per phase / per wave lifetime, summed over waves */
    uint64_t sampler_tries;                /* path_pool: candidates drawn by randomUnitSphereVec3 (Random.cu:50-58) for bounce directions */
} drt_counters;

typedef struct drt_scene drt_scene;         /* replaces struct Scene, Core/Scene/Scene.cuh:41-57 */
typedef struct drt_renderer drt_renderer;   /* replaces class Renderer, Core/Renderer.hpp:14-47 */

/* ---- library ---- */
int         drt_abi_version(void);
const char *drt_last_error(void);
int         drt_device_count(void);                       /* usable HIP devices, 0 when none */
void        drt_default_settings(drt_settings *out);      /* RendererSettings.h:22-34 */
void        drt_default_camera(drt_camera *out);          /* Camera.cuh:32-46 + EditorLayer.cpp:35-40 */
/* Camera host logic, one implementation for every binding (fp32, the reference's operation order):
 * Camera::Rotate (Camera.cu:61-80; delta = sin_x, cos_x, sin_y, cos_y) updates forward and right in place;
 * Camera::OnUpdate (Camera.cu:44-58) moves position by speed * (right*v.x + up*v.y + forward*v.z) * delta. */
void        drt_camera_rotate(float forward[3], float right[3], const float up[3], const float delta[4]);
void        drt_camera_move(float position[3], const float right[3], const float up[3], const float forward[3],
                            const float velocity[3], float speed, float delta);

/* ---- Scene: host-side load + BVH build (Scene.cu:181-317, BVHBuilder.cu:11-92) ---- */
drt_scene *drt_scene_create(void);
void       drt_scene_destroy(drt_scene *s);                                   /* Scene::~Scene, Scene.cu:319-344 */
int        drt_scene_load_gltf(drt_scene *s, const char *path);               /* Scene::loadGLTFmodel */
/* flags = 0: as above.  DRT_LOAD_STRICT: read the file as the glTF 2.0 specification defines it instead of as the
 * reference's loader does (Scene.cu:120-200 ignores node transforms and the scene graph, accessor byteOffset /
 * componentType / byteStride, reads indices as u16 from byte 0 of the buffer, uses texture indices as image indices, and
 * crashes on nodes without a mesh).  A file that satisfies the reference's assumptions loads identically either way. */
#define DRT_LOAD_STRICT 1u
int        drt_scene_load_gltf_ex(drt_scene *s, const char *path, uint32_t flags);
/* Programmatic alternative to a file: de-indexed streams, 3 vertices per triangle. */
int        drt_scene_set_geometry(drt_scene *s, const float *positions, const float *normals, const float *uvs,
                                  const int32_t *material_ids, int32_t n_tris);
int        drt_scene_add_material(drt_scene *s, const float albedo[3], int32_t albedo_tex);
int        drt_scene_add_material_ex(drt_scene *s, const drt_material *m);   /* every field (emissive, roughness, metallic: drt_material_model) */
/* CudaMath/Random.cu:6-17 on the host: the RNG the kernels use (pcg_hash; randomFloat = hash, then seed / 2^32 in [0, 1]). */
uint32_t   drt_pcg_hash(uint32_t input);
float      drt_random_float(uint32_t *seed);
int        drt_scene_add_texture(drt_scene *s, const uint8_t *texels, int32_t width, int32_t height, int32_t components);
/* BVHBuilder::buildIterative.  A build that fails (DRT_ERR_BVH, from any of the three builders below) changes nothing: the scene
 * keeps the nodes and the triangle order it had. */
int        drt_scene_build_bvh(drt_scene *s, int32_t target_leaf_prims, int32_t bin_count);
/* The same build run on GPU `device`: identical nodes, node order and triangle order -- a bound that
 * is a zero may carry the other sign.  build_ms (may be NULL) receives the device time.  DRT_ERR_DEVICE without a GPU. */
/* BVHBuilder::build (BVH/BVHBuilder.cu:100-173): the same tree and triangle order as drt_scene_build_bvh, with the node array in
 * the order the reference's recursion appends it (a node's two children after both of their subtrees, root last). */
int        drt_scene_build_bvh_recursive(drt_scene *s, int32_t target_leaf_prims, int32_t bin_count);
int        drt_scene_build_bvh_device(drt_scene *s, int32_t target_leaf_prims, int32_t bin_count, int32_t device, float *build_ms);
/* Checks what the kernels index without checks: every triangle's material id, every material's texture index, the BVH's
 * child and triangle ranges.  DRT_ERR_INVALID names the first offender; rendering runs the same check before uploading. */
int        drt_scene_validate(const drt_scene *s);
int32_t    drt_scene_triangle_count(const drt_scene *s);                      /* m_PrimitivesBuffer.size() */
int32_t    drt_scene_node_count(const drt_scene *s);                          /* m_BVHNodes.size() */
int32_t    drt_scene_material_count(const drt_scene *s);
int32_t    drt_scene_texture_count(const drt_scene *s);
int32_t    drt_scene_mesh_count(const drt_scene *s);
int32_t    drt_scene_bvh_depth(const drt_scene *s);                           /* levels, 0 when no BVH */
int        drt_scene_get_triangles(const drt_scene *s, drt_triangle *out, int32_t cap);
int        drt_scene_get_nodes(const drt_scene *s, drt_bvh_node *out, int32_t cap);
int        drt_scene_get_materials(const drt_scene *s, drt_material *out, int32_t cap);
int        drt_scene_get_meshes(const drt_scene *s, drt_mesh *out, int32_t cap);
int        drt_scene_get_texture_info(const drt_scene *s, int32_t index, drt_texture_info *out);
int        drt_scene_get_texture_texels(const drt_scene *s, int32_t index, uint8_t *out, size_t cap);

/* ---- Renderer (Core/Renderer.hpp:14-47, Core/Renderer.cu) ---- */
drt_renderer *drt_renderer_create(int32_t device);                            /* Renderer::Renderer */
void          drt_renderer_destroy(drt_renderer *r);                          /* Renderer::~Renderer */
int           drt_renderer_resize(drt_renderer *r, uint32_t width, uint32_t height);   /* ResizeBuffer: no-op for equal size, else realloc + reset */
int           drt_renderer_set_settings(drt_renderer *r, const drt_settings *s);       /* writes m_RendererSettings (caller resets, EditorLayer.cpp:241-277) */
int           drt_renderer_set_material_model(drt_renderer *r, const drt_material_model *m);   /* see drt_material_model */
int           drt_renderer_get_material_model(const drt_renderer *r, drt_material_model *out);
int           drt_renderer_get_settings(const drt_renderer *r, drt_settings *out);
/* Render: ONE frame index, blocking, returns kernel ms in *delta_ms (Renderer.cu:80-117). No-op when sample_count == max_samples. */
int           drt_renderer_render(drt_renderer *r, const drt_camera *cam, const drt_scene *scene, float *delta_ms);
/* spp batch: frames sample_count .. sample_count+n_frames-1 in one launch; per-pixel sum order ((a+c_f)+c_f+1)+... is kept,
 * so the result is bit-identical to n_frames drt_renderer_render calls.  Clamped so that sample_count never passes max_samples. */
int           drt_renderer_render_batch(drt_renderer *r, const drt_camera *cam, const drt_scene *scene,
                                        uint32_t n_frames, float *delta_ms);
/* Non-blocking form: enqueues the batch on the renderer's stream and returns; drt_renderer_wait blocks until it is done
 * and returns its device time.  Lets a caller keep several frames in flight (one renderer + stream per frame). */
int           drt_renderer_render_batch_async(drt_renderer *r, const drt_camera *cam, const drt_scene *scene, uint32_t n_frames);
int           drt_renderer_wait(drt_renderer *r, float *delta_ms);
int           drt_renderer_reset(drt_renderer *r);                            /* resetAccumulationBuffer: zero + sample_count = 1 (and the adaptive state, if any, is dropped) */
uint32_t      drt_renderer_width(const drt_renderer *r);                      /* getBufferWidth */
uint32_t      drt_renderer_height(const drt_renderer *r);                     /* getBufferHeight */
uint32_t      drt_renderer_sample_count(const drt_renderer *r);               /* getSampleCount == m_FrameIndex (starts at 1) */
/* Framebuffer out (replaces the GL RGBA32F texture of Renderer.cu:48,70; row 0 = bottom, alpha = 1).
 * Sharded renderers hold local_rows rows; unsharded ones hold all of them. */
uint32_t      drt_renderer_local_rows(const drt_renderer *r);
int           drt_renderer_read_rgba32f(drt_renderer *r, float *dst, size_t dst_floats);   /* width*local_rows*4 */
int           drt_renderer_read_accum(drt_renderer *r, float *dst, size_t dst_floats);     /* width*local_rows*3 */
void         *drt_renderer_device_rgba(drt_renderer *r);                      /* device float4[width*local_rows] */
void         *drt_renderer_device_accum(drt_renderer *r);                     /* device float3[width*local_rows] */

/* ---- batched ray queries (new; the reference has TraceRay / RayTest, Kernel/TraceRay.cu:15-38, but no public entry) ----
 * One ray = org, tmin, dir, tmax (fp32).  dir is used as given (not normalised; t is in units of |dir|), inv_dir = 1/dir as
 * the renderer computes it.  The traversals are the renderer's, bit for bit (BVH/BVHTraversal.cuh:14-134):
 *   drt_renderer_trace_rays  traverseBVH started as TraceRay starts it: closest.t = tmax (TraceRay.cu:18), a node is culled
 *                            by !(-1 < d && d < tmax) (:38, the interval (-1, tmax) of RayGen), far child pushed first, strict <
 *                            (the first triangle found wins a tie), AnyHit alpha test.  Departure: a triangle hit counts only if
 *                            t > tmin (the reference's TODO "inner clipping", :37).  tmin = 0, tmax = FLT_MAX is TraceRay's hit.
 *   drt_renderer_occluded    traverseBVH_raytest.  Departures: the root is skipped if d < 0 || d > tmax, a child is pushed iff
 *                            d >= 0 && !(d > tmax) (tmax culls boxes), a triangle counts iff t > tmin && t < tmax && AnyHit.
 *                            tmin = 0, tmax = +inf is RayTest, the renderer's shadow test.
 * Results: drt_hit {t, prim, u, v}: prim = triangle index in drt_scene_get_triangles order, u, v = uvw.y, uvw.z of
 * Intersection.cu (uvw.x = 1 - u - v); a miss is {tmax, -1, 0, 0}.  occluded: one byte per ray, 0 or 1.  A result depends on
 * its ray and the scene only (not on its position in the array, the batch size or the scheduling).
 * rays / hits / occluded are device pointers on the renderer's device, rays and hits 16-byte aligned, n < 2^31; n == 0 is a
 * no-op.  hip_stream NULL = the renderer's stream.  The call enqueues and returns (nothing is synchronised); queries of one
 * renderer run in the order they were made, whatever their streams.  The scene is uploaded as for rendering (once, shared);
 * DRT_ERR_UNSUPPORTED for trees deeper than 64 levels; DRT_ERR_INVALID for null / misaligned / host or other-device pointers
 * and while a drt_renderer_render_batch_async batch is pending.  The framebuffer, sample count, counters and kernel info are
 * not touched. */
typedef struct drt_ray { float org[3]; float tmin; float dir[3]; float tmax; } drt_ray;      /* 32 B */
typedef struct drt_hit { float t; int32_t prim; float u, v; } drt_hit;                      /* 16 B */
int           drt_renderer_trace_rays(drt_renderer *r, const drt_scene *scene, const drt_ray *rays, drt_hit *hits, uint32_t n, void *hip_stream);
int           drt_renderer_occluded(drt_renderer *r, const drt_scene *scene, const drt_ray *rays, uint8_t *occluded, uint32_t n, void *hip_stream);

/* ---- nearest-surface queries (new; the reference asks the scene about rays only) ----
 * One query = a point p and a search radius max_dist; the answer is the closest point of the mesh within that radius.
 * All arithmetic is fp32 with one rounding per operation, in the order written; dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z, / is the
 * correctly rounded division.
 * Per triangle k: (v0, e1 = v1 - v0, e2 = v2 - v0) as the ray test reads them (the stored edges; v1, v2 are not recomputed).  The
 * closest point follows Ericson, Real-Time Collision Detection 5.1.5:
 *   ap = p - v0, d1 = dot(e1, ap), d2 = dot(e2, ap);  bp = ap - e1, d3 = dot(e1, bp), d4 = dot(e2, bp);
 *   cp = ap - e2, d5 = dot(e1, cp), d6 = dot(e2, cp);  vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4.
 * The first case that matches, in this order, gives (u, v):
 *   1. d1 <= 0 && d2 <= 0                         (0, 0)
 *   2. d3 >= 0 && d4 <= d3                        (1, 0)
 *   3. vc <= 0 && d1 >= 0 && d3 <= 0              (d1 / (d1 - d3), 0)
 *   4. d6 >= 0 && d5 <= d6                        (0, 1)
 *   5. vb <= 0 && d2 >= 0 && d6 <= 0              (0, d2 / (d2 - d6))
 *   6. va <= 0 && d4 - d3 >= 0 && d5 - d6 >= 0    w = (d4 - d3) / ((d4 - d3) + (d5 - d6)): (1 - w, w)
 *   7. otherwise                                  den = 1 / ((va + vb) + vc): (vb den, vc den)
 * Then c = (v0 + e1 u) + e2 v, diff = p - c, dist2 = dot(diff, diff).  A NaN dist2 (a NaN query; a zero-area triangle whose matching
 * case divides 0 by 0, such as case 3 when v0 = v1) never wins: every comparison below is a strict <.  A zero-area triangle whose
 * matching case has a quotient (v1 = v2, three collinear vertices) counts as the segment or point it is.
 * Box distance: per axis d = fmaxf(fmaxf(bmin - p, 0), p - bmax) (a NaN operand is dropped), box2 = (dx dx + dy dy) + dz dz.
 * Traversal: best = max_dist * max_dist, prim = -1.  The root is pushed with its box2.  A popped entry is dropped unless
 * box2 < best.  A leaf tests its triangles in order; a candidate replaces the result iff dist2 < best (the first one found wins a
 * tie).  An interior node computes box2 of both children and pushes a child iff its box2 < best, the farther one first
 * (b1 > b2 -> child 1), so the nearer one is popped first: drt_renderer_trace_rays' stack discipline with box2 in place of the entry
 * distance.
 * Result: on a hit drt_nearest {c, dist2, prim, u, v, side}, prim = triangle index in drt_scene_get_triangles order,
 * side = dot(p - c, fn) < 0 ? -1 : 1 with fn the stored face normal; on a miss (nothing within max_dist, NaN input)
 * {0, 0, 0, max_dist * max_dist, -1, 0, 0, 0}.  A result depends on its point and the scene only.
 * What this is not: alpha cut-outs are ignored (a geometric query).  `side` is the side of the nearest triangle's plane, not an
 * inside / outside classification: at an edge or vertex of a non-convex mesh it can disagree with a parity test (a robust sign --
 * pseudonormals, ray parity -- is out of scope).  One answer per point: k-nearest and radius-gather queries are
 * drt_renderer_nearest_list, below.
 * Conventions are drt_renderer_trace_rays': device pointers on the renderer's device, 16-byte aligned, n < 2^31, n == 0 is a no-op,
 * hip_stream NULL = the renderer's stream, the call only enqueues, in order with the other queries (the same event), the scene is
 * uploaded as for rendering and a refitted device copy (drt_renderer_refit) is the one queried.  Legal on a sharded renderer.  The
 * framebuffer, accumulation, sample count, counters, kernel info and kernel span are not touched.  Errors as for the ray queries,
 * DRT_ERR_UNSUPPORTED beyond 64 levels and DRT_ERR_INVALID while an asynchronous batch is pending included.
 * (The sign that `side` is not: drt_renderer_inside and drt_renderer_signed_distance, below.) */
typedef struct drt_point   { float p[3]; float max_dist; } drt_point;                                    /* 16 B */
typedef struct drt_nearest { float point[3]; float d2; int32_t prim; float u, v, side; } drt_nearest;   /* 32 B */
int           drt_renderer_nearest(drt_renderer *r, const drt_scene *scene, const drt_point *points, drt_nearest *out, uint32_t n, void *hip_stream);

/* ---- crossing counts, inside / outside and signed distance (new; the sign that drt_renderer_nearest leaves open) ----
 * Crossings of a ray (a drt_ray, read as drt_renderer_trace_rays reads it: dir as given, inv_dir = 1/dir): the triangles it passes
 * through, all of them.  The triangle test is the renderer's (Intersection.cu, the arithmetic of the ray queries) on the stored
 * (v0, e1, e2), with det = dot(e1, cross(dir, e2)).  A triangle counts iff the test hits, t > tmin and t < tmax.  Alpha cut-outs are
 * ignored (a geometric query, as drt_renderer_nearest is).  Per ray, count = the number of counted triangles and winding = the sum
 * over them of (det < 0 ? +1 : -1): exits minus entries by the triangle's own winding e1 x e2, not by the stored face normal.
 * Traversal is drt_renderer_occluded's without the early exit: the root is skipped if d < 0 || d > tmax, a child is pushed iff
 * d >= 0 && !(d > tmax), the farther child is pushed first, the same stack bound applies.  Each triangle lies in one leaf, so the
 * result does not depend on the traversal order.  Result: drt_crossings {count, winding}, 8 bytes; an empty scene or a NaN ray gives
 * {0, 0}.  (The boxes cull as they do for the ray queries: a triangle whose box the fp32 slab test misses is not counted.)
 * Inside vote of a point: three rays are cast from p with tmin = 0, tmax = +inf and the fixed fp32 directions
 *   D0 = (0.6180340f, 0.4142136f, 0.6687403f)   D1 = (-0.7320508f, 0.2360680f, 0.6403124f)   D2 = (0.3166248f, -0.8660254f, 0.3872983f)
 * used as given, not normalised; no component is zero, so the slab test's 0 * inf case cannot arise.  Ray j votes inside iff count_j
 * is odd (rule 0, parity) or winding_j != 0 (rule 1, winding).  The answer is one byte per point: the number of rays voting
 * inside, 0..3; inside means 2 or more.  drt_point's max_dist is ignored.
 * Signed distance: drt_renderer_nearest's record for the point, unchanged in its first seven words; the last word, side, is
 * replaced by -1 (inside) or +1 (outside) from the vote, in miss records too.
 * What this is not: a point on the surface has no defined answer (t > 1e-6 decides, per ray); parity assumes a closed mesh; winding
 * assumes consistent orientation as well.  Angle-weighted pseudonormals and generalised winding numbers for open meshes are out of
 * scope; an ordered list of the first K hits per ray is drt_renderer_list_hits, below.
 * Conventions and errors are drt_renderer_nearest's: device pointers on the renderer's device, rays / points / drt_nearest records
 * 16-byte aligned, drt_crossings 8-byte aligned, n < 2^31, n == 0 is a no-op, hip_stream NULL = the renderer's stream, the call only
 * enqueues, in order with the other queries, a refitted device copy is the one queried, legal on a sharded renderer,
 * DRT_ERR_UNSUPPORTED beyond 64 levels, DRT_ERR_INVALID while an asynchronous batch is pending and for a rule other than 0 or 1
 * (checked first).  drt_renderer_signed_distance enqueues the nearest query and then the vote on the same stream.  The framebuffer,
 * accumulation, sample count, counters, kernel info and kernel span are not touched. */
typedef struct drt_crossings { uint32_t count; int32_t winding; } drt_crossings;                         /* 8 B */
#define DRT_INSIDE_PARITY  0
#define DRT_INSIDE_WINDING 1
int           drt_renderer_crossings(drt_renderer *r, const drt_scene *scene, const drt_ray *rays, drt_crossings *out, uint32_t n, void *hip_stream);
int           drt_renderer_inside(drt_renderer *r, const drt_scene *scene, const drt_point *points, uint8_t *votes, uint32_t n, int32_t rule, void *hip_stream);
int           drt_renderer_signed_distance(drt_renderer *r, const drt_scene *scene, const drt_point *points, drt_nearest *out, uint32_t n, int32_t rule, void *hip_stream);

/* ---- ordered hit lists of rays (new; the triangles drt_renderer_crossings counts, handed out in order) ----
 * Hit list of a ray (a drt_ray, read as drt_renderer_trace_rays reads it: dir as given, inv_dir = 1/dir): the triangles it passes
 * through, sorted.  The triangle test is the renderer's (Intersection.cu, the arithmetic of the ray queries) on the stored
 * (v0, e1, e2); t, u and v carry the bits drt_renderer_trace_rays reports for that ray and triangle.  A triangle is listed iff the
 * test hits, t > tmin and t < tmax: exactly the rule of drt_renderer_crossings.  Alpha cut-outs are ignored (a geometric query), and
 * the boxes cull as they do there: a triangle whose box the fp32 slab test misses is not listed.  Traversal is
 * drt_renderer_crossings', unchanged: the root is skipped if d < 0 || d > tmax, a child is pushed iff d >= 0 && !(d > tmax), the
 * farther child is pushed first, the same stack bound applies.  So the set of listed triangles is the set drt_renderer_crossings
 * counts, and total == drt_crossings.count for the same ray.
 * Order: ascending t; equal t by ascending prim.  a comes before b iff a.t < b.t || (a.t == b.t && a.prim < b.prim).  A listed t is
 * never NaN and always > 1e-6, so the order is total and does not depend on the traversal.
 * Segments: offsets holds n + 1 uint32 values; ray i owns hits[offsets[i] .. offsets[i+1]).  Its capacity is
 * cap_i = offsets[i+1] > offsets[i] ? offsets[i+1] - offsets[i] : 0, then clamped so that offsets[i] + cap_i <= hits_capacity
 * (offsets[i] >= hits_capacity gives 0).  The call writes hits[offsets[i] + j] for j < cap_i and nothing else in hits, whatever
 * offsets contains (segments that overlap are written by more than one ray and hold no defined list).  Slot j < min(cap_i, total_i)
 * holds the j-th listed triangle in order, a drt_hit {t, prim, u, v}; the slots from min(cap_i, total_i) to cap_i - 1 hold the miss
 * record {tmax, -1, 0, 0}, tmax being the ray's own word, bit for bit, as in drt_renderer_trace_rays' miss.  counts[i] = total_i: all
 * listed triangles, not just the stored ones, which is how a caller sees truncation.  A result depends on the ray, the scene and
 * cap_i only, and the first K records of a longer list are the list at capacity K.  An empty scene or a NaN ray lists nothing.
 * Two uses: offsets[i] = K * i gives the first K hits of every ray as an [n, K] table in one pass; drt_renderer_crossings, an
 * exclusive scan of its counts into offsets and one pass give every hit of every ray (CSR) without a capacity guess.
 * counts may be NULL; hits may be NULL iff hits_capacity == 0 (a pure count); both NULL is DRT_ERR_INVALID.
 * What this is not: alpha-tested lists, per-hit normals or materials.  The boxes are NOT culled by the K-th distance once a list is
 * full: counts[i] would no longer be the total, and fp32 box distances and triangle distances do not order consistently, so the
 * stored records would depend on the traversal order.  Every ray traverses as drt_renderer_crossings does, whatever its capacity.
 * The insert moves records one slot at a time: the cost of a hit that arrives out of order grows with the capacity, which suits a
 * small K.
 * Conventions and errors are drt_renderer_crossings': handles are checked before n == 0, n == 0 is a no-op, n < 2^31, all pointers
 * are device pointers on the renderer's device, rays and hits 16-byte aligned, offsets and counts 4-byte aligned, hip_stream NULL =
 * the renderer's stream, the call only enqueues, in order with the other queries, a refitted device copy is the one queried, legal on
 * a sharded renderer, DRT_ERR_UNSUPPORTED beyond 64 levels, DRT_ERR_INVALID while an asynchronous batch is pending.  The framebuffer,
 * accumulation, sample count, counters, kernel info and kernel span are not touched. */
int           drt_renderer_list_hits(drt_renderer *r, const drt_scene *scene, const drt_ray *rays, const uint32_t *offsets, drt_hit *hits,
                                     uint32_t hits_capacity, uint32_t *counts, uint32_t n, void *hip_stream);

/* ---- nearest-triangle lists of points (new; drt_renderer_nearest's candidates, handed out in order) ----
 * Near list of a point (a drt_point, read as drt_renderer_nearest reads it): the triangles within max_dist of p, sorted by distance.
 * Per triangle and per box the arithmetic is drt_renderer_nearest's own on the stored (v0, e1, e2): the Ericson case chain gives
 * (u, v), c = (v0 + e1 u) + e2 v and dist2; box2 is its box distance.  d2, u and v carry the bits drt_renderer_nearest computes for
 * that point and triangle.  r2 = max_dist * max_dist, the point's own product.  A triangle is listed iff dist2 < r2; a NaN dist2 (a NaN
 * point, a zero-area triangle whose matching case divides 0 by 0) is never listed, and for a NaN max_dist r2 is some NaN and nothing is
 * listed.  Alpha cut-outs are ignored (a geometric query).
 * Order: ascending d2; equal d2 by ascending prim.  a comes before b iff a.d2 < b.d2 || (a.d2 == b.d2 && a.prim < b.prim).  A listed
 * d2 is never NaN, so the order is total and independent of the traversal.
 * Segments are drt_renderer_list_hits': offsets holds n + 1 uint32 values; point i owns near[offsets[i] .. offsets[i+1]).  Its capacity
 * is cap_i = offsets[i+1] > offsets[i] ? offsets[i+1] - offsets[i] : 0, then clamped so that offsets[i] + cap_i <= near_capacity
 * (offsets[i] >= near_capacity gives 0).  The call writes near[offsets[i] + j] for j < cap_i and nothing else in near, whatever
 * offsets contains (segments that overlap are written by more than one point and hold no defined list).  Slot j < stored_i holds the
 * j-th record of the list in order, a drt_near {d2, prim, u, v}; the slots from stored_i to cap_i - 1 hold the miss record
 * {r2, -1, 0, 0}, r2 being the point's own product, bit for bit.
 * surf may be NULL; otherwise it is a parallel array of near_capacity drt_near_surf records, written for the same slots and no others.
 * For a stored slot point = (v0 + e1 u) + e2 v and side = dot(p - point, fn) < 0 ? -1 : 1 with fn the stored face normal: the same
 * operations as drt_renderer_nearest's result, on the stored (prim, u, v).  For a miss slot {0, 0, 0, 0}.  It is filled when the point
 * finishes, so the records that move while a list is being sorted stay 16 bytes.
 * Search bound, evaluated at every pop and every push: keep(box2) = (mode == DRT_NEAR_K && stored == cap_i) ? box2 <= tail.d2
 * : box2 < r2, tail being the last stored record.  The <= is deliberate: a node at exactly the tail's distance may hold a triangle of
 * equal d2 and smaller prim, which comes before the tail.
 * Traversal is drt_renderer_nearest's: the root is pushed with its box2; a popped entry is dropped unless keep(box2); a leaf tests its
 * triangles in order, and a listed triangle enters the list if there is room or it comes before the tail (which then leaves); an
 * interior node computes box2 of both children and pushes each child that passes keep, the farther one first
 * (b1 > b2 -> child 1).  The same 64-level stack bound applies.
 * Mode DRT_NEAR_GATHER (0): the bound never shrinks.  counts[i] = total_i, all listed triangles, not just the stored ones, which is how
 * a caller sees truncation; stored_i = min(cap_i, total_i) and the stored records are the first cap_i of the full list.  Each triangle
 * lies in one leaf and the bound is constant, so neither the set nor the list depends on the traversal order, and the first K
 * records of a longer list are the list at capacity K.  (The boxes cull as they do for drt_renderer_nearest: a triangle whose box2 is
 * not below r2 is not listed.)  near may be NULL iff near_capacity == 0: a pure count.  Two passes give every triangle within a
 * radius without a capacity guess: a count with capacity 0, an exclusive scan of the counts into offsets, and a fill.
 * Mode DRT_NEAR_K (1): the cap_i nearest.  counts[i] = stored_i = min(cap_i, listed), the number stored.  A point with cap_i == 0 visits
 * nothing and counts 0.  offsets[i] = K * i gives the K nearest triangles of every point as an [n, K] table in one pass.  fp32 box
 * distances are not exactly conservative: a box2 can round above the dist2 of a triangle inside the box.  The stored records are
 * therefore defined by this traversal, as drt_renderer_nearest's answer is, not by a brute force over all triangles, although on
 * every input tested they equal one.
 * counts may be NULL; both near and counts NULL is DRT_ERR_INVALID.  A result depends on the point, the scene, cap_i and the mode only.
 * An empty scene lists nothing.
 * What this is not: point-to-point neighbours (the records are triangles of the mesh, not other query points); alpha-tested lists; a
 * large-K structure -- the insert moves one record per step, so the cost of a triangle that arrives out of order grows with the
 * capacity, which suits a small K.  Slot 0 of a mode-K list has drt_renderer_nearest's d2, but on an exact tie it holds the smaller
 * prim, not the first one found.
 * Conventions and errors are drt_renderer_list_hits', checked in its order: handles are checked before n == 0, then a mode outside
 * {0, 1} is DRT_ERR_INVALID (checked first after the handles), n == 0 is a no-op, n < 2^31, all pointers are device pointers on the
 * renderer's device, points, near and surf 16-byte aligned, offsets and counts 4-byte aligned, hip_stream NULL = the renderer's stream,
 * the call only enqueues, in order with the other queries, a refitted device copy is the one queried, legal on a sharded renderer,
 * DRT_ERR_UNSUPPORTED beyond 64 levels, DRT_ERR_INVALID while an asynchronous batch is pending.  The framebuffer, accumulation, sample
 * count, counters, kernel info and kernel span are not touched. */
typedef struct drt_near      { float d2; int32_t prim; float u, v; } drt_near;                           /* 16 B */
typedef struct drt_near_surf { float point[3]; float side; } drt_near_surf;                              /* 16 B */
#define DRT_NEAR_GATHER 0
#define DRT_NEAR_K      1
int           drt_renderer_nearest_list(drt_renderer *r, const drt_scene *scene, const drt_point *points, const uint32_t *offsets,
                                        drt_near *near, drt_near_surf *surf, uint32_t near_capacity, uint32_t *counts, uint32_t n,
                                        int32_t mode, void *hip_stream);

/* ---- box overlap queries (new; the triangles that touch each query box -- the first query about a volume) ----
 * One query = a drt_box: 64 bytes, 16-byte aligned, center[3], half[3], axis[3][3] and one pad word that is ignored.  axis[k] is the
 * world direction of box axis k, used as given: not normalised, not orthogonalised.  An axis-aligned box is axis = identity; with
 * identity axes every product below is exact, so the axis-aligned case needs no code path of its own.
 * All arithmetic is fp32 with one rounding per operation, in the order written.  dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z;
 * cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x).  fminf / fmaxf drop a NaN operand, as the box distance of
 * drt_renderer_nearest does.  Alpha cut-outs are ignored (a geometric query).
 * World bounds of the query, computed once per query: ext[j] = (|axis[0][j]| half[0] + |axis[1][j]| half[1]) + |axis[2][j]| half[2],
 * qmin = center - ext, qmax = center + ext.  (They hold the box when the axes are orthonormal.  The box itself is the set of x with
 * |dot(axis[k], x - center)| <= half[k]; axes shorter than 1 describe a box larger than these bounds, and the cull then decides.)
 * Node cull: a box (bmin, bmax) passes iff, on all three axes, qmin[j] <= bmax[j] && bmin[j] <= qmax[j].  The comparisons are closed
 * and no arithmetic is done on the node.  A NaN anywhere in the query makes some qmin / qmax NaN (an infinite half beside a zero axis
 * component does too: 0 * inf); then the root fails, so a NaN query lists nothing.
 * Traversal: the root is tested against the scene's root box; an interior node pushes each child that passes, child 2 first; a leaf
 * tests its triangles in order.  The same 64-level stack bound applies.  Each triangle lies in one leaf and the cull never changes
 * during a query, so the set of listed triangles does not depend on the traversal order.  The boxes cull as they do for the other
 * queries: a triangle whose leaf the cull rejects is not listed, whatever the triangle test would say -- the stored triangle is
 * (v0, e1, e2), and v0 + e1 can round one ulp outside a node box built from the real v1.
 * Triangle test: the separating-axis test of Akenine-Moller (2001) in the box's frame, on the stored (v0, e1, e2).
 * a = v0 - center; for k = 0..2: p0[k] = dot(axis[k], a), f1[k] = dot(axis[k], e1), f2[k] = dot(axis[k], e2); p1 = p0 + f1,
 * p2 = p0 + f2, g = f2 - f1.  With min3(x, y, z) = fminf(fminf(x, y), z) and max3 the same with fmaxf:
 *   box axes, for each k: ok iff min3(p0[k], p1[k], p2[k]) <= half[k] && max3(p0[k], p1[k], p2[k]) >= -half[k]
 *   plane: n = cross(f1, f2), d = dot(n, p0), r = (|n.x| half[0] + |n.y| half[1]) + |n.z| half[2]; ok iff fabsf(d) <= r
 *   nine edge axes L = cross(unit_k, E) for E in (f1, g, f2), k in 0..2, each with its two non-zero components only; s_i over
 *   i = 0, 1, 2 (all three projections, not the two-value shortcut), left operand first:
 *     k = 0, L = (0, -E.z, E.y): s_i = (-E.z) p_i.y + E.y p_i.z, r = half[1] |E.z| + half[2] |E.y|
 *     k = 1, L = (E.z, 0, -E.x): s_i = E.z p_i.x + (-E.x) p_i.z, r = half[0] |E.z| + half[2] |E.x|
 *     k = 2, L = (-E.y, E.x, 0): s_i = (-E.y) p_i.x + E.x p_i.y, r = half[0] |E.y| + half[1] |E.x|
 *     ok iff min3(s0, s1, s2) <= r && max3(s0, s1, s2) >= -r
 * The triangle is listed iff all 13 are ok.  Touching counts.  half = 0 is a point or a flat box, and it works.  A zero-area triangle
 * passes its zero cross axes with 0 <= 0, and the other axes decide it.  Only the predicate leaves the kernel, so bit for bit here
 * means that the 13 comparisons are made on the same rounded values.
 * Mode DRT_OVERLAP_LIST (0): segments are exactly drt_renderer_list_hits': offsets holds n + 1 uint32 values; box i owns
 * prims[offsets[i] .. offsets[i+1]).  Its capacity is cap_i = offsets[i+1] > offsets[i] ? offsets[i+1] - offsets[i] : 0, then clamped
 * so that offsets[i] + cap_i <= prims_capacity (offsets[i] >= prims_capacity gives 0).  The call writes prims[offsets[i] + j] for
 * j < cap_i and nothing else in prims, whatever offsets contains (segments that overlap are written by more than one box and hold no
 * defined list).  The records are int32 triangle indices in ascending order; unused slots hold -1.  counts[i] is the total number
 * listed, stored or not, which is how a caller sees truncation; the first K of a longer list are the list at capacity K.  prims may
 * be NULL iff prims_capacity == 0: a pure count.  counts may be NULL; both prims and counts NULL is DRT_ERR_INVALID.  Two passes give
 * every triangle of every box without a capacity guess: a count with capacity 0, an exclusive scan of the counts into offsets, a fill.
 * Mode DRT_OVERLAP_ANY (1): the traversal ends at the first listed triangle, and counts[i] is 0 or 1.  prims must be NULL and
 * prims_capacity 0; offsets is not read; counts NULL is DRT_ERR_INVALID.
 * A result depends on the box, the scene, cap_i and the mode only.  An empty scene lists nothing.
 * What this is not: box-versus-box (the other side is always the mesh's triangles); clipped polygons (a triangle is listed whole, by
 * index); a large-list structure -- the insert is the one-record-per-step insert of drt_renderer_list_hits, so the cost of a triangle
 * that arrives out of order grows with the capacity, and a box that lists thousands is better counted than stored.
 * Conventions and errors are drt_renderer_nearest_list's, checked in its order: handles are checked before n == 0, then a mode outside
 * {0, 1} is DRT_ERR_INVALID (checked first after the handles), n == 0 is a no-op, n < 2^31, all pointers are device pointers on the
 * renderer's device, boxes 16-byte aligned, offsets, prims and counts 4-byte aligned, hip_stream NULL = the renderer's stream, the
 * call only enqueues, in order with the other queries, a refitted device copy is the one queried, legal on a sharded renderer,
 * DRT_ERR_UNSUPPORTED beyond 64 levels, DRT_ERR_INVALID while an asynchronous batch is pending.  The framebuffer, accumulation, sample
 * count, counters, kernel info and kernel span are not touched. */
typedef struct drt_box { float center[3]; float half[3]; float axis[3][3]; float pad; } drt_box;       /* 64 B */
#define DRT_OVERLAP_LIST 0
#define DRT_OVERLAP_ANY  1
int           drt_renderer_overlap_boxes(drt_renderer *r, const drt_scene *scene, const drt_box *boxes, const uint32_t *offsets,
                                         int32_t *prims, uint32_t prims_capacity, uint32_t *counts, uint32_t n, int32_t mode,
                                         void *hip_stream);

/* ---- triangle overlap queries (new; the mesh triangles that each query triangle touches -- the first query about another mesh) ----
 * One query = a drt_tri: 48 bytes, 16-byte aligned, v[3][3] (the vertices q0 = v[0], q1 = v[1], q2 = v[2]) and three pad words that
 * are ignored.  A mesh is a batch of queries.
 * Everything that is not stated here is drt_renderer_overlap_boxes', word for word, with "query" for "box" and tris for boxes: the
 * modes DRT_OVERLAP_LIST and DRT_OVERLAP_ANY; the segments, the -1 fill and counts[i] as the total listed, stored or not; the NULL
 * rules and the argument checks in that order; the error codes and the stream ordering; a refitted device copy is the one queried;
 * the 64-level bound; and that the framebuffer, accumulation, sample count, counters, kernel info and kernel span are not touched.
 * All arithmetic is fp32 with one rounding per operation, in the order written.  dot and cross are as the box overlap block defines
 * them; min3(x, y, z) = fminf(fminf(x, y), z) and max3 the same with fmaxf.
 * Validity: a query is valid iff all nine coordinates satisfy fabsf(x) <= FLT_MAX.  An invalid query (a NaN or an infinity anywhere
 * in v) pushes nothing and lists nothing.  (fminf would otherwise drop a NaN vertex from the bounds, and the query would go on as
 * if the vertex were not there.)
 * Bounds, once per query: qmin[j] = min3(q0[j], q1[j], q2[j]), qmax[j] = max3(q0[j], q1[j], q2[j]).  They are exact.
 * Node cull and traversal: the box query's, unchanged -- a box (bmin, bmax) passes iff, on all three axes, qmin[j] <= bmax[j] &&
 * bmin[j] <= qmax[j], closed comparisons; the root is tested against the scene's root box; an interior node pushes each child that
 * passes, child 2 first; a leaf tests its triangles in order.  The same remark applies: the stored triangle is (v0, e1, e2), v0 + e1
 * can round one ulp outside a node box built from the real v1, and a triangle whose leaf the cull rejects is not listed, whatever the
 * triangle test would say.
 * Triangle test, on the query (q0, q1, q2) and the stored (v0, e1, e2), relative to q0:
 *   a1 = q1 - q0, a2 = q2 - q0, g = a2 - a1; h = e2 - e1; p0 = v0 - q0, p1 = p0 + e1, p2 = p0 + e2;
 *   nq = cross(a1, a2), nt = cross(e1, e2).
 * Seventeen axes L, in this order:
 *   1. nq
 *   2. nt
 *   3. cross(A, E) for A in (a1, g, a2) (outer) and E in (e1, h, e2) (inner): nine
 *   4. cross(nq, A) for A in (a1, g, a2): three
 *   5. cross(nt, E) for E in (e1, h, e2): three
 * For each axis sq = (0, dot(L, a1), dot(L, a2)) and st = (dot(L, p0), dot(L, p1), dot(L, p2)); the axis is ok iff
 * min3(st) <= max3(sq) && min3(sq) <= max3(st).  The triangle is listed iff all seventeen are ok.  Touching counts: a shared vertex
 * or a shared edge is a touch, and a triangle of the scene given as a query lists itself.  Only the predicate leaves the kernel, so
 * the kernel may evaluate the axes in any order and stop at the first failure; bit for bit means that the comparisons are made on the
 * same rounded values.
 * What the predicate is.  For two triangles of non-zero area it is, in real arithmetic, the exact intersection test of the two
 * closed sets: the standard 11 axes (the two normals and the nine cross products of edges) decide the skew case, and the six
 * in-plane edge normals (groups 4 and 5) decide the coplanar case, where the nine cross products vanish and pass with 0 <= 0.  For a
 * zero-area triangle on either side (a segment or a point) it is conservative: it never misses, and it may list a near miss in the
 * triangle's own plane.  In fp32 the products reach the fourth power of the coordinate differences.  Where that overflows, the
 * projections are infinities and NaNs, a comparison on a NaN fails and the pair is not listed.  (fminf / fmaxf drop a NaN beside a
 * finite projection, so the header promises no more about such a pair than that the call completes.)  Below that range the rounded
 * predicate can differ from the real one only for pairs within rounding of touching.
 * What this is not: the intersection segment is not returned -- no clipping, no contour; there is no pair exclusion at this level --
 * the neighbours of a query taken from the same mesh are listed, because they touch; and it is not a large-list structure -- the
 * insert is the one-record-per-step insert of drt_renderer_list_hits.
 * tris is 16-byte aligned; offsets, prims and counts 4-byte aligned. */
typedef struct drt_tri { float v[3][3]; float pad[3]; } drt_tri;                                        /* 48 B */
int           drt_renderer_overlap_triangles(drt_renderer *r, const drt_scene *scene, const drt_tri *tris, const uint32_t *offsets,
                                             int32_t *prims, uint32_t prims_capacity, uint32_t *counts, uint32_t n, int32_t mode,
                                             void *hip_stream);

/* ---- plane sections (new; the segments where each plane cuts the mesh -- the first query that returns the geometry of a cut) ----
 * One query = a drt_plane: 16 bytes, 16-byte aligned, n[3] and d.  It is the set dot(n, x) = d.  n is used as given and is not
 * normalised.  Slicing a mesh is a batch of parallel planes.
 * Everything that is not stated here is drt_renderer_overlap_boxes', word for word, with "plane" for "box", planes for boxes and out
 * for prims: the NULL rules and the argument checks in that order; the error codes and the stream ordering; a refitted device copy is
 * the one queried; the 64-level bound; and that the framebuffer, accumulation, sample count, counters, kernel info and kernel span are
 * not touched.
 * All arithmetic is fp32 with one rounding per operation, in the order written.  dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z and cross
 * are as the box overlap block defines them.  Alpha cut-outs are ignored (a geometric query).
 * Validity: a plane is valid iff all four words satisfy fabsf(x) <= FLT_MAX.  An invalid plane (a NaN or an infinity in n or d) pushes
 * nothing and lists nothing.  n = 0 is valid and cuts nothing.
 * Signed value: s(x) = dot(n, x) - d.  A vertex is above iff s >= 0 (closed), otherwise below.  (-0.0 is above.)
 * Node cull: per axis, cmin[j] = n[j] >= 0 ? bmin[j] : bmax[j] and cmax[j] is the other one.  A box (bmin, bmax) passes iff
 * s(cmin) < 0 && s(cmax) >= 0.  The root is tested against the scene's root box; an interior node keeps each child that passes, child 1
 * before child 2.  Every product and sum in s is monotone in each coordinate, and rounding is monotone, so
 * s(cmin) <= s(v) <= s(cmax) holds in fp32 for every v inside the box: the cull never drops a cut triangle whose vertices lie in the
 * box.  The known remark applies: the stored triangle is (v0, e1, e2), v0 + e1 can round one ulp outside a node box built from the
 * real v1, and a triangle whose leaf the cull rejects is not listed.
 * Triangle test, on the stored (v0, e1, e2): v1 = v0 + e1, v2 = v0 + e2; s0, s1, s2 = s(v0), s(v1), s(v2).  The triangle is cut iff
 * its three vertices are not all in the same class.  A triangle lying in the plane is all above and is not cut.
 * Segment: exactly one vertex k is alone in its class: the apex.  cut(a, b): let lo be the below one of the two and hi the above one;
 * t = s_lo / (s_lo - s_hi), and the point is lo + (hi - lo) * t per component.  The canonical below-to-above direction makes the point
 * of a shared edge depend on that edge's two vertices only.  P = cut(k, k+1) and Q = cut(k, k+2), indices mod 3.  Apex above: the
 * segment is P -> Q.  Apex below: it is Q -> P.  So dot(q - p, cross(n, fn)) >= 0 with fn = cross(e1, e2): on a closed mesh with
 * outward faces the contours run counter-clockwise seen from the side n points to, and 0.5 * sum dot(n / |n|, cross(p, q)) is the
 * positive section area.  code = k + 4 * (apex above).  A vertex exactly on the plane is above; an apex on the plane with the other
 * two below gives a zero-length segment, and it is listed.
 * Record: a drt_section, 32 bytes: p[3], prim, q[3], code.  The miss record is all zeros with prim = -1.
 * List: ascending triangle index.  Each triangle lies in one leaf and the cull never changes during a query, so the set of records
 * does not depend on the traversal order.
 * Mode DRT_SECTION_LIST (0): offsets / out / out_capacity / counts are exactly drt_renderer_overlap_boxes' segments, with 32-byte
 * records in place of int32: offsets holds n + 1 uint32 values; plane i owns out[offsets[i] .. offsets[i+1]).  Its capacity is
 * cap_i = offsets[i+1] > offsets[i] ? offsets[i+1] - offsets[i] : 0, then clamped so that offsets[i] + cap_i <= out_capacity
 * (offsets[i] >= out_capacity gives 0).  The call writes out[offsets[i] + j] for j < cap_i and nothing else in out.  The first cap_i
 * records of the list are stored; the rest of the cap_i slots hold the miss record.  counts[i] is the total, stored or not.  out is
 * NULL iff out_capacity == 0: a pure count.  counts may be NULL; both out and counts NULL is DRT_ERR_INVALID.  Two passes give every
 * segment of every plane without a capacity guess: a count with capacity 0, an exclusive scan of the counts into offsets, a fill.
 * Mode DRT_SECTION_ANY (1): the work ends at the first cut triangle found, and counts[i] is 0 or 1.  (An implementation may finish
 * the group of leaves it is testing before it stops; counts[i] is the same.)  out must be NULL and out_capacity 0; offsets is not
 * read; counts NULL is DRT_ERR_INVALID.
 * A result depends on the plane, the scene, cap_i and the mode only.  An empty scene lists nothing.
 * The lists are ascending because the builder splits a range [first, last) into [first, mid) and [mid, last): the leaves, child 1
 * first, hold ascending triangle ranges.  The library checks that when it packs a scene and returns DRT_ERR_UNSUPPORTED for a tree
 * where it is false, instead of handing out an unsorted list.
 * What this is not: no chaining into loops -- the records of a plane are separate segments in triangle order; endpoints of neighbouring
 * triangles agree only as far as their stored vertices do (v0 + e1 of one against v0' + e2' of the other), so a caller welds with a
 * tolerance; no caps or filled polygons; alpha cut-outs are ignored; and it is not built for millions of planes with near-empty lists
 * -- it works there, one wave each.
 * planes and out are 16-byte aligned; offsets and counts 4-byte aligned. */
typedef struct drt_plane { float n[3]; float d; } drt_plane;                                            /* 16 B */
typedef struct drt_section { float p[3]; int32_t prim; float q[3]; int32_t code; } drt_section;         /* 32 B */
#define DRT_SECTION_LIST 0
#define DRT_SECTION_ANY  1
int           drt_renderer_plane_sections(drt_renderer *r, const drt_scene *scene, const drt_plane *planes, const uint32_t *offsets,
                                          drt_section *out, uint32_t out_capacity, uint32_t *counts, uint32_t n, int32_t mode,
                                          void *hip_stream);

/* ---- section contours (new; a plane's segments chained into open polylines and closed loops, by integers only) ----
 * The records of a plane are separate segments in triangle order.  prim and code of a record say which two edges of which triangle
 * the segment enters and leaves through, so with a table of the mesh's edge adjacency the successor of a segment is an integer
 * question: no coordinate is compared, no tolerance is chosen, and nothing is welded.
 * Edge adjacency, drt_scene_edge_adjacency: out receives 3 * n_triangles host values; capacity is the room in values.  Half-edge
 * h = 3 * t + e, with t in tree order (the index every query reports) and e in {0, 1, 2}, runs from vertex e to vertex (e + 1) % 3
 * of the positions the host scene holds (drt_scene_get_triangles; not the packed v0 + e1).  Two positions are the same iff their
 * three words are bit-equal (-0.0 is not +0.0).  The half-edges are grouped by their unordered pair of endpoint positions.  A group
 * of exactly two half-edges that run in opposite directions is a pair of twins: adj[h] = h' and adj[h'] = h.  A group of one is a
 * boundary edge: adj[h] = -1.  Everything else is -2: three or more half-edges, two that run the same way, and an edge whose two
 * ends are the same position.  DRT_ERR_INVALID: a NULL scene, capacity below 3 * n_triangles, no BVH (the table is in tree order).
 * A renderer keeps a device copy of the table beside its copy of the scene: made by the first drt_renderer_chain_sections after an
 * upload, dropped with that upload.  After a device-only drt_renderer_refit the table is still the host scene's: a refit keeps the
 * triangle order, and a deformation keeps shared positions shared.
 * drt_renderer_chain_sections: segs, splits, slots and chains are device pointers on the renderer's device; the call is enqueued on
 * hip_stream (NULL = the renderer's) and orders with the other queries as they do.
 * Inputs: splits holds n + 1 values; plane i owns segs[splits[i] .. splits[i+1]) and slots[splits[i] .. splits[i+1]).  The range
 * is clamped as drt_renderer_plane_sections clamps cap_i: a decreasing pair is an empty range, and nothing beyond total is read or
 * written.  A range is what a fill wrote: records in ascending prim, followed by any miss records (prim < 0).  Unsorted input gives
 * unspecified links, but the call completes and every index it writes is inside the plane's own range.  Records outside every
 * range belong to no chain and their slots are not written.
 * Link: for a record j, k = code & 3 and up = code >> 2.  It is entered through edge in_j = up ? k : (k + 2) % 3 and left
 * through edge out_j = up ? (k + 2) % 3 : k (P lies on edge k, Q lies on edge (k + 2) % 3, and the segment runs P -> Q iff the
 * apex is above).  Let a = adj[3 * prim_j + out_j].  succ(j) = m iff a >= 0, m is the record of the same plane with
 * prim_m == a / 3 (found by binary search in the ascending prefix), and 3 * prim_m + in_m == a.  Otherwise j has no successor and
 * its exit status says why: 1 = boundary edge (a == -1), 2 = non-manifold or flipped (a == -2), 3 = the neighbour is not in the
 * list, 4 = the neighbour is cut through other edges, 5 = j is a miss record.  0 = linked.  adj pairs half-edges one to one, so
 * succ is injective: every record has at most one predecessor, and the components are simple paths and simple cycles.
 * Canonical order: a path starts at its record without a predecessor; a cycle starts at its record of smallest index, and is
 * closed.  The chains of a plane are ordered by the ascending index of their first record.  Miss records stay where they are, after
 * all chains.  Position pos runs over the plane's range in that order, and slots[pos] holds: seg = the index into segs of the
 * record that stands there; first = the position of its chain's first record; length = its chain's length; flags: bit 0 = the
 * chain is closed, bits 1..3 = that record's exit status.  A miss record is {own index, own position, 1, 5 << 1}.
 * chains[2 * i] is the number of chains of plane i, misses not counted; chains[2 * i + 1] is how many of them are closed.  chains
 * may be NULL.  The result depends on segs, splits and the adjacency only.
 * What it is not: no welding and no new points -- a contour's vertices are the p of its records, plus the last q of an open
 * chain; a contour is closed exactly where neighbouring triangles agree on which of their shared vertices are above the plane, and
 * statuses 3 and 4 mark the places where they do not; no caps or filled polygons; no RendererGroup; nothing on the command line.
 * Checks, in drt_renderer_plane_sections' order: NULL r or scene; n == 0 or total == 0 is DRT_OK with no launch; NULL segs, splits
 * or slots; segs and slots 16-byte aligned, splits and chains 4-byte aligned; n < 2^31 and total < 2^31; no pending asynchronous
 * batch; device memory on the renderer's device; the scene's upload (DRT_ERR_UNSUPPORTED beyond 64 levels).  All DRT_ERR_INVALID
 * but the last.  The framebuffer, accumulation, sample count, counters, kernel info and kernel span are not touched. */
typedef struct drt_chain_slot { uint32_t seg; uint32_t first; uint32_t length; uint32_t flags; } drt_chain_slot;   /* 16 B */
int           drt_scene_edge_adjacency(const drt_scene *scene, int32_t *out, uint32_t capacity);
int           drt_renderer_chain_sections(drt_renderer *r, const drt_scene *scene, const drt_section *segs, const uint32_t *splits,
                                          drt_chain_slot *slots, uint32_t *chains, uint32_t n, uint32_t total, void *hip_stream);

/* ---- mesh topology (new; shells, boundary loops, per-triangle area and volume terms) ----
 * How many pieces a mesh is, which triangle belongs to which, whether a piece is watertight, where its holes are, and what area and
 * volume it has.  Everything is in tree order, the order of drt_scene_get_triangles and of drt_scene_edge_adjacency
 * (drt_scene_get_triangle_order maps it to load order), and adj is the table of drt_scene_edge_adjacency, exactly as it stands: the
 * labels and the loops are a property of that table alone, and any correct method gives the same bytes.
 * Shells: triangles t and t' are joined iff adj[3 * t + e] >= 0 and adj[3 * t + e] / 3 == t' for some e: a pair of twins.  A
 * boundary edge (-1) and a non-manifold, flipped or zero-length edge (-2) join nothing: the three leaves of a book are three shells, and
 * triangles that share only a vertex are separate shells.  label[t] is the smallest triangle index of t's connected component.
 * counts = {shells, open half-edges, bad half-edges}: the triangles with label[t] == t, the half-edges with adj == -1 and those
 * with adj == -2.  Per shell, open_edges[s] and bad_edges[s] count the same over the half-edges of its triangles, and a shell is
 * watertight iff both are zero.
 * Boundary loops: the records are the half-edges h = 3 * t + e with adj[h] == -1, in ascending h.  Half-edge h runs from vertex e
 * to vertex b = (e + 1) % 3 of t.  Its successor is found by rotating about b through the adjacency; no coordinate is read.  Start
 * with g = 3 * t + (e + 1) % 3.  While adj[g] >= 0: g' = adj[g], t' = g' / 3, e' = g' % 3, g = 3 * t' + (e' + 1) % 3.  If
 * adj[g] == -1 then succ(h) = g.  If adj[g] == -2 the record has no successor and its exit status is 2; the statuses are the section
 * contours': 0 = linked, 2 = non-manifold or flipped.  The walk ends: twins pair half-edges one to one, so the half-edges around b
 * that the steps visit form a path of degree at most 2, the walk starts at an end of it and cannot cycle, and it ends within the
 * valence of b.  An implementation still carries a step guard of 3 * n_triangles and treats its expiry as status 2.  succ is
 * injective, so the components are simple paths and simple cycles.  Canonical order, the contours' rule: a path starts at its record
 * without a predecessor; a cycle starts at its smallest h, and is closed; the loops are ordered by their first record.  All
 * half-edges of a loop lie in one shell: a loop carries that shell's label.
 * Position pos runs over the records in that order, and slots[pos] holds: half_edge = the h that stands there; first = the position
 * of its loop's first record; length = its loop's length; flags: bit 0 = the loop is closed, bits 1..3 = that record's exit status.
 * counts = {records, loops, closed loops}.  slots[pos] is written for pos < capacity and nothing else is: a too small capacity
 * truncates, and counts still holds the true numbers.  slots is NULL iff capacity == 0: a pure count.
 * Measure terms: one 32-byte record per triangle, computed from the device's packed (v0, e1, e2) -- after a device-only
 * drt_renderer_refit these are the refitted positions.  With v0, e1, e2 converted to float64: c = cross(e1, e2), each component as
 * a * b - c * d (c.x = e1.y e2.z - e1.z e2.y, c.y = e1.z e2.x - e1.x e2.z, c.z = e1.x e2.y - e1.y e2.x), and
 * w = (v0.x * c.x + v0.y * c.y) + v0.z * c.z.  Every product and sum is rounded on its own, no contraction, no square root.  The
 * record is {c.x, c.y, c.z, w}.  dot(v0, cross(v0 + e1, v0 + e2)) == dot(v0, cross(e1, e2)) in exact arithmetic, so w / 6 summed
 * over a shell is its signed volume, |c| / 2 is a triangle's area, and sum c / 2 is near zero for a watertight shell.
 * The calls: labels (n_triangles int32), counts, slots and terms (4 float64 per triangle) are device pointers on the renderer's
 * device; the work is enqueued on hip_stream (NULL = the renderer's) and orders with the other queries as they do.  The labels, the
 * counts and the list of records depend on adj only: a renderer makes them with the first call after a scene upload (that call
 * waits for the stream while it labels), keeps them beside its copy of adj across device refits, and drops them with that upload.
 * drt_renderer_edge_adjacency copies the renderer's device copy of adj (3 * n_triangles int32) to a device array, for work on
 * the table that stays on the device.  drt_renderer_topology_steps: out receives 3 host values about that labelling: the steps enqueued, those that did something and
 * those that hooked.
 * What it is not: no joining across non-manifold edges or by shared vertices; no Euler characteristic, genus or vertex welding; no
 * orientation repair; the other queries are not filtered by shell; no RendererGroup; nothing on the command line.
 * Checks, in drt_renderer_chain_sections' order: NULL r or scene; NULL labels, counts of drt_renderer_boundary_loops or terms (the
 * counts of drt_renderer_shell_labels may be NULL), slots NULL with a capacity or not NULL without one; labels and counts 4-byte
 * aligned, slots and terms 16-byte aligned; capacity < 2^31; no pending asynchronous batch; device memory on the renderer's device;
 * the scene's upload (DRT_ERR_UNSUPPORTED beyond 64 levels); no BVH as drt_scene_edge_adjacency.  All DRT_ERR_INVALID but the upload's.
 * DRT_ERR_DEVICE if the labelling does not settle within its bound on steps.  A scene without triangles is DRT_OK with zero counts.
 * The framebuffer, accumulation, sample count, counters, kernel info and kernel span are not touched. */
typedef struct drt_loop_slot { uint32_t half_edge; uint32_t first; uint32_t length; uint32_t flags; } drt_loop_slot;   /* 16 B */
typedef struct drt_shell_term { double c[3]; double w; } drt_shell_term;                                              /* 32 B */
int           drt_renderer_shell_labels(drt_renderer *r, const drt_scene *scene, int32_t *labels, uint32_t *counts, void *hip_stream);
int           drt_renderer_boundary_loops(drt_renderer *r, const drt_scene *scene, drt_loop_slot *slots, uint32_t capacity,
                                          uint32_t *counts, void *hip_stream);
int           drt_renderer_shell_terms(drt_renderer *r, const drt_scene *scene, double *terms, void *hip_stream);
int           drt_renderer_edge_adjacency(drt_renderer *r, const drt_scene *scene, int32_t *adj, void *hip_stream);
int           drt_renderer_topology_steps(const drt_renderer *r, uint32_t *out);

/* ---- triangle intersection segments (new; where a query mesh cuts the scene -- one oriented segment per cutting pair) ----
 * One query = a drt_tri with vertices q0, q1, q2, as for drt_renderer_overlap_triangles.  A mesh is a batch of queries, and the
 * records of a batch are the curve along which that mesh cuts the scene's surface, in pieces: one segment per pair (query, scene
 * triangle) that cut each other.
 * Stored scene triangle (v0, e1, e2), with world vertices w0 = v0, w1 = v0 + e1, w2 = v0 + e2.
 * All arithmetic is fp32 with one rounding per operation, in the order written.  dot, cross and min3 / max3 are as the box-overlap
 * block defines them.  Alpha cut-outs are ignored (a geometric query).
 * Validity, bounds, cull and traversal are drt_renderer_overlap_triangles', word for word: a query is valid iff all nine coordinates
 * satisfy fabsf(x) <= FLT_MAX, and an invalid query pushes nothing and lists nothing; qmin[j] = min3(q0[j], q1[j], q2[j]),
 * qmax[j] = max3(q0[j], q1[j], q2[j]), exact; a box (bmin, bmax) passes iff, on all three axes, qmin[j] <= bmax[j] &&
 * bmin[j] <= qmax[j], closed comparisons; the root is tested against the scene's root box; an interior node pushes each child that
 * passes, child 2 first; a leaf's triangles are tested in order.  The known remark applies: v0 + e1 can round one ulp outside a node
 * box built from the real v1, and a triangle whose leaf the cull rejects gives no record.
 * Signed values.  The scene triangle against the query's plane: a1 = q1 - q0, a2 = q2 - q0, nq = cross(a1, a2); p_k = w_k - q0,
 * s_k = dot(nq, p_k) for k = 0, 1, 2; vertex k is above iff s_k >= 0, otherwise below; all three in one class: no record.  The query
 * against the scene triangle's plane: nt = cross(e1, e2); r_k = q_k - v0, u_k = dot(nt, r_k); above iff u_k >= 0; all three in one
 * class: no record.  p_k and r_k are taken from the world vertex itself, not built as p_0 + e1: the s of a vertex that two scene
 * triangles share depends on that vertex and the query alone.
 * A coplanar pair, and a zero-area triangle on either side, are therefore all above and give no record: this is stricter than
 * drt_renderer_overlap_triangles' predicate, which lists coplanar pairs that touch and is conservative for zero-area triangles.
 * Line direction: D = cross(nq, nt).  Axis choice: j = 0; if (fabsf(D[1]) > fabsf(D[0])) j = 1; if (fabsf(D[2]) > fabsf(D[j])) j = 2.
 * If !(fabsf(D[j]) > 0): no record.
 * Cut points use drt_renderer_plane_sections' cut(a, b): lo is the below vertex of the two and hi the above one,
 * t = s_lo / (s_lo - s_hi), and the point is lo + (hi - lo) * t per component, on the world vertices.  For the scene triangle, with
 * apex k (the vertex alone in its class): T1 = cut(k, k+1) lies on edge k and T2 = cut(k, k+2) lies on edge (k+2) % 3, indices mod 3;
 * edge e runs from vertex e to vertex (e+1) % 3, as drt_scene_edge_adjacency has it.  For the query Q1 and Q2 are built the same
 * way from q_k and u_k.
 * Intervals on axis j: (tl, th) = (T1, T2) if T1[j] <= T2[j], else (T2, T1); (ql, qh) likewise from Q1, Q2.
 * lo = ql if ql[j] > tl[j] else tl; hi = qh if qh[j] < th[j] else th: on a tie the scene's point is kept.  A record exists iff
 * lo[j] <= hi[j]: touching counts, and a zero-length segment is listed; a NaN fails, and the pair is not listed.
 * Orientation: if D[j] > 0 then p = lo and q = hi, otherwise p = hi and q = lo.  So the segment runs along cross(nq, nt).
 * Record: a drt_isect, 32 bytes, 16-byte aligned: p[3], prim, q[3], code.  prim is the scene triangle.  code = cp + 16 * cq, where
 * an endpoint's code is the scene triangle's edge (0..2) for a point of T, or 4 + the query's edge for a point of Q.  The miss record
 * is all zeros with prim = -1.
 * Endpoints are never interpolated along the line: each one is one of the four cut points, so an endpoint on a shared edge is the
 * same bits from both neighbours wherever their stored vertices agree.
 * List: ascending triangle index, at most one record per pair.  Segments, capacities, the miss fill, counts[i] as the total, the NULL
 * rules and the two-pass recipe are drt_renderer_plane_sections' in mode LIST, with tris for planes; there is no mode argument:
 * offsets holds n + 1 uint32 values; query i owns out[offsets[i] .. offsets[i+1]); cap_i = offsets[i+1] > offsets[i] ?
 * offsets[i+1] - offsets[i] : 0, then clamped so that offsets[i] + cap_i <= out_capacity; the call writes out[offsets[i] + j] for
 * j < cap_i and nothing else in out; the first cap_i records of the list are stored and the rest of the cap_i slots hold the miss
 * record; counts[i] is the total, stored or not; out is NULL iff out_capacity == 0: a pure count; counts may be NULL; both NULL is
 * DRT_ERR_INVALID; a count with capacity 0, an exclusive scan of the counts into offsets, a fill.  As there, the call returns
 * DRT_ERR_UNSUPPORTED for a tree whose leaves, child 1 first, do not hold ascending triangle ranges: the list is appended to and
 * never inserted into.  The checks, the error codes, the stream ordering, the refitted device copy, the 64-level bound and the
 * untouched framebuffer, accumulation, sample count, counters, kernel info and kernel span are drt_renderer_plane_sections' too.
 * What the rule is.  In real arithmetic, for non-coplanar triangles of non-zero area, a record exists iff the two closed triangles
 * meet.  In fp32 the set of pairs with a record can differ from drt_renderer_overlap_triangles' list only for pairs within rounding
 * of touching.
 * Scale.  D is a fourth power of coordinate differences.  Scaling a mesh and its queries by a power of two changes no record (p and q
 * scaled, prim and code the same) for 2^-24 to 2^32, measured in steps of 2^2 on the mesh and the triangle queries the working-range
 * block below was measured on (drt_renderer_overlap_triangles there: 2^-30 to 2^30; only comparisons leave that test, while here s and
 * u, third powers, are divided); beyond, s, u or D overflow or lose bits as subnormals and records vanish or move
 * (tests/test_intersect_ref.py asserts the figure).
 * What this is not: the segments are not chained into curves -- the records of a query are separate segments in triangle order, and
 * joining them across queries and triangles is the caller's; no clipped polygons and no boolean; coplanar overlaps give nothing; there
 * is no pair exclusion at this level -- for a query taken from the scene itself the s of a shared vertex is a rounding error of
 * either sign, so a neighbour can give a record along the shared edge, and a caller filters such pairs; and it is not built for queries that cut tens of thousands of triangles each -- it
 * works there, one lane per query.
 * tris and out are 16-byte aligned; offsets and counts 4-byte aligned. */
typedef struct drt_isect { float p[3]; int32_t prim; float q[3]; int32_t code; } drt_isect;             /* 32 B */
int           drt_renderer_intersect_triangles(drt_renderer *r, const drt_scene *scene, const drt_tri *tris, const uint32_t *offsets,
                                               drt_isect *out, uint32_t out_capacity, uint32_t *counts, uint32_t n, void *hip_stream);

/* ---- sphere casts (new; the first contact of a moving sphere with the mesh) ----
 * One cast = a drt_ray (org o, tmin, dir d, tmax, read as drt_renderer_trace_rays reads it: dir as given, t in units of |d|,
 * inv_dir = 1/dir) and a radius r.  The sphere's centre at parameter t is o + d t; the answer is the smallest t in [tmin, tmax) at
 * which the sphere touches a triangle, with that triangle, the contact point on it and the feature touched.  r = 0 is a ray with a
 * closed start (a centre that starts on the surface hits at tmin).
 * All arithmetic is fp32 with one rounding per operation, in the order written; dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z, / is the
 * correctly rounded division and sqrt the correctly rounded square root.  A NaN fails every test.
 * The sphere touches a triangle where its centre enters the triangle's offset volume: the union of seven convex shapes, a prism over
 * the face, a cylinder round each edge and a sphere at each vertex.  The shapes overlap on purpose: every edge cylinder is a whole
 * cylinder and every vertex sphere a whole sphere, and no shape's test is restricted to its Voronoi region.  A centre that misses the
 * prism's face by a rounding error enters the neighbouring cylinder an instant later; nothing slips through a seam.
 * Per cast: s = o + d tmin (the start centre), dd = dot(d, d), r2 = r r.  Every entry time is tau >= 0, measured from s; a
 * candidate's t = tmin + tau.
 * Per triangle k: (v0, e1, e2) as drt_renderer_nearest reads them (the stored edges).  d11 = dot(e1, e1), d22 = dot(e2, e2),
 * d12 = dot(e1, e2); the vertices p0 = v0, p1 = v0 + e1, p2 = v0 + e2 and, for j = 0, 1, 2, mj = s - pj, bj = dot(mj, d),
 * cj = dot(mj, mj) - r2.  The triangle's candidate starts as t = +inf, feature -1; the seven shapes are taken in feature order and
 * a later one replaces an earlier one only on a strict <.
 *   Face (feature 0).  n = cross(e1, e2), k = r sqrt(dot(n, n)), h = dot(n, m0), dn = dot(n, d).  Containment branch: |h| <= k, the
 *     centre starts inside the slab, tau = 0.  Otherwise the sphere must approach, (h > 0 && dn < 0) || (h < 0 && dn > 0), and
 *     tau = (|h| - k) / |dn|.  The centre at tau, q = m0 + d tau, is projected onto the plane and must lie in the triangle:
 *     q1 = dot(q, e1), q2 = dot(q, e2), nu = d22 q1 - d12 q2, nv = d11 q2 - d12 q1, den = d11 d22 - d12 d12, accepted iff
 *     den > 0 && nu >= 0 && nv >= 0 && nu + nv <= den.  A zero-area triangle (den <= 0) has no face candidate; its edges and
 *     vertices still count.
 *   Edges (features 1, 2, 3).  (a, e, m, md, c, ee) = (p0, e1, m0, b0, c0, d11), (p0, e2, m0, b0, c0, d22) and, with e3 = e2 - e1,
 *     (p1, e3, m1, b1, c1, dot(e3, e3)).  me = dot(m, e), de = dot(d, e), Cq = ee c - me me.  Containment branch: Cq <= 0, the centre
 *     starts inside the infinite cylinder, tau = 0.  Otherwise x = cross(d, e), det = dot(m, x), A = dot(x, x), B = ee md - de me;
 *     require A > 0 && B < 0 and disc = ee (A r2 - det det) >= 0; then tau = Cq / (sqrt(disc) - B).  Accepted iff the axial
 *     coordinate ax = me + tau de satisfies ee > 0 && ax >= 0 && ax <= ee (an edge of length zero is its two vertices).
 *   Vertices (features 4, 5, 6).  (m, b, c) = (m0, b0, c0), (m1, b1, c1), (m2, b2, c2).  Containment branch: c <= 0, tau = 0.
 *     Otherwise require dd > 0 && b < 0 and, with x = cross(m, d), disc = dd r2 - dot(x, x) >= 0; then tau = c / (sqrt(disc) - b).
 * These are the quadratics A tau^2 + 2 B tau + Cq = 0 (A = ee dd - de de) and dd tau^2 + 2 b tau + c = 0 with both cancellations
 * taken out.  The discriminants B B - A Cq and b b - dd c are differences of two numbers that grow with the square of the start's
 * distance and differ by a term of the radius' size; by Lagrange's identity they equal ee (|d x e|^2 r2 - (m . (d x e))^2) and
 * dd r2 - |m x d|^2, whose rounding error grows with the distance only.  tau = Cq / (sqrt(disc) - B) is the smaller root
 * (-B - sqrt(disc)) / A with numerator and denominator multiplied by -B + sqrt(disc): Cq > 0 and sqrt(disc) - B > 0, so every entry
 * time is 0 (a containment branch) or a quotient of two positive numbers.  A sphere resting at distance r (1 +- eps) from a surface
 * and pushed into it gets tau = 0 or a small positive tau, never a slightly negative root that is thrown away; there is no separate
 * start-overlap test.  A tau = 0 found by a containment branch adds 8 to the feature (8 = face, 9..11 = edges, 12..14 = vertices):
 * the sphere overlapped the triangle at tmin.
 * Across triangles: a triangle's candidate (t, k) replaces the result iff t < best || (t == best && k < prim); best starts as tmax
 * with prim = -1, so a candidate is valid iff t < tmax, and the answer does not depend on the tree.
 * Traversal: a node's box is inflated by r on every side and slab-tested: per axis t0 = ((bmin - r) - o) inv_dir,
 * t1 = ((bmax + r) - o) inv_dir, enter = the largest of fminf(t0, t1), exit = the smallest of fmaxf(t1, t0) (a NaN operand, 0 * inf,
 * is dropped).  A node is visited iff enter <= exit && exit >= tmin && enter <= best.  The root is pushed iff it passes, r >= 0 and no
 * component of o or d is NaN (a NaN tmin or tmax fails the test by itself), so such a cast visits nothing; a popped
 * entry is dropped unless its enter <= best still holds; a leaf tests its triangles in order; an interior node pushes each child that
 * passes, the farther one first (enter1 > enter2 -> child 1): drt_renderer_trace_rays' stack discipline and its 64-level limit.
 * (The fp32 slab test culls as it does for the ray queries: a contact whose inflated box the test misses by a rounding is not found.)
 * A zero direction gives the static overlap test that the containment branches are: inv_dir is +-inf, a box that contains o after
 * inflation has enter = -inf and exit = +inf and is visited, no entry branch can pass (dn = 0, A = 0, dd = 0), so the result is the
 * lowest-numbered triangle that the sphere at o overlaps, with t = tmin, or a miss.
 * Result: one drt_sweep_hit {t, prim, u, v, point, feature}.  (u, v) and the point are computed once, after the traversal, from the
 * winning (prim, feature, t): cc = o + d t, q = cc - v0, and by feature & 7
 *   0: (nu / den, nv / den) with q1, q2, nu, nv, den as in the face test;   1: (w, 0), w = fminf(fmaxf(dot(q, e1) / d11, 0), 1);
 *   2: (0, w), w = fminf(fmaxf(dot(q, e2) / d22, 0), 1);   3: (1 - w, w), w = fminf(fmaxf(dot(q - e1, e3) / dot(e3, e3), 0), 1);
 *   4: (0, 0);   5: (1, 0);   6: (0, 1);
 * point = (v0 + e1 u) + e2 v.  The contact normal is (o + d t) - point; the caller can form it.  For a containment feature the point
 * is where the shape's axis is nearest the start centre, not the deepest point of the overlap.
 * A miss -- nothing touched in [tmin, tmax), a negative or NaN radius, a NaN ray, an empty scene -- is {tmax, -1, 0, 0, 0, 0, 0, -1},
 * tmax being the ray's own word.  A result depends on its cast and the scene only.
 * What this is not: alpha cut-outs are ignored (a geometric query); capsules, boxes and rotating bodies are out of scope, as is the
 * penetration depth of a sphere that starts in overlap.
 * Conventions and errors are drt_renderer_nearest's, checked in its order: device pointers on the renderer's device, rays and results
 * 16-byte aligned, radii a float[n] 4-byte aligned, n < 2^31, n == 0 is a no-op, hip_stream NULL = the renderer's stream, the call only
 * enqueues, in order with the other queries (the same event), the scene is uploaded as for rendering and a refitted device copy
 * (drt_renderer_refit) is the one queried.  Legal on a sharded renderer.  DRT_ERR_UNSUPPORTED beyond 64 levels, DRT_ERR_INVALID while
 * an asynchronous batch is pending.  The framebuffer, accumulation, sample count, counters, kernel info and kernel span are not
 * touched. */
typedef struct drt_sweep_hit { float t; int32_t prim; float u, v; float point[3]; int32_t feature; } drt_sweep_hit;   /* 32 B */
int           drt_renderer_sphere_cast(drt_renderer *r, const drt_scene *scene, const drt_ray *rays, const float *radii, drt_sweep_hit *out,
                                       uint32_t n, void *hip_stream);

/* ---- working range of the mesh queries (what the rules above assume of the scale of a mesh; no rule is changed here) ----
 * Scaling a mesh and its queries by a power of two changes nothing while every intermediate value stays a normal fp32 number: every
 * product and sum is the plain one with another exponent, so every field of every answer is the plain answer scaled, bit for bit, and
 * every index, count, u, v and (with the direction scaled too) t is the same.  The ranges below were measured in steps of 2^2 on a mesh
 * with edges of 2^-2 to 2^4 and queries up to 2^7 from it, zero-area triangles, slivers and needles included
 * (tests/test_hostile_meshes_ref.py asserts these figures); a mesh that far from the origin, at (4096, -8192, 16384), keeps the
 * nearest distance within one unit of 2^-23 times its largest coordinate.
 * The ray family -- drt_renderer_trace_rays, _occluded, _crossings, _inside, the sign of _signed_distance, _list_hits -- inherits two
 * ABSOLUTE constants of the renderer's triangle test, in scene units: a triangle with |det| < 1e-6 is dropped, det = dot(e1, cross(dir,
 * e2)), and a hit counts only if t > 1e-6.  det is the product of two edge lengths and |dir|, so with a unit direction triangles with
 * edges of about 1e-3 and below disappear: a millimetre tessellation of a mesh kept in metres.  drt_renderer_inside and
 * drt_renderer_signed_distance always cast the fixed unit directions D0, D1, D2: on such a mesh crossings are lost one by one, every
 * lost crossing turns a parity vote, and once all are lost every point is called outside, silently.  On the test mesh, with the
 * directions scaled as well (det is then a third power), the first crossing is lost at 2^-4 and the first vote changes there too; at
 * 2^-20 every count is 0, every vote is 0 and drt_renderer_trace_rays misses.  Going up nothing is lost, but grazing triangles that
 * were below 1e-6 come back, and a vote can change.  Rescale such a mesh before it is loaded.
 * drt_renderer_nearest, _nearest_list: vc, vb, va are products of four lengths (two edges and two offsets of the query), and
 * den = 1 / ((va + vb) + vc).  They keep their digits while those products stay normal numbers, 2^-126 to 2^128: lengths of about 2^-31
 * to 2^32 when all four are alike, less where a query lies close to a short edge.  Measured: unchanged for 2^-22 to 2^30; beyond, the
 * products overflow to infinities and NaNs or lose bits as subnormals, and answers go wrong (a NaN dist2 never wins, so triangles
 * vanish).
 * drt_renderer_overlap_boxes: the cross axes are third powers and only comparisons leave the test: unchanged for 2^-32 to 2^42.
 * drt_renderer_overlap_triangles: fourth powers: unchanged for 2^-30 to 2^30; beyond, pairs are no longer listed.
 * drt_renderer_triangle_distance: the point-triangle candidates are drt_renderer_nearest's fourth powers, den = a e - b b of an edge
 * pair is one too, and the predicate is drt_renderer_overlap_triangles': unchanged for 2^-30 to 2^26 on a mesh of the same kind with
 * query triangles of the same sizes (tests/test_tri_distance_ref.py asserts the figure); beyond, candidates become NaNs, which never
 * win, and pairs that touch are no longer seen to.
 * drt_renderer_triangle_cast: every det and numerator is a THIRD power of the lengths when d is scaled with the mesh (t stays), and only
 * comparisons and one quotient of two of them leave a candidate: unchanged for 2^-42 to 2^36 on a mesh of the same kind with query
 * triangles of the same sizes and motions towards and away from it (tests/test_tri_cast_ref.py asserts the figure); beyond, the
 * determinants pass through the subnormals to 0 (no candidate) or overflow to infinities and NaNs, which fail every test, and the
 * predicate's fourth powers go as drt_renderer_overlap_triangles' do: contacts and start overlaps are lost.
 * drt_renderer_sphere_cast: disc = ee (A r2 - det det) with A = |cross(d, e)|^2 is an EIGHTH power of the lengths when the direction is
 * scaled with the mesh (t stays), a sixth with a direction of fixed length: unchanged for 2^-4 to 2^10 only.  Give a large or a tiny mesh
 * directions of about unit length, or rescale it.  Apart from scale, a sliver (three vertices collinear to the last bit) has a face test
 * whose den, nu and nv are all rounding errors: where den comes out positive the face can be reported for a sphere that passes the sliver
 * at a distance of thousands of units of 2^-23 of the scene's size.  Exactly zero-area triangles have den = 0 and no face, as stated.
 * drt_renderer_plane_sections: s = dot(n, x) - d, t and the cut points are linear in the lengths; there is no such limit (unchanged at
 * 2^-40 and at 2^50), short of overflow of the coordinates themselves.
 * The four newest queries on that same mesh -- zero-area triangles, slivers, needles, duplicates and shared edges included -- with query
 * triangles and motions aimed at its thin triangles (tests/test_hostile_queries_ref.py asserts these figures; the ranges above for
 * the triangle distance and the triangle cast were measured on a well-behaved mesh of the same size):
 * the triangle distance is unchanged for 2^-22 to 2^28, the triangle cast with d scaled along for 2^-32 to 2^32, so 2^20 and 2^-20 change
 * no field of either.  Against float64 over all triangles the distance stays within 0.55 units of 2^-23 times the largest coordinate,
 * and a contact of the cast within 0.40 (0.21 on the scene's slivers and needles) for proper query triangles.  Where the QUERY is
 * itself a sliver or a needle every determinant and numerator of a candidate is a rounding error and a candidate can pass with
 * tau = 0: a copy of a thin triangle, held tenths of a scene unit off and cast back at it, is reported in contact at t = 0.  A duplicate
 * pair is an exact tie and goes to the smaller prim in both.
 * The conservative predicate above reaches both queries: a segment or point QUERY has d2 = 0 and t = 0 (feature bit 16) against a
 * POINT of the scene wherever it is, and is reported so exactly where the traversal comes by that point's leaf (of 54 segment queries
 * all 54 over all triangles, 12 from the tree); tests/test_gpu_hostile_queries.py holds the kernels to the tree's answer for 128
 * zero-area query triangles and about 100 zero-area casts on every mesh.  At coordinates of
 * 16384 the predicate's sums cancel, and 6 of 711 proper casts are not separated from a far zero-area triangle over all triangles, which
 * the traversal never reaches.
 * The surface weights: a = |cross(e1, e2)| is a second power of the lengths and a a, under the square root, a fourth.  The table is
 * relative to the largest area and is unchanged for 2^-22 to 2^32; below, the squares of the smallest areas (slivers, needles) go
 * subnormal and then to 0, above, the largest overflow to infinity, which counts as 0.  Of the 360 triangles 26 weigh 0 as loaded (the 24
 * of zero area and two slivers whose fp32 area is exactly 0), 331 at 2^-36 and 220 at 2^34 -- the rest still sample, and no sample lands
 * on a triangle of weight 0 -- and all at 2^-40 and 2^50, where the total is 0 and every sample is the miss record.  amax is the
 * square root of a float32 and is 0 or at least 2^-75: it is never subnormal.  The lookup is linear: position = (v0 + u e1) + v e2 keeps
 * its bits at any scale a float32 holds, and at coordinates of 16384 it is rounded to 2^-9; the stored face normal of a zero-area
 * triangle is a NaN (normalize of a zero vector) and is returned as stored.
 * drt_renderer_ambient_occlusion is of the ray family: at 2^-20 every triangle is below 1e-6 and every sample of every point is open; at
 * 2^20 grazing triangles come back (14 to 17 of 132 records differ).  At coordinates of 16384 a bias of 0.001 is half an ulp:
 * o = p + n * bias keeps p's coordinate wherever |n| bias rounds away (27 of 132 points), and the surface the point lies on can block
 * its own samples.  A point whose normal is a NaN (the lookup on a zero-area triangle) has NaN directions, which hit nothing:
 * every sample is open and bent is 0.
 * Outside these ranges every call still completes and still equals the rule as written, operation by operation, infinities, NaNs and
 * subnormals included -- tests/test_gpu_hostile_meshes.py compares the kernels there too -- but the rule no longer says anything useful.
 * (drt_renderer_overlap_triangles' predicate is conservative for zero-area triangles in a stronger sense than "a near miss in the
 * triangle's own plane": a segment or point query passes all seventeen axes against a POINT of the scene wherever it is, and only the
 * node cull keeps such a pair out of the list.) */

/* ---- intersection curves (new; the records of drt_renderer_intersect_triangles chained into closed loops and open polylines) ----
 * The records of a batch of queries are the curve along which a query mesh cuts the scene, in pieces.  code = cp + 16 * cq names
 * the edge each endpoint lies on -- edges 0..2 of the scene triangle, 4..6 of the query -- endpoints are cut points, never
 * interpolated, and the segment runs from p to q along cross(nq, nt), which flows one way along the curve on consistently oriented
 * meshes.  So the successor of a segment is an integer question to two edge adjacency tables: leaving through a scene edge, the
 * curve continues in the twin scene triangle with the same query; leaving through a query edge, it continues in the same scene
 * triangle with the twin query.  No coordinate is compared, no tolerance is chosen, nothing is welded, and the result is the same
 * bytes on every run.
 * Edge adjacency of a query mesh, drt_tri_edge_adjacency: tris and out are HOST pointers; out receives 3 * n values and capacity
 * is the room in values.  The rule is drt_scene_edge_adjacency's, word for word, on the nine coordinates of each drt_tri (the pad
 * is not read): half-edge 3 * i + e runs from vertex e to vertex (e + 1) % 3 of query i; two positions are the same iff their
 * three words are bit-equal; twins, -1 and -2 as there.  There is no BVH and no order other than the caller's.  DRT_ERR_INVALID:
 * capacity below 3 * n, or a NULL pointer with n > 0.
 * drt_renderer_chain_intersections: segs, splits (n + 1 values), query_adj (3 * n values), slots (total entries) and counts (3
 * words, may be NULL) are device pointers on the renderer's device; the call is enqueued on hip_stream (NULL = the renderer's)
 * and orders with the other queries as they do.  The scene's table is the renderer's device copy of drt_scene_edge_adjacency, the
 * one drt_renderer_chain_sections makes and drops; after a device-only drt_renderer_refit it is still the host scene's.
 * Ranges: query i's range is segs[splits[i] .. splits[i+1]), clamped exactly as drt_renderer_chain_sections clamps it: a
 * decreasing pair is an empty range, and nothing beyond total is read or written.  A range is what a fill wrote: records in
 * ascending prim, followed by any miss records.  The owner of record j is found by binary search as if splits ascended: lo = 0,
 * hi = n; while lo < hi: mid = lo + (hi - lo) / 2, and lo = mid + 1 if splits[mid] <= j, else hi = mid; j is owned by query
 * lo - 1 iff lo > 0 and j lies in that query's range, and by no query otherwise.  On ascending splits that is the one range that
 * holds j.
 * Live records: a record is live iff it has an owner, 0 <= prim < n_triangles (a miss record has prim -1), and both cp = code & 15
 * and cq = code >> 4 are in {0, 1, 2, 4, 5, 6}.  A record that is not live has no successor, takes no predecessor, and gets exit
 * status 5.
 * Link: for a live record j of query i, let T = prim_j.  If cq < 4: a = adj[3 * T + cq], the target range is query i's, the
 * target prim is a / 3 and the required entry code is a % 3.  If cq >= 4: a = query_adj[3 * i + cq - 4], the target range is
 * query a / 3, the target prim is T and the required entry code is 4 + a % 3; a value with a / 3 >= n is treated as -2, and so
 * is every negative value but -1.  a == -1: exit status 1 (a boundary edge).  a == -2: exit status 2 (non-manifold or flipped).
 * Otherwise m is the first record of the target range whose prim, read as unsigned, is not below the target prim, found by binary
 * search over the range (lo, hi = its ends; while lo < hi: mid = lo + (hi - lo) / 2, and lo = mid + 1 if prim_mid < target, else
 * hi = mid; m = lo).  If there is no such m, or prim_m is not the target prim, or m is not live, or m's owner is not the target
 * query: exit status 3 (the neighbour is not in the list).  Else if (code_m & 15) is not the required entry code: exit status 4
 * (the neighbour is cut through other edges).  Else succ(j) = m, exit status 0.  Both tables pair half-edges one to one, so m's
 * range, prim and entry code name j uniquely: succ is injective, and the components are simple paths and simple cycles.  On input
 * that breaks this (a query_adj that is no involution, a prim twice in a range), of the records that claim the same successor the
 * one of smallest index keeps it and the others get exit status 3: the components are simple paths and simple cycles on any
 * input, and every index written is below total.
 * Canonical order: one order over the whole list, because a curve crosses queries.  A path starts at its record without a
 * predecessor; a cycle starts at its record of smallest index, and is closed.  A record that is not live is a chain of one.  The
 * chains are ordered by the ascending index of their first record, and position pos runs over [0, total) in that order.
 * slots[pos] = {seg, first, length, flags} as drt_renderer_chain_sections has them: seg = the index into segs of the record that
 * stands there; first = the position of its chain's first record; length = its chain's length; flags: bit 0 = the chain is
 * closed, bits 1..3 = that record's exit status.  Every slot below total is written.  counts = {chains of live records, closed
 * ones among them, records that are not live}.  The result depends on segs, splits and the two tables only.
 * What this is not: no welding and no new points -- a curve's vertices are the p of its records, plus the last q of an open
 * chain; a curve is closed exactly where neighbouring triangles of either mesh agree on the side of their shared vertices, and
 * statuses 3 and 4 mark the places where they do not (a curve that runs through vertices or along edges falls into open chains);
 * self-intersection curves are not chained -- a mesh against itself lists each pair from both sides with different roles and
 * orientation; no clipped polygons and no boolean; no RendererGroup; nothing on the command line.
 * Working range and hostile surfaces (measured on the restatements, tests/test_hostile_surfaces_ref.py asserts the figures, and
 * compared with the kernels bit for bit in tests/test_gpu_hostile_surfaces.py; no rule is changed here).  Far from the origin: two
 * UV spheres of 1520 and 960 triangles of radius about 1 cut in one closed loop of 186 records; moved to (4096, -8192, 16384) and
 * rounded to fp32 the same pair gives three open chains of 58, 123 and 8 records that all end with status 4 -- a coordinate of 16384
 * leaves 2^-9 of resolution, and neighbours no longer agree on the side of a shared vertex.  Translate such a pair to its own
 * origin first.  Zero-area triangles inside a connected mesh (the cap (a, b, m) that closes an edge a b split on one side only, m
 * its midpoint): drt_renderer_chain_sections runs THROUGH an exactly flat cap -- the cap is cut like any triangle, its record has
 * zero length, and the contour stays closed (a band of 1040 triangles with 120 such caps: one closed chain at every level).
 * drt_renderer_intersect_triangles gives an exactly flat triangle no record at all (nt = 0, so u0 = u1 = u2 = 0 are one class), and
 * a curve that reaches one ends there with status 3; a cap whose midpoint was rounded is a sliver, has records, and links or ends
 * with 3 or 4 as its rounded normal decides.  A cap on each side of one edge makes the edges a m and m b non-manifold (-2).
 * Scale: the records are unchanged for 2^-24 to 2^32 (nq, nt are second powers of the lengths, D = cross(nq, nt) a fourth).  Beyond,
 * they are lost one by one, not all at once: of 229 records of the degenerate test mesh 213 are left at 2^-32, 68 at 2^-36 and none
 * at 2^-40 (D passes through the subnormals to 0 and fabsf(D[j]) > 0 fails); 161 at 2^36, 125 at 2^42 and 4 at 2^50 (infinities
 * compare like large numbers until inf - inf gives a NaN, which fails every comparison).  The chains of what is left follow the
 * rules as written.
 * Checks, drt_renderer_chain_sections' in its order, with query_adj checked where splits is: NULL r or scene; n == 0 or
 * total == 0 is DRT_OK with no launch; NULL segs, splits, query_adj or slots; segs and slots 16-byte aligned, splits, query_adj
 * and counts 4-byte aligned; n < 2^31 and total < 2^31; no pending asynchronous batch; device memory on the renderer's device;
 * the scene's upload (DRT_ERR_UNSUPPORTED beyond 64 levels); no BVH as drt_scene_edge_adjacency.  All DRT_ERR_INVALID but the
 * upload's.  The framebuffer, accumulation, sample count, counters, kernel info and kernel span are not touched. */
int           drt_tri_edge_adjacency(const drt_tri *tris, uint32_t n, int32_t *out, uint32_t capacity);
int           drt_renderer_chain_intersections(drt_renderer *r, const drt_scene *scene, const drt_isect *segs, const uint32_t *splits,
                                               const int32_t *query_adj, drt_chain_slot *slots, uint32_t *counts, uint32_t n,
                                               uint32_t total, void *hip_stream);

/* ---- triangle distance queries (new; the mesh triangle nearest each query triangle -- how far apart two meshes are) ----
 * One query = a drt_tri (48 bytes, 16-byte aligned, the three pad words are ignored) and a search distance: max_dist[i], or infinite
 * when max_dist is NULL.  The answer is the triangle of the mesh nearest the query triangle within that distance, the squared
 * distance and a witness pair of points.  A mesh is a batch of queries; the clearance of two meshes is the smallest d2 of the batch.
 * All arithmetic is fp32 with one rounding per operation, in the order written; dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z, / is the
 * correctly rounded division; there is no tolerance anywhere.
 * Validity and bounds are drt_renderer_overlap_triangles', unchanged: a query is valid iff all nine coordinates satisfy
 * fabsf(x) <= FLT_MAX, and qmin[j] = min3(q0[j], q1[j], q2[j]), qmax[j] = max3(q0[j], q1[j], q2[j]).  An invalid query pushes nothing
 * and gets the miss record.
 * Pair distance, on the query (q0, q1, q2) and the stored (v0, e1, e2), relative to q0 as the overlap test is, so that the magnitudes
 * are those of the pair and not of its distance from the origin:
 *   a1 = q1 - q0, a2 = q2 - q0, g = a2 - a1; p0 = v0 - q0, p1 = p0 + e1, p2 = p0 + e2, h = e2 - e1.
 * Fifteen candidates, in this order:
 *   0..2   the query's vertices 0, a1, a2 against the scene triangle (p0, e1, e2), by the seven cases of drt_renderer_nearest:
 *          c_query = the vertex, c_scene = (p0 + e1 u) + e2 v, dist2 as there
 *   3..5   the scene triangle's vertices p0, p1, p2 against the query triangle (0, a1, a2), by the same routine with v0 = 0:
 *          c_scene = the vertex, c_query = (0 + a1 u) + a2 v
 *   6..14  the nine edge pairs: query edge i of ((0, a1), (a1, g), (a2, -a2)) against scene edge j of ((p0, e1), (p1, h), (p2, -e2)),
 *          candidate 6 + 3 i + j
 * An edge pair (P1, d1), (P2, d2) is the clamped segment-segment closest points of Ericson, Real-Time Collision Detection 5.1.9, with
 * exact-zero degenerate cases and no epsilon:
 *   r = P1 - P2, a = dot(d1, d1), e = dot(d2, d2), f = dot(d2, r), c = dot(d1, r), b = dot(d1, d2), den = a e - b b;
 *   clamp(x) = fminf(fmaxf(x, 0), 1) + 0 (a NaN x gives 0; the sum makes a zero result +0 whichever zero fmaxf(-0, 0) returns);
 *   a <= 0 && e <= 0: s = t = 0;  else a <= 0: s = 0, t = clamp(f / e);  else e <= 0: t = 0, s = clamp(-c / a);
 *   otherwise s = den > 0 ? clamp((b f - c e) / den) : 0 and t = (b s + f) / e; if t < 0 then t = 0 and s = clamp(-c / a); else if
 *   t > 1 then t = 1 and s = clamp((b - c) / a);
 *   c_query = c1 = P1 + d1 s, c_scene = c2 = P2 + d2 t, diff = c1 - c2, dist2 = dot(diff, diff).
 * The pair's d2 and its candidate: d2 = +infinity, candidate = 0, and candidate k, in order, replaces them iff its dist2 < d2 -- strict,
 * so the first wins a tie and a NaN never wins.  Every candidate is the squared distance of two points that lie on the two triangles,
 * so d2 never understates the true distance by more than rounding.  Then, if the seventeen axes of drt_renderer_overlap_triangles'
 * triangle test (unchanged) do not separate the pair: d2 = 0 and feature = candidate | 16; the witness points stay those of the best
 * candidate and are then NOT a contact point.  Otherwise feature = candidate.  The predicate is part of the rule because the fifteen
 * candidates alone cannot see an edge that pierces the interior of a large triangle: there all fifteen are positive.  Its conservatism
 * on zero-area triangles is inherited: a segment or a point may get d2 = 0 for a near miss in the triangle's own plane.
 * Node bound: per axis d = fmaxf(fmaxf(bmin - qmax, 0), qmin - bmax) (a NaN operand is dropped), box2 = (dx dx + dy dy) + dz dz:
 * drt_renderer_nearest's box distance with the point replaced by the query's interval.
 * Traversal: drt_renderer_nearest's, word for word.  best = max_dist * max_dist, prim = -1.  The root is pushed with its box2.  A
 * popped entry is dropped unless box2 < best.  A leaf tests its triangles in order; a pair replaces the result iff d2 < best.  An
 * interior node computes box2 of both children and pushes a child iff its box2 < best, the farther one first (b1 > b2 -> child 1).
 * Once a pair with d2 = 0 is found nothing passes any more, so touching meshes end early.  The node bound is taken in absolute
 * coordinates and the pair relative to q0: for a query far from a flat wall the two can differ by an ulp, and a triangle whose node
 * the bound rejects is not tested, whatever its pair distance would be.
 * Modes: DRT_TRIDIST_NEAREST is the search above.  DRT_TRIDIST_ANY ends a query at the first pair with d2 < best and records that
 * pair: the first within the distance in traversal order, not the nearest.  Its purpose is the boolean prim >= 0.
 * Result: drt_tri_near {point_q, d2, point_t, prim, u, v, feature, pad}, 48 bytes.  point_q = q0 + c_query and point_t = q0 + c_scene
 * of the winning candidate of the winning pair; prim = triangle index in drt_scene_get_triangles order; (u, v) are the barycentrics
 * of point_t on the scene triangle, v0 + e1 u + e2 v: the routine's own for candidates 0..2; (0, 0), (1, 0), (0, 1) for 3, 4, 5; and
 * from the edge parameter t for 6..14 -- (t, 0) on scene edge 0, (1 - t, t) on edge 1, (0, 1 - t) on edge 2, one subtraction.  pad = 0.
 * The miss record (nothing within max_dist, an invalid query, a NaN max_dist, an empty scene) is all zero with d2 = max_dist * max_dist
 * and prim = -1.  A negative max_dist searches as its absolute value does, as drt_renderer_nearest's.  A result depends on its query
 * and the scene only.
 * What this is not: there is no penetration depth -- d2 = 0 says that the conservative overlap predicate does not separate the pair,
 * and nothing about how deep; no self-clearance -- a query taken from the scene itself touches itself and its neighbours; one answer
 * per query -- no k-nearest or within-distance list of triangles; alpha cut-outs are ignored.
 * Conventions are drt_renderer_nearest's and drt_renderer_overlap_triangles': the argument checks in that order (the handles, the mode,
 * n == 0 is a no-op, NULL tris or out, alignment -- tris and out 16-byte, max_dist 4-byte --, n < 2^31, a pending batch, device memory
 * on the renderer's device), hip_stream NULL = the renderer's stream, the call only enqueues, in order with the other queries (the
 * same event), a refitted device copy is the one queried, the 64-level bound, legal on a sharded renderer, and the framebuffer,
 * accumulation, sample count, counters, kernel info and kernel span are not touched. */
typedef struct drt_tri_near { float point_q[3]; float d2; float point_t[3]; int32_t prim; float u, v; int32_t feature; int32_t pad; } drt_tri_near;   /* 48 B */
#define DRT_TRIDIST_NEAREST 0
#define DRT_TRIDIST_ANY     1
int           drt_renderer_triangle_distance(drt_renderer *r, const drt_scene *scene, const drt_tri *tris, const float *max_dist,
                                             drt_tri_near *out, uint32_t n, int32_t mode, void *hip_stream);

/* ---- triangle casts (new; the first contact of a translating triangle with the mesh -- when a moving mesh touches) ----
 * One cast = a drt_tri (48 bytes, 16-byte aligned, the three pad words are ignored) and a drt_motion {d[3], tmax} (16 bytes, 16-byte
 * aligned).  The triangle is at q + d t; the answer is the smallest t in [0, tmax) at which it touches a triangle of the mesh, that
 * triangle, the contact point on it and a contact normal.  There is no tmin: the caller passes the triangle where the motion starts, so
 * t is a quotient and not a sum.  A moving mesh is a batch of casts; its time of impact is the smallest t of the batch.
 * All arithmetic is fp32 with one rounding per operation, in the order written; dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z,
 * cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x), / is the correctly rounded division; there is no tolerance
 * and no thickness anywhere.
 * Validity: the query is valid iff drt_renderer_overlap_triangles' validity holds (all nine coordinates satisfy fabsf(x) <= FLT_MAX)
 * and no component of d and not tmax is a NaN.  An invalid cast pushes nothing and gets the miss record.
 * Pair, on the query (q0, q1, q2) and the stored (v0, e1, e2), relative to q0 as the distance query is:
 *   a1 = q1 - q0, a2 = q2 - q0, g = a2 - a1, nq = cross(a1, a2); p0 = v0 - q0, p1 = p0 + e1, p2 = p0 + e2, h = e2 - e1.
 * How a quotient is formed, everywhere: a candidate has ONE determinant det and three numerators.  sg = det < 0 ? -1 : 1 and
 * ad = fabsf(det); every numerator is multiplied by sg (exact); every test compares a numerator with 0 or with ad, all closed; and a
 * parameter is fabsf(numerator) / ad, one division, formed only for a candidate that passed (so a zero is +0).  No parameter is
 * divided before it is tested, and no reciprocal is taken.  A NaN fails every test; det = 0 has no candidate.
 * Fifteen candidates, in this order:
 *   0..2   the query's vertices 0, a1, a2 as rays (o, d) against the scene triangle (p0, e1, e2); 3..5 the scene triangle's vertices
 *          p0, p1, p2 as rays (o, -d) against the query triangle (0, a1, a2).  A ray (o, d) against (w0, f1, f2) is Moller-Trumbore
 *          without the renderer's 1e-6: pv = cross(d, f2), det = dot(f1, pv), tv = o - w0, qv = cross(tv, f1),
 *          nu = dot(tv, pv) sg, nv = dot(d, qv) sg, ntau = dot(f2, qv) sg;
 *          passes iff det != 0 && nu >= 0 && nv >= 0 && nu + nv <= ad && ntau >= 0; tau = fabsf(ntau) / ad.
 *   6..14  the nine edge pairs: query edge i of ((0, a1), (a1, g), (a2, -a2)) against scene edge j of ((p0, e1), (p1, h), (p2, -e2)),
 *          candidate 6 + 3 i + j.  An edge pair (a, ea), (b, eb) solves a + ea s + d tau = b + eb w by Cramer's rule on the columns
 *          (ea, d, -eb): nb = -eb, c = cross(d, nb), det = dot(ea, c), r = b - a,
 *          ns = dot(r, c) sg, ntau = dot(ea, cross(r, nb)) sg, nw = dot(ea, cross(d, r)) sg;
 *          passes iff det != 0 && ns >= 0 && ns <= ad && nw >= 0 && nw <= ad && ntau >= 0; tau = fabsf(ntau) / ad.
 * The pair's t and its candidate: t = +infinity, candidate = 15, and candidate k, in order, replaces them iff it passes and its
 * tau < t -- strict, so the first wins a tie.  Touching counts: every comparison is closed.
 * Start overlap: if the seventeen axes of drt_renderer_overlap_triangles' triangle test (unchanged) do not separate the query at
 * t = 0 from the scene triangle, the pair's t = 0 and feature = candidate | 16 (31 if no candidate passed).  Otherwise feature =
 * candidate.  The predicate is part of the rule because the candidates alone cannot see a pair that already interpenetrates: an edge
 * through the interior of a large triangle moving along that triangle's plane has no candidate at all, or only positive ones.  Its
 * conservatism on zero-area triangles is inherited.
 * Across triangles, drt_renderer_sphere_cast's rule: best = tmax, prim = -1, and the pair of triangle k replaces the result iff
 * t < best || (t == best && k < prim), so the answer does not depend on the tree.  tmax <= 0 finds nothing.
 * Traversal: drt_renderer_sphere_cast's slab test with the query's extent in place of the radius.  ext_lo = qmin - q0 and
 * ext_hi = qmax - q0 with qmin, qmax drt_renderer_overlap_triangles' bounds; inv_d = 1 / d per component; per axis
 * t0 = ((bmin - ext_hi) - q0) inv_d, t1 = ((bmax - ext_lo) - q0) inv_d, enter = the largest of fminf(t0, t1), exit = the smallest of
 * fmaxf(t1, t0) (a NaN operand, 0 * inf, is dropped).  A node is visited iff enter <= exit && exit >= 0 && enter <= best.  The root is
 * pushed iff it passes and the cast is valid; a popped entry is dropped unless its enter <= best still holds; a leaf tests its
 * triangles in order; an interior node pushes each child that passes, the farther one first (enter1 > enter2 -> child 1); the limit is
 * 64 levels.  The node test is taken in absolute coordinates and the pair relative to q0: a contact whose widened box the fp32 slab test
 * misses by a rounding is not found.  d = 0 degenerates to the static overlap test, as the sphere cast's zero direction does: every det
 * is 0, inv_d is +-inf, and the result is the lowest-numbered triangle that the predicate does not separate, with t = 0, or a miss.
 * Modes: DRT_TRICAST_FIRST is the search above.  DRT_TRICAST_ANY ends a cast at the first pair with t < best in traversal order and
 * records that pair: not the first contact.  Its purpose is the boolean prim >= 0.
 * Result: drt_tri_hit {point, t, normal, prim, u, v, feature, pad}, 48 bytes.  The contact is recomputed once, after the traversal,
 * from the winning (prim, candidate), by the candidate's own operations:
 *   0..2   u = fabsf(nu) / ad, v = fabsf(nv) / ad, c = (p0 + e1 u) + e2 v, normal = cross(e1, e2)
 *   3..5   c = the vertex p0, p1 or p2, (u, v) = (0, 0), (1, 0), (0, 1), normal = nq
 *   6..14  w = fabsf(nw) / ad, c = b + eb w, (u, v) = (w, 0) on scene edge 0, (1 - w, w) on edge 1, (0, 1 - w) on edge 2, one
 *          subtraction, normal = cross(ea, eb)
 * point = q0 + c is the contact point on the scene triangle (which does not move) and (u, v) its barycentrics there, v0 + e1 u + e2 v.
 * normal is unnormalised and flipped against the motion: if dot(normal, d) > 0 every component is negated, so dot(normal, d) <= 0.  A
 * start overlap (bit 16) has no contact: point, normal, u and v are zeros, t = 0.  pad = 0.  The miss record (nothing touched in
 * [0, tmax), an invalid cast, an empty scene) is all zero with t = tmax, the motion's own word, prim = -1 and feature = -1.  A result
 * depends on its cast and the scene only.  (Beyond the working range a field can be a NaN, inf / inf; which NaN is not specified.)
 * What this is not: a pair that is coplanar and slides in its common plane is seen only by the start overlap -- every det is 0 there --
 * as drt_renderer_intersect_triangles has no coplanar records either; there is no tolerance and no thickness -- a contact exactly on a
 * seam (a vertex onto an edge, an edge onto a vertex) is found by whichever neighbouring candidate's closed test passes, and in fp32
 * in rare cases by none; no rotation; no penetration depth -- t = 0 with bit 16 says that the conservative predicate does not separate
 * the pair at the start, and nothing about how deep; alpha cut-outs are ignored; one answer per cast.
 * Conventions are drt_renderer_triangle_distance's: the argument checks in that order (the handles, the mode, n == 0 is a no-op, NULL
 * tris, motions or out, alignment -- all three 16-byte --, n < 2^31, a pending batch, device memory on the renderer's device),
 * hip_stream NULL = the renderer's stream, the call only enqueues, in order with the other queries (the same event), a refitted device
 * copy is the one queried, DRT_ERR_UNSUPPORTED beyond 64 levels, DRT_ERR_INVALID while an asynchronous batch is pending, legal on a
 * sharded renderer, and the framebuffer, accumulation, sample count, counters, kernel info and kernel span are not touched. */
typedef struct drt_motion { float d[3]; float tmax; } drt_motion;   /* 16 B */
typedef struct drt_tri_hit { float point[3]; float t; float normal[3]; int32_t prim; float u, v; int32_t feature; int32_t pad; } drt_tri_hit;   /* 48 B */
#define DRT_TRICAST_FIRST 0
#define DRT_TRICAST_ANY   1
int           drt_renderer_triangle_cast(drt_renderer *r, const drt_scene *scene, const drt_tri *tris, const drt_motion *motions,
                                         drt_tri_hit *out, uint32_t n, int32_t mode, void *hip_stream);

/* ---- surface lookups and area-weighted sampling (new; the reference has neither) ----
 * Every query above answers with a triangle index and two barycentrics.  drt_renderer_surface_lookup turns such a reference into what
 * lies on the surface there, read from the renderer's device copy of the scene; drt_renderer_sample_surface draws references on the
 * mesh with probability proportional to area.  Neither traverses the BVH.  Both are stated bit for bit: fp32 with one rounding per
 * operation, in the order written.
 *
 * drt_renderer_surface_lookup.  refs: n drt_hit {t, prim, u, v} (16 bytes, 16-byte aligned) -- the output of drt_renderer_trace_rays
 * and drt_renderer_list_hits as it stands; t is not read.  out: n drt_surface, 96 bytes, 16-byte aligned, written with six 16-byte
 * stores.
 *   valid      0 <= prim < n_tris.  Anything else (a query's miss -1, an index beyond the mesh) gets the miss record: all zero bits
 *              except material = load_index = texture = -1.
 *   (u, v)     are used as given: no clamp, outside the triangle every field extrapolates.  w = 1.0f - u - v (Intersection.cu's).
 *   position   (v0 + u e1) + v e2 per component, of the device copy's v0, e1 = v1 - v0, e2 = v2 - v0: after drt_renderer_refit the
 *              moved triangle.
 *   normal     the stored face normal, as is -- not turned, there is no ray; of a zero-area triangle a NaN, which NaN is not specified.
 *   uv         (w uv0 + u uv1) + v uv2 per component (RayGen.cuh:116).
 *   albedo,    a material without a texture: its flat albedo, alpha = 1.  Otherwise the reference's getPixel / getAlpha
 *   alpha      (Texture.cu:33-75): with f = c - floorf(c) per component, x = (int)(f.x width), y = (int)(f.y height), the texel
 *              y width + x of the renderer's own pool, every texture followed by width + 1 zero texels (uv = 1 or a tiny negative
 *              one reads them, as the renderer does); albedo = (c / 255)^2 per channel for 3 and 4 channels, (0, 0, 1) for any other
 *              count; alpha = a / 255 with 4 channels, else 1.  This is what the ALBEDO view and drt_renderer_render_guides show.
 *   departure  the caller supplies (u, v), so uv can be a NaN or an infinity, which the renderer never meets: a fractional part f
 *              that fails f >= 0 && f <= 1 is taken as 0 before the conversion.  A finite uv is unaffected; nothing is read outside
 *              the pool.
 *   material   the triangle's material id; texture = its albedo_tex, or -1 if that is negative; emissive, roughness,
 *              refractive_index as drt_scene_add_material_ex set them; flags bit 0 = metallic, bit 1 = transmission.
 *   shading    (w N0 + u N1) + v N2 of the three vertex normals: NOT normalised and not turned.  normals = NULL: the HOST scene's
 *              vertex normals (drt_scene_get_triangles), also after a drt_renderer_refit that was given others -- the device keeps only
 *              their average.  normals != NULL: a device array float[n_tris][3][3] in LOAD order, the array drt_renderer_refit takes
 *              (4-byte aligned, n_tris * 36 bytes), read through drt_scene_get_triangle_order; used instead and not retained.
 *   load_index drt_scene_get_triangle_order's entry of prim.
 * The first lookup after a scene upload uploads the host scene's vertex normals and the load-order table into buffers of its own.
 *
 * drt_renderer_surface_weights writes the table the samples are drawn from: cdf, a device uint64[n_tris], 16-byte aligned.
 *   a_k        c = cross(e1, e2) of the device copy, a = sqrtf((c.x c.x + c.y c.y) + c.z c.z), the correctly rounded sqrt: twice the
 *              area.  A non-finite a (a NaN or an infinity in the triangle, or an overflow) counts as 0.
 *   amax       the maximum of a_k.  amax == 0: every q is 0.  Otherwise e = frexp's exponent of amax (amax = m 2^e, 0.5 <= m < 1,
 *              subnormals included).
 *   q_k        (uint64_t)ldexp((double)a_k, 35 - e), truncated; the scaling is exact in double.  q_k < 2^36, so no sum below 2^28
 *              triangles overflows; a triangle smaller than amax 2^-36 has weight 0.
 *   cdf[k]     q_0 + ... + q_k.  total = cdf[n_tris - 1].  Integers: the same bytes whatever computes them and in whatever order
 *              (on the device a three-phase scan over blocks of DRT_SURFACE_SCAN_BLOCK triangles; no workgroup waits for another).
 * A mesh scaled by a power of two has the same table.  n_tris == 0 is a no-op.
 *
 * drt_renderer_sample_surface.  Sample k of a call has index i = first + k; first + n <= 2^32.  pcg = the reference's pcg_hash
 * (Random.cu:6-11).  s = pcg(i ^ pcg(seed)), h1 = pcg(s), h2 = pcg(h1), h3 = pcg(h2), h4 = pcg(h3).
 *   prim       R = (uint64_t)h1 << 32 | h2, target = the high 64 bits of R total; prim = the smallest k with cdf[k] > target.  A
 *              triangle of weight 0 is never drawn.  total == 0 (no triangle, or none with an area): the miss record {0, -1, 0, 0}.
 *   (u, v)     a = h3 >> 8, b = h4 >> 8; if a + b > 2^24 then a = 2^24 - a and b = 2^24 - b; u = a 2^-24, v = b 2^-24.  So u, v >= 0,
 *              u + v <= 1, and w = 1 - u - v is exact and >= 0.
 *   record     drt_hit {t = 0, prim, u, v}: it feeds drt_renderer_surface_lookup as it is.
 * A sample depends on (seed, i) and the scene only: a batch split in two with `first` gives the same records.  The table is computed
 * again by every call (one pass over the triangles), from the device copy: after drt_renderer_refit the moved mesh is sampled.
 *
 * What this is not: the nearest texel only, as the reference has -- no filtering, no mip levels; no normal maps and no tangents;
 * shading is not normalised; no stratified or blue-noise sampling -- independent hashes; no drt_group_* form and no command line.
 * Conventions are drt_renderer_trace_rays': the argument checks in that order (the handles, n == 0 is a no-op, NULL refs or out,
 * alignment, n < 2^31, a pending batch, device memory on the renderer's device -- a normals allocation shorter than n_tris * 36 bytes
 * and a table shorter than n_tris * 8 are refused where the runtime can tell), hip_stream NULL = the renderer's stream, the call only
 * enqueues, in order with the other queries (the same event), the scene is uploaded as for rendering -- a scene without a BVH is
 * refused, but there is no limit of 64 levels: nothing here traverses --, DRT_ERR_INVALID while an
 * asynchronous batch is pending, legal on a sharded renderer, and the framebuffer, accumulation, sample count, counters, kernel info
 * and kernel span are not touched. */
typedef struct drt_surface {
    float position[3]; int32_t material;      /* material id, -1 = no such triangle                         */
    float normal[3];   float   alpha;         /* stored face normal, as is;  texel alpha or 1                */
    float shading[3];  int32_t load_index;    /* interpolated vertex normals, NOT normalised;  triangleOrder */
    float albedo[3];   int32_t texture;       /* what the ALBEDO view shows;  albedo_tex or -1               */
    float uv[2];       float roughness; uint32_t flags;   /* bit 0 metallic, bit 1 transmission             */
    float emissive[3]; float refractive_index;
} drt_surface;                                /* 96 B */
#define DRT_SURFACE_SCAN_BLOCK 256
int           drt_renderer_surface_lookup(drt_renderer *r, const drt_scene *scene, const drt_hit *refs, const float *normals,
                                          drt_surface *out, uint32_t n, void *hip_stream);
int           drt_renderer_surface_weights(drt_renderer *r, const drt_scene *scene, uint64_t *cdf, void *hip_stream);   /* device uint64[n_tris] */
int           drt_renderer_sample_surface(drt_renderer *r, const drt_scene *scene, uint32_t seed, uint32_t first, drt_hit *out,
                                          uint32_t n, void *hip_stream);

/* ---- ambient occlusion (new; cosine-weighted visibility at surface points -- the reference shades only along its paths) ----
 * How much of the hemisphere above a surface point is open: ambient occlusion, sky-view factor, accessibility, and the bent normal.
 * For every point S occlusion rays are made where they are used, in the renderer's own bounce directions, traced by
 * drt_renderer_occluded's traversal and reduced per point; no ray is stored.  Stated bit for bit: fp32 with one rounding per
 * operation, in the order written; dot(a, b) = a.x b.x + a.y b.y + a.z b.z, left to right (helper_math.cuh:1264);
 * normalize(v) = v * (1.0f / sqrtf(dot(v, v))) (helper_math.cuh:1325, :78-81), division and sqrtf correctly rounded.
 *
 * A query point is drt_ao_point {p[3], max_dist, n[3], bias}: 32 bytes, the layout of drt_ray, 16-byte aligned.  Per call
 * drt_ao_params {samples, seed, first, flags}: samples = S with 1 <= S <= 4096; first continues a stream as
 * drt_renderer_sample_surface's does, first + n <= 2^32; flags must be 0.  pcg = the reference's pcg_hash (Random.cu:6-11).
 * For point i of the call and sample j in [0, S):
 *   h          pcg((first + i) ^ pcg(seed))
 *   state      pcg(j ^ h)
 *   fuzz       randomUnitSphereVec3(state) (Random.cu:50-58): candidates ((float)state / 2^32) * 2 - 1 per component after
 *              state = pcg(state), x, then y, then z, normalised, until len * len < 1 with len = sqrtf(dot(c, c)); with the renderer's
 *              guard: the 1024th candidate is kept whatever its length.  The renderer's diffuse bounce draws it the same way.
 *   d          normalize(n + fuzz) (RayGen.cuh:133-134)
 *   o          p + n * bias per component (RayGen.cuh:121 with bias for 0.001)
 *   occluded   iff drt_renderer_occluded says so for the ray {o, tmin = 0, d, tmax = max_dist}: the same traversal, the root skipped
 *              if its entry distance e has e < 0 || e > tmax, a child pushed iff e >= 0 && !(e > tmax), a triangle counts iff
 *              t > tmin && t < tmax && AnyHit -- alpha cut-outs are seen through as there.  Otherwise the sample is open.
 * n is used as given: pass a unit normal for a cosine-weighted answer (fuzz lies on the unit sphere, so d is then distributed as the
 * cosine of its angle to n).  No guard is added: a NaN anywhere in o or d hits nothing, as in drt_renderer_occluded, and the sample
 * counts as open; n + fuzz = 0 makes d a NaN.
 *
 * The answer per point is drt_ao_result {open, bent[3]}: 16 bytes, 16-byte aligned, int32 each.
 *   open       the number of open samples.
 *   bent[k]    the sum over the open samples of (int32_t)(d[k] * 65536.0f): the product is exact, the cast truncates.  A product that
 *              is a NaN or not below 2^31 in magnitude adds 0 (the cast has no value there).  |d[k]| <= 1 up to rounding, so
 *              |bent[k]| <= 4096 * 65536 = 2^28: it cannot overflow.  bent / (65536 open) is the mean open direction, the bent normal,
 *              not normalised.
 *   skipped    a point with !(max_dist >= 0) (negative or a NaN) costs no rays; its record is {-1, 0, 0, 0}.  max_dist = 0: every
 *              sample is open (t < 0 never holds).  max_dist = +inf: sky visibility.
 * Both fields are integer sums, so a record is the same bytes whatever order, tiling or hardware computes it: that is why bent is not a
 * float.  A record depends on (seed, first + i, S), its point and the scene only: a batch split in two with `first` gives the same
 * records.  After drt_renderer_refit the moved mesh occludes.
 *
 * On the device the work unit is a tile of 64 lanes: for S >= 64 samples [64 t, min(64 t + 64, S)) of one point; for S in {1, 2, 4, 8,
 * 16, 32} 64 / S consecutive points with S lanes each; for any other S < 64 one point with idle lanes.  The tile count is a 64-bit
 * number.  One lane per point writes the whole record with one 16-byte store (S <= 64) or adds to it with integer atomics (S > 64); a
 * pass before the tracing kernel writes the skipped points' records.  There are no floating-point atomics.
 *
 * What this is not: no distance falloff and no weighting beyond the cosine of the draw; no stratified or low-discrepancy directions --
 * independent hashes; no indirect light -- drt_renderer_radiance does that; no filtering across points; the absolute bias and the ray
 * family's 1e-6 apply as in drt_renderer_trace_rays (the "working range" paragraph above says what that means for small meshes); no
 * drt_group_* form and no command line.
 * Conventions are drt_renderer_occluded's, with every argument checked before any device work, in this order: the handles and params,
 * samples 0 or > 4096, flags != 0, n == 0 is a no-op, NULL pts or out, 16-byte alignment, n < 2^31, first + n <= 2^32, a scene without
 * a BVH, a pending asynchronous batch (DRT_ERR_INVALID each); then pts and out must be device memory on the renderer's device.
 * hip_stream NULL = the renderer's stream; the call only enqueues, in order with the other queries (the same event); the scene is
 * uploaded as for rendering; DRT_ERR_UNSUPPORTED for trees deeper than 64 levels; legal on a sharded renderer; the framebuffer,
 * accumulation, sample count, counters, kernel info and kernel span are not touched.
 * drt_debug_ambient_stats switches the tracing kernel's counting build on (enable != 0, counters zeroed) or off and reads, after the
 * queries in flight, {trips of the waves' traversal loops, lanes that took a step in them}: lane utilisation = out[1] / (64 out[0]).
 * Results do not change. */
typedef struct drt_ao_point  { float p[3]; float max_dist; float n[3]; float bias; } drt_ao_point;       /* 32 B */
typedef struct drt_ao_params { uint32_t samples; uint32_t seed; uint32_t first; uint32_t flags; } drt_ao_params;
typedef struct drt_ao_result { int32_t open; int32_t bent[3]; } drt_ao_result;                           /* 16 B */
int           drt_renderer_ambient_occlusion(drt_renderer *r, const drt_scene *scene, const drt_ao_point *pts, uint32_t n,
                                             const drt_ao_params *params, drt_ao_result *out, void *hip_stream);
int           drt_debug_ambient_stats(drt_renderer *r, int32_t enable, uint64_t out[2]);

/* ---- generalised winding numbers (new; inside tests and signed distance for meshes that are open or unevenly oriented) ----
 * w(q) = the sum over the triangles of the signed solid angle each subtends at q, divided by 4 pi (Jacobson et al. 2013): exactly 1
 * inside and 0 outside a closed mesh with outward faces, and on a mesh with holes a value that degrades smoothly instead of flipping,
 * so that w >= 0.5 is an inside test that a missing triangle does not break.  It is evaluated on the renderer's tree (Barill et al.
 * 2018, first order): a subtree that is far from the point is replaced by one dipole term from a per-node moment.  Stated bit for
 * bit: fp32 with one rounding per operation, in the order written, a + b + c + d = ((a + b) + c) + d; dot(a, b) = a.x b.x + a.y b.y +
 * a.z b.z; cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x); division and sqrtf correctly rounded; |v| =
 * sqrtf(dot(v, v)).
 *
 * Triangle term, on the stored (v0, e1, e2) of a triangle, for the point q:
 *   a = v0 - q, b = a + e1, c = a + e2
 *   det = dot(a, cross(e1, e2)) -- the triangle's own winding e1 x e2, as drt_renderer_crossings uses it, not the stored face normal
 *   den = |a| * |b| * |c| + dot(a, b) * |c| + dot(b, c) * |a| + dot(c, a) * |b|
 *   omega = 2.0f * atan2(det, den), in steradians (van Oosterom and Strackee 1983)
 * A triangle with det == 0 contributes exactly 0 -- an edge-on view, a zero-area triangle, q in the triangle's plane -- so atan2(0, x)
 * is never evaluated.
 * atan2(y, x) is the project's own, one division and a fixed polynomial in plain fp32 + * / (the library's atan2f is not used: it
 * cannot be restated to the bit), for y != 0:
 *   ax = |x|, ay = |y|; swap = ay > ax; mx = swap ? ay : ax; mn = swap ? ax : ay
 *   big = mn > 0.414213562f * mx
 *   t = big ? (mn - mx) / (mn + mx) : mn / mx;  s = t * t
 *   r = (((8.05374449538e-2f * s - 1.38776856032e-1f) * s + 1.99777106478e-1f) * s - 3.33329491539e-1f) * s * t + t
 *   if big: r = 0.785398163f + r;  if swap: r = 1.57079633f - r;  if x < 0: r = 3.14159265f - r;  if y < 0: r = -r
 * (the coefficients are those of the Cephes library's atanf for |t| <= tan(pi / 8)).  A NaN in x or y gives a NaN; so does inf / inf.
 *
 * Node moment, 32 bytes per tree node, interior and leaf: drt_winding_moment {N[3], r2, p[3], pad}, pad = 0.  Per triangle
 * n_t = 0.5f * cross(e1, e2), area_t = |n_t|, c_t = v0 + (e1 + e2) / 3.0f.  A leaf sums its triangles in ascending tree index from
 * zeros: N = N + n_t, A = A + area_t, S = S + area_t * c_t, per component.  A parent is child 1 + child 2, in that order, for N, A and
 * S.  Then p = S / A per component, the area-weighted centroid; if !(A > 0), or A or a component of p is not finite, p = 0.5f * (lo + hi),
 * the centre of the node's box as the tree stores it: the child box in the parent's record, or the root box.  r2 = dx dx + dy dy + dz dz
 * with dx = max(|p.x - lo.x|, |hi.x - p.x|) and so on: the squared distance from p to the farthest corner of that box.  Every moment is
 * therefore the same bytes whatever computes it.  The moments are made from the device's triangles and boxes by the first winding call
 * after an upload or a drt_renderer_refit, on that call's stream, and kept until the next one: a refitted copy answers for the moved mesh.
 *
 * Evaluation of a point: a depth-first walk from the root, child 1 before child 2, over a stack that never holds more entries than the
 * tree has levels.  One fp32 accumulator, in steradians, starts at 0 and is added to in visit order.  For a visited node, the root or a
 * leaf as a whole included, d = p - q and dd = dot(d, d):
 *   iff dd > (beta * beta) * r2   the node is replaced by its dipole: accumulator += dot(d, N) / (dd * sqrtf(dd))
 *   otherwise                     an interior node is descended; a leaf adds omega of its triangles in ascending index.
 * w = accumulator * 0.0795774715f: the 1 / (4 pi) is applied once, at the end.  beta = +inf never approximates (inf * 0 is a NaN and
 * the comparison fails, which is the intended reading): the exact sum over all triangles.  beta = 0 answers with the root's dipole
 * alone.  beta = 2 is the default of the wrappers.  A point with a NaN or an infinity answers NaN without walking; an empty scene
 * answers 0.  Alpha cut-outs are ignored; drt_point's max_dist is ignored by the first two entry points.
 * Results: drt_renderer_winding_numbers writes the float w; drt_renderer_winding_inside one byte, w >= threshold ? 1 : 0 (a NaN is 0);
 * drt_renderer_winding_signed_distance runs drt_renderer_nearest and then, on the same stream, replaces the last word, side, of every
 * record by w >= threshold ? -1 : +1, in miss records too; the first seven words are unchanged.  Results are written with ordinary
 * stores; there are no floating-point atomics and no sums across lanes: a point's answer depends on its own walk only, so a batch in
 * any order, size or tiling gives the same bytes.
 *
 * What this is not: first order only -- the dipole's error falls as 1 / beta^2 and the second-order terms of Barill et al. are not
 * built; a point on the surface has no defined answer; orientation is still assumed per connected patch -- a patch with flipped
 * faces subtracts; fp32 throughout, so the determinant of a triangle that is far away and seen edge-on cancels; no drt_group_* form
 * and no command line.  drt_renderer_inside's rules stay 0 and 1: this is a separate entry point.
 * Conventions are drt_renderer_nearest's, with every argument checked before any device work, in this order: the handles, a negative
 * or NaN beta, n == 0 is a no-op, NULL points or out, points and drt_nearest records 16-byte aligned and floats 4-byte aligned,
 * n < 2^31, a pending asynchronous batch (DRT_ERR_INVALID each); then points and out must be device memory on the renderer's device.
 * hip_stream NULL = the renderer's stream; the call only enqueues, in order with the other queries (the same event);
 * DRT_ERR_UNSUPPORTED for trees deeper than 64 levels; legal on a sharded renderer; the framebuffer, accumulation, sample count,
 * counters, kernel info and kernel span are not touched.
 * drt_debug_winding_moments reads the moments back (making them if they are stale): *count = interior nodes + leaves, and into out,
 * if it is not NULL and holds 8 * *count floats, the interior nodes' records in the host scene's node order followed by the leaves'. */
typedef struct drt_winding_moment { float N[3]; float r2; float p[3]; float pad; } drt_winding_moment;     /* 32 B */
int           drt_renderer_winding_numbers(drt_renderer *r, const drt_scene *scene, const drt_point *points, uint32_t n, float beta,
                                           float *out, void *hip_stream);
int           drt_renderer_winding_inside(drt_renderer *r, const drt_scene *scene, const drt_point *points, uint32_t n, float beta,
                                          float threshold, uint8_t *out, void *hip_stream);
int           drt_renderer_winding_signed_distance(drt_renderer *r, const drt_scene *scene, const drt_point *points, uint32_t n, float beta,
                                                   float threshold, drt_nearest *out, void *hip_stream);
int           drt_debug_winding_moments(drt_renderer *r, const drt_scene *scene, float *out, size_t out_floats, uint32_t *count);

/* ---- isosurface extraction (new; a watertight triangle mesh from a 3-D field -- the step that turns drt_renderer_signed_distance's
 * and drt_renderer_winding_numbers' grids, or any field of the caller's, back into a surface) ----
 * Marching tetrahedra on the six-tetrahedron Kuhn split of every cube around its 0 -> 7 diagonal.  Neighbouring cubes agree on every
 * face diagonal, so the output is a closed, consistently oriented 2-manifold by construction wherever it does not leave the grid;
 * there are no ambiguous cases, and the whole table is the 16 rows below.  The call needs no scene and no tree.
 * All arithmetic is fp32 with one rounding per operation, in the order written.
 * Field: float32 [Z][Y][X] on the renderer's device, x fastest; drt_grid {lo[3], cell[3], dims[3] = (X, Y, Z)} is a small POD read on
 * the host.  Sample (i, j, k) lies at lo + ((float)idx + 0.5f) * cell per component -- the conversion, the add of 0.5f, the multiply
 * and the add are each rounded on their own.  That is the layout of the Python wrapper's sdfGrid, whose grids pass straight in with
 * cell = (hi - lo) / res per component in fp32.
 * Cubes: one per 2x2x2 block of neighbouring samples; its corners are numbered c = dx + 2 dy + 4 dz.  Without a border there are
 * (X-1)(Y-1)(Z-1) cubes and cube (cx, cy, cz) has its corner 0 at sample (cx, cy, cz).  The linear cube index is cx + nx * (cy + ny * cz)
 * with nx, ny the cubes per axis.  Its tetrahedra, in this order, by corner: (0,1,3,7) (0,1,5,7) (0,2,3,7) (0,2,6,7) (0,4,5,7) (0,4,6,7).
 * The local vertices 0, 1, 2, 3 of a tetrahedron are its corners in that order, so a smaller local number is a smaller corner number
 * and a smaller linear sample index.
 * Class: a corner is above iff f >= level (closed, the planes' convention; -0.0 >= 0.0 is above), otherwise below.  A tetrahedron
 * with a corner that fails fabsf(f) <= FLT_MAX (a NaN or an infinity) emits nothing; the cube's other tetrahedra are not affected.
 * Case: 4 bits, bit j set iff local vertex j is above.
 * Vertex: on a tetrahedron edge (p, q), p < q, whose ends differ in class, always interpolated from the end a = p with the smaller
 * corner number to the other end b = q:  t = (level - fa) / (fb - fa),  P = pa + (pb - pa) * t per component, pa and pb the sample
 * positions above.  Every tetrahedron and every cube that shares a lattice edge therefore computes the same bits; no vertex is taken
 * from a neighbour's arithmetic.
 * Edges are numbered 0 = (0,1), 1 = (0,2), 2 = (0,3), 3 = (1,2), 4 = (1,3), 5 = (2,3) by local vertex.  Table, case: triangles of
 * three edge numbers each, triangle 0 then triangle 1 (a 2-2 split is a quad split along a fixed diagonal):
 *    0: --                  1: (0,2,1)             2: (0,3,4)             3: (1,3,4) (1,4,2)
 *    4: (1,5,3)             5: (2,5,3) (2,3,0)     6: (0,1,5) (0,5,4)     7: (2,5,4)
 *    8: (2,4,5)             9: (0,4,5) (0,5,1)    10: (3,5,2) (3,2,0)    11: (1,3,5)
 *   12: (1,2,4) (1,4,3)    13: (0,4,3)            14: (0,1,2)            15: --
 * The table is written for a tetrahedron of positive orientation.  Tetrahedra 1, 2 and 5 are mirror images: the second and third
 * vertex of each of their triangles change places.  flip = 1 makes them change places once more, in every tetrahedron.  With flip = 0
 * and positive cell components the geometric normal cross(v1 - v0, v2 - v0) points to the above side: a signed distance field that is
 * negative inside gives outward faces.  flip = 1 is for fields that are large inside, such as winding numbers.  (A negative component
 * of cell mirrors the lattice and with it the orientation.)
 * Order: ascending cube index (z, then y, then x), then tetrahedron 0..5, then the table's triangle 0..1: the same bytes on every run.
 * Record: a drt_iso_tri, 48 bytes, laid out as a drt_tri: v[3][3], then cube (the linear cube index), code = tetrahedron | case << 4,
 * and a zero word.  A fill's output can be handed to drt_renderer_overlap_triangles and its relatives as it stands.  The miss record
 * is cube = 0xffffffff and zeros everywhere else.
 * Border: NaN means none.  A finite border puts one virtual layer of samples with that value around the grid on all six sides, at
 * lattice indices -1 and dims[k], positioned by the same formula.  There are then (X+1)(Y+1)(Z+1) cubes, and cube (cx, cy, cz) has its
 * corner 0 at lattice index (cx-1, cy-1, cz-1).  With a border on the outside class every surface closes inside the padded grid,
 * whatever the field; without one a surface that reaches the grid's edge is open there.  Nothing of the padded field is materialised.
 * Rows: a row is the run of cubes along x for one (cy, cz), row = cy + ny * cz; counts[row] is the number of triangles in the row and
 * offsets holds rows + 1 values.  offsets / out / out_capacity / counts are exactly drt_renderer_plane_sections' segments with
 * "row" for "plane" and 48-byte records: the clamped capacity cap_r, the first cap_r records stored, the miss record in the rest of
 * the cap_r slots, nothing else in out written, counts[r] the total whether stored or not.  out is NULL iff out_capacity == 0: a pure
 * count, which does not read offsets (it may be NULL).  counts may be NULL in a fill; both out and counts NULL is DRT_ERR_INVALID.
 * Two passes give every triangle without a capacity guess: a count, an exclusive scan of the counts into offsets, a fill.
 * Checks, each DRT_ERR_INVALID before any device work, in this order: NULL r, field or grid; flip other than 0 or 1; out and counts
 * both NULL; out NULL without out_capacity 0 or the reverse; a fill without offsets; out 16-byte aligned and field, offsets and counts
 * 4-byte aligned; an infinite border; every dims[k] >= 2 (>= 1 with a border); the sample count and the cube count < 2^31; level
 * finite; lo and cell finite; a pending asynchronous batch; then field, offsets, out and counts must be device memory on the renderer's
 * device.  hip_stream NULL = the renderer's stream; the call only enqueues.  The framebuffer, accumulation, sample count, counters,
 * kernel info and kernel span are not touched.
 * What this is not: no vertex index buffer -- it is triangle soup with bit-equal shared positions, and drt_tri_edge_adjacency recovers
 * the connectivity; a sample exactly equal to level is above, t = 0 there, several edges yield the corner's own position, and
 * zero-area triangles with zero-length edges appear, which the adjacency marks -2 -- shift level by an ulp or accept them; no gradient
 * normals; marching tetrahedra emit roughly twice the triangles of marching cubes; the surface is that of the piecewise-linear
 * interpolant and is no better; no simplification, no smoothing and no dual or sharp-feature methods; no drt_group_* form and no
 * command line. */
typedef struct drt_grid { float lo[3]; float cell[3]; uint32_t dims[3]; } drt_grid;                       /* 36 B, host memory */
typedef struct drt_iso_tri { float v[3][3]; uint32_t cube; uint32_t code; uint32_t zero; } drt_iso_tri;   /* 48 B */
int           drt_renderer_isosurface(drt_renderer *r, const float *field, const drt_grid *grid, float level, float border, int32_t flip,
                                      const uint32_t *offsets, drt_iso_tri *out, uint32_t out_capacity, uint32_t *counts,
                                      void *hip_stream);

/* ---- vertex welding, vertex normals and smoothing (new; the map from the corners of a triangle soup to vertices, made on the device
 * and in integers, and the two scatters over it) ----
 * The three calls need no scene and no tree; they work on any triangles in device memory, drt_renderer_isosurface's output included.
 *
 * drt_renderer_weld -- the index buffer.  Input: n triangles at tris, `stride` bytes apart: 36 (float [N][3][3]) or 48 (drt_tri /
 * drt_iso_tri records; only the nine floats are read).  3 n < 2^31.  Corner c = 3 t + k is vertex k of triangle t.
 * Same vertex: two corners are the same vertex iff their three 32-bit words are equal as integers -- drt_tri_edge_adjacency's notion
 * of the same position, so the two tables always agree.  -0.0 and +0.0 are different vertices, NaNs are compared by their bits; there
 * is no tolerance and nothing is moved.
 * rep[c] is the smallest corner index with c's position.  Vertices are numbered in ascending rep, that is by first appearance.
 * Outputs: faces int32 [n][3], the vertex id of every corner; first int32 [V], the representative corner of each vertex; vertices
 * float [V][3], its position copied bit for bit (may be NULL); vertex_count, one device word that is always the total V.
 * capacity is the room in first and vertices, in vertices: 3 n always suffices.  A smaller capacity stores the first `capacity`
 * vertices only; faces and the count are still complete.  first is NULL iff capacity == 0.
 * The result depends on the input bytes alone: the same bytes on every run, in every launch shape.  (How: an insert-only hash table of
 * corner indices claimed by compare-and-swap and lowered by an integer minimum, a flag scan, a scatter; the hash decides nothing
 * that can be observed.  The restatement is a unique() over the 12-byte positions, reordered by first index.)  n == 0 stores V = 0.
 * Checks, each DRT_ERR_INVALID before any device work, in this order: NULL r or vertex_count; a stride other than 36 or 48; 3 n >= 2^31;
 * NULL tris or faces with n > 0; first NULL without capacity 0 or the reverse; vertices without first; every pointer 4-byte aligned;
 * a pending asynchronous batch; then every pointer must be device memory on the renderer's device.  The table and the flags are the
 * renderer's scratch, grown on demand; running out of device memory is DRT_ERR_DEVICE.
 *
 * drt_renderer_vertex_normals -- float [V][3] from vertices float [V][3], faces int32 [N][3] and a weight.  fp32 with one rounding
 * per operation, in the order written, unless float64 is named; cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x)
 * and dot(a, b) = a.x b.x + a.y b.y + a.z b.z, summed left to right.  The sums over a vertex's triangles are int64 fixed point, added
 * with integer atomics: the same bytes in any order.
 * Per triangle (v0, v1, v2): n = cross(v1 - v0, v2 - v0), l = sqrtf(dot(n, n)).  The triangle adds nothing if an index is outside
 * [0, V) (a bounds check, never a fault), if a coordinate of it is not finite, or if l is 0 or not finite.
 * DRT_NORMALS_ANGLE (0): u = n / l, three divisions.  At corner k, a = v[(k+1) % 3] - v[k], b = v[(k+2) % 3] - v[k] and
 * angle = atan2(l, dot(a, b)), the atan2 of the winding numbers above; its precondition y != 0 holds because l > 0.  For a finite x it
 * gives the interior angle; x = +inf (the dot product overflowed) gives 0 and x = -inf gives 3.14159265f; a NaN x (+inf - inf in the
 * dot product) gives a NaN angle, and a corner whose angle is not finite adds nothing.  Otherwise component j adds
 * (int64) trunc((double)(angle * u_j) * 2^28) to vertex faces[t][k]; angle * u_j is one fp32 product.
 * DRT_NORMALS_AREA (1): M is the largest |n_j| over all contributing triangles, e = floor(log2 M); every vertex of the triangle
 * gets (int64) trunc((double)n_j * 2^(28 - e)), the power of two applied in float64, which is exact.  M = 0 gives all zeros.
 * Result, in float64 and rounded once to fp32: x / sqrt(x x + y y + z z) with x, y, z the sums converted to float64 (the squares
 * summed left to right), and zeros if the length is 0 -- a vertex in no contributing triangle.
 * Checks, in this order: NULL r; a weight other than 0 or 1; V == 0 is a no-op; NULL vertices or out; NULL faces with N > 0; 4-byte
 * alignment; 3 N >= 2^31; V >= 2^31; a pending batch; device memory.
 *
 * drt_renderer_smooth_vertices -- Laplacian and Taubin smoothing: out float [V][3] from vertices, faces, `n_factors` factors in
 * host memory and an optional fixed uint8 [V] in device memory.  Step s uses f = factors[s]; |f| <= 1, else DRT_ERR_INVALID.
 * {0.5, 0.5, ...} is Laplacian smoothing, {0.5, -0.53, 0.5, -0.53, ...} Taubin's lambda | mu.  out may not alias vertices; the steps
 * between ping-pong in the renderer's scratch.  No factors: out is a copy of vertices.
 * A step over its input positions p:  M is the largest finite |coordinate| of p, e = floor(log2 M), k = 27 - e (M = 0: k = 0), and
 * q(x) = (int64) trunc((double)x * 2^k), so |q| < 2^28 in every step.  A triangle with an index outside [0, V) or a coordinate that
 * is not finite adds nothing.  Every other triangle (a, b, c) adds q(p_b) + q(p_c) to acc[a] per component, and cyclically for b and
 * c, and adds 2 to cnt of each; a triangle that names a vertex twice is not special-cased.  Update, in float64 with one rounding
 * per operation, then one rounding to fp32:  m = (double)acc / ((double)cnt * 2^k),  p' = (float)((double)p + (double)f * (m - (double)p)).
 * A vertex keeps its bits if cnt = 0, if fixed is set for it, or if a coordinate of it is not finite.  (With f = 0 a coordinate -0.0
 * becomes +0.0 where m - p is not negative: that is the formula.)  Shared vertices stay shared because there is one position per id:
 * a smoothed watertight mesh is watertight by construction.
 * Checks, in this order: NULL r; NULL factors with n_factors > 0; |f| > 1 or a NaN; V == 0 is a no-op; then
 * drt_renderer_vertex_normals' from "NULL vertices or out" to "V >= 2^31"; out overlapping vertices; a pending batch; device memory.
 *
 * All three: hip_stream NULL = the renderer's stream; the call only enqueues, in order with the other queries (the same event),
 * because the calls share the renderer's scratch; legal on a sharded renderer; the framebuffer, accumulation, sample count, counters,
 * kernel info and kernel span are not touched.
 * What this is not: no cotangent weights -- the umbrella operator shrinks and slides vertices along the surface; no feature
 * preservation; no boundary detection -- pass fixed, for instance from drt_renderer_boundary_loops; no simplification; no
 * vertex-to-triangle lists; no device edge adjacency from faces; welding is by bit-equal positions only, with no tolerance; no
 * drt_group_* form and no command line. */
#define DRT_NORMALS_ANGLE 0
#define DRT_NORMALS_AREA 1
int           drt_renderer_weld(drt_renderer *r, const void *tris, uint32_t n, uint32_t stride, int32_t *faces, int32_t *first,
                                float *vertices, uint32_t capacity, uint32_t *vertex_count, void *hip_stream);
int           drt_renderer_vertex_normals(drt_renderer *r, const float *vertices, uint32_t n_vertices, const int32_t *faces,
                                          uint32_t n_tris, int32_t weight, float *out, void *hip_stream);
int           drt_renderer_smooth_vertices(drt_renderer *r, const float *vertices, uint32_t n_vertices, const int32_t *faces,
                                           uint32_t n_tris, const float *factors, uint32_t n_factors, const uint8_t *fixed, float *out,
                                           void *hip_stream);

/* ---- mesh simplification (new; vertex clustering on a grid with a mean or a quadric-optimal representative: one map from vertices
 * to clusters, made on the device and in integers as the weld's map is, and the sums over it) ----
 * drt_renderer_simplify needs no scene and no tree; it works on any indexed mesh in device memory, drt_renderer_weld's output
 * included: vertices float [V][3], faces int32 [N][3].  Rossignac-Borrel cells with Lindstrom's placement: every grid cell that holds
 * vertices becomes one vertex, and the triangles that still have three different vertices survive.  The result does not depend on
 * any order of operations; there is no edge collapse.
 * fp32 with one rounding per operation, in the order written, unless float64 is named; cross and dot as for the vertex normals above.
 * Grid: the drt_grid POD of the isosurface call, read on the host: lo finite, cell finite and greater than 0, dims at least 1 and
 * X Y Z < 2^31, with (X, Y, Z) = dims.
 * Cell of a vertex: per axis f = (p - lo) / cell, two fp32 operations.  The vertex is in the grid iff its three coordinates are
 * finite and 0 <= f < (float)dims on every axis; then i = (int)f (i < dims follows, also where (float)dims is rounded) and its key is
 * ix + X (iy + Y iz).  Nothing is clamped.
 * Clusters: in-grid vertices with the same key are one cluster; every other vertex -- outside the grid, or not finite -- is a cluster
 * of its own, so a grid over part of a mesh simplifies that part and leaves the rest alone.  first[c] is the smallest input vertex in
 * cluster c; clusters are numbered in ascending first; cluster[v] is total: every vertex gets an id.
 * Position of a cluster: a cluster with one member copies that member's 12 bytes.  Any other cluster lies in a cell (ix, iy, iz) with
 * the centre g = lo + ((float)i + 0.5f) * cell per component, the grid-sample rule above, and a member or a corner at p has
 * r = (p - g) / cell per component.
 * Mean: acc_a += (int64) trunc((double)r_a * 2^30) per component and cnt += 1 per member;  m_a = (double)acc_a / ((double)cnt * 2^30).
 * Quadric: per triangle (v0, v1, v2): n = cross(v1 - v0, v2 - v0), l = sqrtf(dot(n, n)), u = n / l, three divisions.  A triangle
 * contributes iff its indices are inside [0, V) (a bounds check, never a fault), its nine coordinates are finite and l is finite and
 * greater than 0.  L is the largest l of the contributing triangles, e = floor(log2 L), and w = (float)((double)l * 2^-(e+1)): the power
 * of two applied in float64, which is exact, then one rounding.  Each corner k of a contributing triangle whose vertex is in the grid
 * and in a cluster c with more than one member adds, with r taken at that corner and s = dot(u, r):
 *   (int64) trunc((double)((w * u_i) * u_j) * 2^30) to A_ij[c] for the six entries ij = 00, 01, 02, 11, 12, 22, and
 *   (int64) trunc((double)((w * u_i) * s) * 2^30) to b_i[c].
 * A triangle with two corners in one cluster is not special-cased: each corner adds.  All sums are int64, added with integer
 * atomics: the same bytes in any order.
 * Finish, in float64 with one rounding per operation; A_ij, b_i below are the sums converted to float64:
 *   tr = (A00 + A11) + A22,  lam = tr * 2^-10,  a00 = A00 + lam, a11 = A11 + lam, a22 = A22 + lam, a01 = A01, a02 = A02, a12 = A12,
 *   d_i = b_i + lam * m_i,
 *   c0 = a11 * a22 - a12 * a12,  c1 = a01 * a22 - a12 * a02,  c2 = a01 * a12 - a11 * a02,  det = (a00 * c0 - a01 * c1) + a02 * c2,
 *   e0 = d1 * a22 - a12 * d2,  e1 = d1 * a12 - a11 * d2,  e2 = a01 * d2 - d1 * a02,
 *   x0 = ((d0 * c0 - a01 * e0) + a02 * e1) / det,  x1 = ((a00 * e0 - d0 * c1) + a02 * e2) / det,  x2 = ((d0 * c2 - a00 * e1) - a01 * e2) / det:
 * Cramer's rule for (A + lam I) x = b + lam m, the minimiser of the summed squared plane distances, drawn to the mean where the planes
 * leave it free.  If tr == 0, or any x_a is not finite, or any |x_a| > 0.5, then x = m: an optimum outside its cell is not trusted.
 * DRT_SIMPLIFY_MEAN (0) is x = m throughout and reads no triangle for the positions; DRT_SIMPLIFY_QUADRIC (1) is the above.
 * Position: (float)((double)g_a + x_a * (double)cell_a).
 * Triangles: input triangle t survives iff its three indices are inside [0, V) and its three cluster ids differ pairwise.  Survivors
 * keep input order; out_faces[m] holds the cluster ids and source[m] = t, so per-triangle attributes can follow.  Duplicate triangles
 * are not removed, and that makes the boundary identity exact: a closed oriented input gives an output in which every directed edge
 * (a, b) appears as often as (b, a).
 * Outputs: cluster int32 [V]; out_vertices float [C][3] and first int32 [C]; out_faces int32 [M][3] and source int32 [M]; counts, two
 * device words that are always complete: C, then M.  Only the first vertex_capacity clusters and the first tri_capacity triangles
 * are stored (V and N always suffice); cluster and counts are always complete.  out_vertices and first are NULL iff vertex_capacity
 * == 0, out_faces and source are NULL iff tri_capacity == 0.
 * Consequences: a grid so fine that every cluster is a singleton returns vertices and the surviving faces byte for byte; the result
 * depends on the input bytes alone: the same bytes on every run, in every launch shape.  (How: an insert-only hash table of vertex
 * indices keyed by the cell, claimed by compare-and-swap and lowered by an integer minimum, a flag scan, a scatter -- the weld's
 * shape; the hash decides nothing that can be observed.)
 * Checks, each DRT_ERR_INVALID before any device work, in this order: NULL r, grid or counts; NULL vertices or cluster with V > 0; NULL
 * faces with N > 0; out_vertices or first NULL without vertex_capacity 0 or the reverse; out_faces or source NULL without tri_capacity
 * 0 or the reverse; a placement other than 0 or 1; lo not finite; cell not finite or not greater than 0; a dims below 1; X Y Z >= 2^31;
 * V >= 2^31; 3 N >= 2^31.  V == 0 is a no-op that stores C = M = 0: of the checks below only those of counts apply to it.  Then every
 * pointer 4-byte aligned; an output overlapping vertices or faces; a pending asynchronous batch; then every pointer must be device
 * memory on the renderer's device.  The table, the keys and the sums are the renderer's scratch, grown on demand (96 bytes of sums
 * per input vertex with quadric placement, 24 with mean); running out of device memory is DRT_ERR_DEVICE.
 * hip_stream NULL = the renderer's stream; the call only enqueues, in order with the other queries (the same event), because it
 * shares the renderer's scratch; legal on a sharded renderer; the framebuffer, accumulation, sample count, counters, kernel info and
 * kernel span are not touched.
 * What this is not: no edge collapse and no error-bounded or target-count simplification -- the grid is the only control; duplicate
 * and opposite triangle pairs are not removed; clustering can create non-manifold edges and vertices where a cell holds two sheets of
 * a surface, and they are not repaired; no attribute quadrics, no interpolated normals or uvs -- source says which input triangle an
 * output triangle was; no adaptive (octree) cells; the cross product and dot(n, n) are fp32, so triangles with edges below about
 * 2^-37 or above about 2^31 under- or overflow there and contribute nothing, and a cluster without contributions gets the mean; no
 * drt_group_* form and no command line. */
#define DRT_SIMPLIFY_MEAN 0
#define DRT_SIMPLIFY_QUADRIC 1
int           drt_renderer_simplify(drt_renderer *r, const float *vertices, uint32_t n_vertices, const int32_t *faces, uint32_t n_tris,
                                    const drt_grid *grid, int32_t placement, int32_t *cluster, float *out_vertices, int32_t *first,
                                    uint32_t vertex_capacity, int32_t *out_faces, int32_t *source, uint32_t tri_capacity,
                                    uint32_t *counts, void *hip_stream);

/* ---- device edge adjacency (new; drt_scene_edge_adjacency's and drt_tri_edge_adjacency's table made on the device, for triangle
 * soups, index buffers and the uploaded scene, with the numbering of the undirected edges and the boundary vertices) ----
 * drt_renderer_tri_adjacency and drt_renderer_face_adjacency need no scene and no tree.  Half-edge h = 3 t + e runs from corner e to
 * corner (e + 1) % 3 of triangle t.  An END of a half-edge is
 *   by position (drt_renderer_tri_adjacency): the three 32-bit words of the corner at tris + t * stride + 12 e, stride 36 (float
 *     [N][3][3]) or 48 (drt_tri), compared as integers -- drt_tri_edge_adjacency's rule exactly: -0.0 and +0.0 differ, NaNs are compared
 *     by their bits, there is no tolerance;
 *   by index (drt_renderer_face_adjacency): the int32 word faces[3 t + e], compared as an integer.  No vertex array is read, so no
 *     value is out of range.
 * Two half-edges are in one GROUP iff they have the same unordered pair of ends.  The rule, for both kinds of end:
 *   a half-edge whose two ends are equal (zero length) gets -2 and is in no group;
 *   a group of one half-edge gets -1;
 *   a group of exactly two that run in opposite directions (the start of one is the end of the other) are each other's twins:
 *     adj[h] = the other half-edge;
 *   every other group -- three or more, two that run the same way -- gets -2.
 * adj is int32 [3 N], the same bytes as drt_tri_edge_adjacency's table of the same triangles for every input.
 * Edge numbering (optional: edge, half_edge and edge_count are NULL together): every group is one undirected edge; its representative
 * is its smallest half-edge; edges are numbered in ascending representative, which is by first appearance.  edge int32 [3 N] is each
 * half-edge's edge id, -1 for a zero-length one; half_edge int32 [capacity] is the representative of each of the first `capacity`
 * edges (3 N always suffices; half_edge is NULL iff capacity == 0); *edge_count = E, stored whether or not capacity held all edges.
 * With V from drt_renderer_weld this gives V - E + F without a host pass.
 * drt_renderer_boundary_vertices: out uint8 [n_vertices] is zeroed, then out[v] = 1 iff a half-edge with adj == -1 starts or ends at
 * v, i.e. v is faces[3 t + e] or faces[3 t + (e + 1) % 3] of such a half-edge 3 t + e.  With DRT_BOUNDARY_BAD_EDGES (flag bit 0)
 * adj == -2 counts as well.  A triangle with an index outside [0, n_vertices) is skipped (a bounds check, never a fault).
 * The uploaded scene's table (drt_renderer_chain_sections, _chain_intersections, _shell_labels, _boundary_loops,
 * _edge_adjacency) is made the same way from the host scene's positions in tree order by the first such call after an upload; it is
 * the same bytes as drt_scene_edge_adjacency, and a device refit leaves it alone.  DRT_ADJACENCY=host in the environment when the
 * renderer is created selects the host's sort instead.  drt_renderer_adjacency_route: 0 = no table since the last upload, 1 = it was
 * made on the host, 2 = on the device.
 * Consequences: the result depends on the input bytes alone: the same bytes on every run, in every launch shape.  (How: the weld's
 * insert-only hash table, here of half-edge indices keyed by the unordered pair, claimed by compare-and-swap and lowered by an
 * integer minimum; a second integer minimum finds the second member of a group; a flag scan numbers the edges.  No lane waits for
 * another; the hash decides nothing that can be observed.)
 * Checks, each DRT_ERR_INVALID before any device work, in this order: NULL r; a stride other than 36 or 48; 3 N >= 2^31; N == 0 is a
 * no-op that touches nothing, edge_count included; NULL tris / faces or adj; edge NULL without edge_count NULL or the reverse;
 * half_edge or a capacity without edge; half_edge NULL without capacity 0 or the reverse; every pointer 4-byte aligned; a pending
 * asynchronous batch; then every pointer must be device memory on the renderer's device.  drt_renderer_boundary_vertices: NULL r; a
 * flag bit other than bit 0; 3 N >= 2^31; n_vertices >= 2^31; n_vertices == 0 is a no-op; NULL out; NULL faces or adj with N > 0;
 * faces and adj 4-byte aligned; a pending batch; device memory.  The table and two words per half-edge are the renderer's scratch,
 * shared with the welding calls and grown on demand (48 to 72 bytes per triangle); running out of device memory is DRT_ERR_DEVICE.
 * hip_stream NULL = the renderer's stream; the calls only enqueue, in order with the other queries (the same event), because they
 * share the renderer's scratch; legal on a sharded renderer; the framebuffer, accumulation, sample count, counters, kernel info and
 * kernel span are not touched.
 * What this is not: no vertex-to-triangle lists; no tolerance -- ends that differ in one bit are different ends; no orientation
 * repair -- two triangles that run the same way along an edge get -2 and stay so; no drt_group_* form and no command line. */
#define DRT_BOUNDARY_BAD_EDGES 1u
int           drt_renderer_tri_adjacency(drt_renderer *r, const void *tris, uint32_t n, uint32_t stride, int32_t *adj, int32_t *edge,
                                         int32_t *half_edge, uint32_t capacity, uint32_t *edge_count, void *hip_stream);
int           drt_renderer_face_adjacency(drt_renderer *r, const int32_t *faces, uint32_t n, int32_t *adj, int32_t *edge,
                                          int32_t *half_edge, uint32_t capacity, uint32_t *edge_count, void *hip_stream);
int           drt_renderer_boundary_vertices(drt_renderer *r, const int32_t *faces, const int32_t *adj, uint32_t n_tris,
                                             uint32_t n_vertices, uint32_t flags, uint8_t *out, void *hip_stream);
int           drt_renderer_adjacency_route(const drt_renderer *r);

/* ---- mesh subdivision (new; one level of Loop or midpoint refinement of an indexed mesh, on the connectivity above: the odd vertex
 * of edge e is vertex V + e, so nothing is sorted and no host pass is needed) ----
 * drt_renderer_subdivide needs no scene and no tree; it works on any indexed mesh in device memory, drt_renderer_weld's and
 * drt_renderer_simplify's output included: vertices float [V][3], faces int32 [N][3].  One call is one level: every triangle
 * becomes four.  Callers loop for more levels.
 * Topology, identical for both schemes.  The connectivity is drt_renderer_face_adjacency's of faces -- by index, with the edges
 * numbered: adj, edge and half_edge below are its outputs and E is its edge count; next(h) is the half-edge after h in its triangle,
 * 3 t + (e + 1) % 3 for h = 3 t + e.  Even vertices keep their ids 0 ... V - 1; the odd vertex of edge e is V + e;
 * *vertex_count = V + E always.  Only the first vertex_capacity vertices are stored in out_vertices and parents (V + 3 N always
 * suffices); out_vertices and parents are NULL iff vertex_capacity == 0, and parents alone may be NULL.
 * m(h) = V + edge[h] if edge[h] >= 0, otherwise faces[h]: an index edge of zero length has no new vertex.  out_faces is int32
 * [4 N][3], always complete, with no compaction: for t = (a, b, c) and m0 = m(3 t), m1 = m(3 t + 1), m2 = m(3 t + 2),
 *   child 4 t + 0 = (a, m0, m2),  child 4 t + 1 = (b, m1, m0),  child 4 t + 2 = (c, m2, m1),  child 4 t + 3 = (m0, m1, m2).
 * Orientation is kept; child k < 3 starts at corner k; the source triangle of child j is j >> 2.  Out-of-range indices are copied
 * as they are (the children read no position), and nothing faults.
 * parents is int32 [V'][2]: (v, v) for an even vertex; for the odd vertex V + e, with h = half_edge[e], (faces[h], faces[next(h)]):
 * the ends of the representative half-edge, in that order.
 * Consequences: a closed oriented manifold input gives a closed oriented manifold output, adj >= 0 everywhere;
 * V' - E' + F' = V - E + F; a same-way pair, a fan or a boundary stays one in the output.
 * Positions: float64 with one rounding per operation, in the order written, then one rounding to fp32.  An edge is USABLE iff both
 * ends of its representative half-edge are inside [0, V) (a bounds check, never a fault) and all six coordinates are finite.  The odd
 * vertex of an unusable edge is three words 0x7FC00000.  pa and pb below are a coordinate of the two ends.
 * DRT_SUBDIVIDE_MIDPOINT (0): even vertices copy their 12 bytes; an odd vertex is (float)(((double)pa + (double)pb) * 0.5), the same
 * bits whichever half-edge represents the edge.
 * DRT_SUBDIVIDE_LOOP (1): an edge is INTERIOR iff its representative h has adj[h] >= 0; every other edge (-1 or -2: boundary, fan,
 * same-way pair) is a CREASE.  Interior odd vertex: c and d are the corners opposite h and opposite adj[h] -- faces[next(next(h))] and
 * the same of adj[h] -- and the position is (float)(((double)pa + (double)pb) * 0.375 + ((double)pc + (double)pd) * 0.125); if c or d
 * is out of range or not finite, the midpoint.  A crease odd vertex is the midpoint.
 * Even vertices need sums over neighbours; these are int64 fixed point added with integer atomics, exactly
 * drt_renderer_smooth_vertices' quantisation: M is the largest finite |coordinate| over the input vertices, e = floor(log2 M),
 * k = 27 - e (M = 0: k = 0), q(x) = (int64) trunc((double)x * 2^k).  One pass over the EDGES, not the half-edges, so an edge counts
 * once however many triangles share it: each usable edge (a, b) adds q(pb) to acc[a] and q(pa) to acc[b], in the interior or the
 * crease set of sums according to its kind, and adds 1 to the matching count, n_int or n_cr, of each end.  Unusable edges add nothing.
 * Finish per vertex, with S = (double)acc * 2^-k per coordinate:
 *   a coordinate that is not finite, or n_cr == 0 && n_int == 0: the vertex keeps its bits;
 *   n_cr == 0: beta = (n_int == 3) ? 0.1875 : 0.375 / (double)n_int (Warren's weights),
 *     p' = (float)((double)p + beta * (S_int - (double)n_int * (double)p));
 *   n_cr == 2: p' = (float)((double)p + 0.125 * (S_cr - 2.0 * (double)p)); interior edges are ignored;
 *   any other n_cr (a dart, a corner where three creases meet, a non-manifold vertex): the vertex keeps its bits.
 * The result depends on the input bytes alone: the same bytes on every run, in every launch shape.  (How: the adjacency's integers,
 * integer sums, and float64 operations that are each rounded once; the hash decides nothing that can be observed.)
 * Checks, each DRT_ERR_INVALID before any device work, in this order: NULL r or vertex_count; a scheme other than 0 or 1;
 * 3 N >= 2^31; V + 3 N >= 2^31; 12 N >= 2^31.  N == 0 stores *vertex_count = V, copies the stored vertices -- with (v, v) in parents --
 * and is otherwise a no-op; the checks below apply to it as far as they name something it touches.  NULL vertices with V > 0; NULL
 * faces or out_faces with N > 0; out_vertices NULL without vertex_capacity 0 or the reverse; parents without out_vertices; every
 * pointer 4-byte aligned; an output overlapping vertices or faces; a pending asynchronous batch; then every pointer must be device
 * memory on the renderer's device.  The adjacency's table and outputs, the counts and the sums are the renderer's scratch, shared
 * with the welding calls and grown on demand (84 to 108 bytes per triangle, and 56 per vertex with Loop); running out of device
 * memory is DRT_ERR_DEVICE.
 * hip_stream NULL = the renderer's stream; the call only enqueues, in order with the other queries (the same event), because it
 * shares the renderer's scratch; legal on a sharded renderer; the framebuffer, accumulation, sample count, counters, kernel info and
 * kernel span are not touched.
 * What this is not: no Catmull-Clark, Butterfly or sqrt(3); no user crease tags or sharpness -- the creases are the edges that are
 * not a twin pair; no limit-surface projection or limit normals; no adaptive refinement; no attribute interpolation beyond parents
 * and the child order; no drt_group_* form and no command line. */
#define DRT_SUBDIVIDE_MIDPOINT 0
#define DRT_SUBDIVIDE_LOOP 1
int           drt_renderer_subdivide(drt_renderer *r, const float *vertices, uint32_t n_vertices, const int32_t *faces, uint32_t n_tris,
                                     int32_t scheme, float *out_vertices, int32_t *parents, uint32_t vertex_capacity,
                                     int32_t *out_faces, uint32_t *vertex_count, void *hip_stream);

/* ---- first-hit guide buffers and the a-trous denoiser (new; the reference's TODO list, RayGen.cuh:13-21, starts with "DLSS 3.5
 * like features") ----
 * drt_renderer_render_guides writes one drt_guide per pixel x + y * width (row 0 = bottom, as the framebuffer) for frame
 * `frame_index` (>= 1): the renderer's primary ray of that pixel and frame (uv = ((float)x / width) * 2 - 1, ((float)y / height)
 * * 2 - 1, seed = (x + y * width) * frame_index, Camera::GetRay with jitter and defocus), traced as drt_renderer_trace_rays
 * traces it with tmin 0 and tmax FLT_MAX (TraceRay, bit for bit).  On a hit: albedo = the first hit's material albedo or texel
 * (the ALBEDO debug view), normal = the face normal turned against the ray (the NORMAL debug view), t and prim as
 * drt_renderer_trace_rays returns them.  On a miss: albedo = the sky term the ALBEDO debug view shows (settings' sky colour and
 * intensity), normal = 0, t = FLT_MAX, prim = -1.  A component is stored as the views store it, added to a zeroed sum (-0 reads +0).
 * `guides` is a 16-byte aligned device pointer on the renderer's device; hip_stream NULL = the renderer's stream; the call only
 * enqueues, in order with the renderer's ray queries, and uploads the scene as rendering does.
 * drt_renderer_denoise filters the current framebuffer c_0 (RGB; display-referred: every sample is tone-mapped) with the guides of
 * frame 1: passes i = 0 .. iterations-1, step s = 2^i, h = {1/16, 1/4, 3/8, 1/4, 1/16}; for each pixel p, over b then a in 0..4,
 * q = (clamp(x + (a-2)s, 0, W-1), clamp(y + (b-2)s, 0, H-1)),
 *   e = |c_i(p)-c_i(q)|^2 * 2^i / sigma_color^2 + |n(p)-n(q)|^2 / sigma_normal^2 + |alb(p)-alb(q)|^2 / sigma_albedo^2,
 *   w = h[a] h[b] expf(-e),  c_{i+1}(p) = sum w c_i(q) / sum w  (squared distances summed over x, y, z in that order).
 * The result (c_K, the input's alpha; iterations 0 = a copy of the framebuffer) lands in a renderer-owned float4[width*height]
 * buffer, allocated by the first call and freed by resize and destroy.  Blocking; *delta_ms = device time of guides + filter.
 * Neither call touches the accumulation buffer, the framebuffer, the sample count, the counters, kernel info or kernel span.
 * DRT_ERR_INVALID: a NULL argument, frame_index 0, no frame size, a misaligned / host / other-device `guides`, iterations outside
 * [0, 10], a sigma not finite or not > 0, a pending drt_renderer_render_batch_async batch.  DRT_ERR_UNSUPPORTED: a sharded
 * renderer (world > 1: the filter needs its neighbours' rows), a tree deeper than 64 levels. */
typedef struct drt_guide { float albedo[3]; float t; float normal[3]; int32_t prim; } drt_guide;                  /* 32 B */
int           drt_renderer_render_guides(drt_renderer *r, const drt_camera *cam, const drt_scene *scene, uint32_t frame_index,
                                         drt_guide *guides, void *hip_stream);
typedef struct drt_denoise_params { int32_t iterations; float sigma_color, sigma_normal, sigma_albedo; } drt_denoise_params;
void          drt_default_denoise_params(drt_denoise_params *out);                                           /* 5, 0.5, 0.1, 0.1 */
int           drt_renderer_denoise(drt_renderer *r, const drt_camera *cam, const drt_scene *scene, const drt_denoise_params *p,
                                   float *delta_ms);
int           drt_renderer_read_denoised_rgba32f(drt_renderer *r, float *dst, size_t dst_floats);        /* width*height*4 */
void         *drt_renderer_device_denoised(drt_renderer *r);              /* device float4[width*height], NULL before the first denoise */

/* ---- temporal reprojection and the variance-guided a-trous filter (new; SVGF, Schied et al. 2017, on the guides above) ----
 * drt_renderer_temporal_denoise carries a per-pixel history from call to call.  One call, for the current framebuffer c (RGB,
 * display-referred, whatever has been rendered since the last reset) and camera `cam`, W x H pixels p = (x, y), row 0 = bottom.
 * All arithmetic is fp32, one rounding per operation, in the order written (sums left to right); dot(a, b) = a.x b.x + a.y b.y +
 * a.z b.z, normalize(v) = v * (1 / sqrtf(dot(v, v))), lum(c) = 0.2126f c.r + 0.7152f c.g + 0.0722f c.b.
 * (a) g = the guides of frame 1 for `cam` (drt_renderer_render_guides: what drt_renderer_denoise uses).
 * (b) Reproject and accumulate.  l = lum(c(p)).  The pixel has NO history on the first call after a reset and where g.prim < 0.
 *   Otherwise u = ((float)x / W) * 2 - 1, v = ((float)y / H) * 2 - 1, d0 = normalize(fwd_focus + u * horizontal + v * vertical)
 *   (Camera::GetRay's direction without jitter and defocus: the jitter is +-0.00175 in uv, +-1.7 pixels at 1080p, and reprojecting
 *   the jittered hit would blur a still camera's image), P = cam_pos + d0 * g.t(p).  With the PREVIOUS call's camera (position
 *   pos', forward f' = normalize(forward), right' = normalize(cross(f', (0,1,0))), up' = cross(right', f'), focus' = focus_dist,
 *   plane_h' = 2 * tanf((vfov_rad / 2) / 2) * focus', plane_w' = plane_h' * ((float)W / (float)H): Camera.cu:82's, the tan(vfov/4)
 *   quirk included): pv = P - pos', z = dot(pv, f'); no history unless z > 0;
 *     su = (dot(pv, right') * focus') / (z * plane_w'),  sv = (dot(pv, up') * focus') / (z * plane_h'),
 *     fx = ((su + 1) * 0.5f) * W,  fy = ((sv + 1) * 0.5f) * H;  no history unless -1 < fx < W and -1 < fy < H.
 *   Taps j = 0, 1 (outer), i = 0, 1 (inner) at q = (floorf(fx) + i, floorf(fy) + j), weight w = wx_i * wy_j with wx_1 = fx -
 *   floorf(fx), wx_0 = 1 - wx_1 (wy alike).  A tap is valid iff q is inside the image, its stored N >= 1 (every record a call stores
 *   has: the test is "a previous call exists"), its stored prim == g.prim(p) and dot(n_stored(q), g.normal(p)) >= normal_cos_min.
 *   On a planar triangle the same prim through nearly the same pixel is the same surface point: prim equality is the
 *   disocclusion test, and it holds across refits, which keep the triangle order.  Over the valid taps in tap order, from 0:
 *   S += w, hc += colour(q) * w, hN += N(q) * w, h1 += m1(q) * w, h2 += m2(q) * w.
 *     S >= 0.01f: N = fminf(floorf(hN / S + 0.5f) + 1, (float)max_history), a = fmaxf(1 / N, alpha_min),
 *                 colour = (hc / S) * (1 - a) + c * a,  m1 = (h1 / S) * (1 - a) + l * a,  m2 = (h2 / S) * (1 - a) + (l * l) * a.
 *     else:       N = 1, colour = c, m1 = l, m2 = l * l.
 *   Variance: N >= 4: fmaxf(0, m2 - m1 * m1).  N < 4: over the 7x7 window (dy = -3..3 outer, dx inner, coordinates clamped to the
 *   image) of THIS call's integrated colour, the pixels q with g.prim(q) == g.prim(p): s1 += lum(colour(q)), s2 += lum * lum, n += 1;
 *   variance = fmaxf(0, s2 / n - (s1 / n) * (s1 / n)) * (4 / N).
 *   Stored in the other half of a ping-pong history: (colour, N), (g.normal, g.prim), (m1, m2, variance, S); the camera on the host.
 *   No transcendental: with -ffp-contract=off and correctly rounded / and sqrtf this stage is reproducible bit for bit.
 * (c) Variance-guided a-trous: c_0 = the integrated colour, var_0 = the variance of (b); passes i = 0 .. iterations-1 with the
 *   taps, h, clamping, normal and albedo terms of drt_renderer_denoise.  gv_i(p) = the 3x3 Gaussian of var_i (dy = -1..1 outer,
 *   dx inner, clamped, weights {0.25, 0.5, 0.25}[dy] * {0.25, 0.5, 0.25}[dx], summed from 0), r = 1 / (sigma_luma * sqrtf(gv_i(p))
 *   + 1e-4f),
 *     e = fabsf(lum(c_i(p)) - lum(c_i(q))) * r + |n(p)-n(q)|^2 * (1 / sigma_normal^2) + |alb(p)-alb(q)|^2 * (1 / sigma_albedo^2),
 *     w = h[a] h[b] expf(-e),  c_{i+1}(p) = sum w c_i(q) / sum w,  var_{i+1}(p) = sum (w * w) var_i(q) / ((sum w) * (sum w)).
 *   The result (c_K, alpha 1; iterations 0 = the integrated colour itself) lands in the renderer's denoised target:
 *   drt_renderer_read_denoised_rgba32f and drt_renderer_device_denoised read it.  The history keeps the UNFILTERED colour.
 * Side effects: none beyond the history and the denoised target (accumulation buffer, framebuffer, sample count, counters, kernel
 * info and span untouched).  The history is allocated by the first call and freed by resize, destroy and
 * drt_renderer_temporal_reset (the next call then starts at N = 1).  Blocking; *delta_ms = device time of all stages.
 * drt_renderer_read_temporal / drt_renderer_device_temporal: which 0 = (colour rgb, N), 1 = (m1, m2, variance, S) of the last call,
 * float4[width * height].
 * DRT_ERR_INVALID: a NULL argument, no frame size, a pending drt_renderer_render_batch_async batch, iterations outside [0, 10],
 * max_history < 1, alpha_min outside [0, 1], a normal_cos_min or sigma that is not finite, a sigma not > 0, `which` outside 0..1, a
 * too short dst, a read before the first call.  DRT_ERR_UNSUPPORTED: a sharded renderer (world > 1), a tree deeper than 64 levels.
 * Geometry that a drt_renderer_refit moved between two calls is followed when drt_renderer_track_motion is on (the section
 * below: P and the normal test of (b) are replaced per pixel, everything else stays).  Out of scope: motion through a host-side
 * drt_scene_refit and re-upload (such triangles reproject as if they were static: reset the history or accept it); feeding the
 * filtered colour back into the history; drt_group. */
typedef struct drt_temporal_params {
    int32_t iterations;      /* a-trous passes, 0..10, default 5 */
    int32_t max_history;     /* history length cap, >= 1, default 32 */
    float   alpha_min;       /* floor of the blend weight, [0, 1], default 0 */
    float   normal_cos_min;  /* a tap is valid only if dot(n_prev, n_cur) >= this, default 0.9 */
    float   sigma_luma, sigma_normal, sigma_albedo;   /* default 4, 0.1, 0.1 */
} drt_temporal_params;
void          drt_default_temporal_params(drt_temporal_params *out);
int           drt_renderer_temporal_denoise(drt_renderer *r, const drt_camera *cam, const drt_scene *scene,
                                            const drt_temporal_params *p, float *delta_ms);
int           drt_renderer_temporal_reset(drt_renderer *r);               /* drop the history; the next call starts at N = 1 */
int           drt_renderer_read_temporal(drt_renderer *r, int32_t which, float *dst, size_t dst_floats);
void         *drt_renderer_device_temporal(drt_renderer *r, int32_t which);     /* device float4[width*height], NULL before the first call */

/* ---- motion vectors: the temporal filter follows refitted geometry (new; opt-in, the reference has neither) ----
 * drt_renderer_track_motion(r, 1): from now on drt_renderer_refit copies this renderer's device TriHot records (csrc/device_scene.hpp:
 * v0, e1 = v1 - v0, e2 = v2 - v0, face normal fn; 48 B per triangle) into a renderer-owned SNAPSHOT before its kernels run, on
 * the refit's stream, but only if the snapshot is not ARMED; the copy arms it.  Several refits between two temporal calls thus
 * keep the oldest state.  drt_renderer_temporal_denoise disarms it at the end of its stage (b), drt_renderer_motion_advance
 * disarms it at once ("the geometry as it is now is the PREVIOUS geometry from here on": for callers that feed the motion buffer
 * to a filter of their own); the buffer is kept for reuse.  It is dropped whenever the renderer's device copy of the scene is
 * uploaded again (the scene's revision moved, another scene, a failed refit), by drt_renderer_track_motion(r, 0) and by destroy.
 * A host-side drt_scene_refit moves the revision: the re-upload drops the snapshot and every pixel reprojects as static.
 * Default 0: every call launches exactly the kernels it launches without this section, and no memory is added.
 * The rule.  fp32, one rounding per operation, in the order written; dot and normalize as above.  For a pixel with k = g.prim >= 0
 * and P = cam_pos + d0 * g.t of stage (b), (v0, e1, e2, fn) = the current record k, (v0', e1', e2', fn') = the snapshot's record k:
 *   STATIC rule -- no armed snapshot, or the nine words v0, e1, e2 are bitwise equal to v0', e1', e2':  P' = P, and a tap is tested
 *     with dot(n_stored(q), g.normal(p)) >= normal_cos_min.  Stage (b) exactly as written above.
 *   MOVED rule -- otherwise:  w = P - v0, d11 = dot(e1, e1), d12 = dot(e1, e2), d22 = dot(e2, e2), w1 = dot(w, e1), w2 = dot(w, e2),
 *     den = d11 * d22 - d12 * d12.  If not den > 0 (zero area, NaN): the static rule.  Else
 *     b1 = (d22 * w1 - d12 * w2) / den,  b2 = (d11 * w2 - d12 * w1) / den,  P' = (v0' + e1' * b1) + e2' * b2,
 *     n' = dot(fn, g.normal(p)) < 0 ? -fn' : fn'  (the previous face normal on the side the guide's normal is on), and a tap is
 *     tested with dot(n_stored(q), n') >= normal_cos_min.
 *   P' replaces P in pv = P' - pos'; projection, taps, prim equality, sums, blend, variance and what is stored are unchanged (the
 *   key stores the CURRENT g.normal and g.prim).  The barycentric form carries deformation as well as rigid motion.  No
 *   transcendental: stage (b) stays reproducible bit for bit.  A snapshot record that is itself degenerate needs no case of its
 *   own: a NaN in it makes z or the normal test fail (no history), never a stored NaN.
 * drt_renderer_motion_vectors writes, for the guides of frame 1 for `cam` and the previous camera `prev_cam` (NULL = the camera of
 * the last drt_renderer_temporal_denoise call), per pixel x + y * width: (fx - (float)x, fy - (float)y, z, flag) with fx, fy, z of
 * stage (b) for P' and NO bounds test on fx, fy; flag 1 = static rule, 2 = moved rule, 0 = no vector (g.prim < 0 or not z > 0:
 * then all four words are 0).  It works with tracking off (every flag then 0 or 1) and does not disarm the snapshot.  `out` is a
 * 16-byte aligned device pointer on the renderer's device, float4[width * height]; hip_stream NULL = the renderer's stream; the
 * call only enqueues, in order with the renderer's ray queries and guide passes (the same event), and uploads the scene as
 * rendering does.  The guides it traces live in a renderer-owned buffer allocated by the first call, freed by resize and destroy.
 * None of the three calls touches the accumulation buffer, the framebuffer, the sample count, the counters, kernel info, kernel
 * span, the temporal history or the denoised target.  track_motion and motion_advance only manage the snapshot and are legal on a
 * sharded renderer.
 * DRT_ERR_INVALID: a NULL argument (prev_cam excepted), prev_cam NULL before the first temporal call (or after a reset / resize), no
 * frame size, a misaligned / host / other-device `out`, a pending drt_renderer_render_batch_async batch.  DRT_ERR_UNSUPPORTED
 * (motion_vectors): a sharded renderer (world > 1), a tree deeper than 64 levels. */
int           drt_renderer_track_motion(drt_renderer *r, int32_t enable);
int           drt_renderer_motion_advance(drt_renderer *r);
int           drt_renderer_motion_vectors(drt_renderer *r, const drt_camera *cam, const drt_camera *prev_cam, const drt_scene *scene,
                                          float *out /* float4[width*height] */, void *hip_stream);

/* ---- guide-driven upscaling: render at low resolution, show at full size (new; joint-bilateral upsampling, Kopf et al. 2007, on
 * the guides above) ----
 * drt_renderer_upscale(r, cam, scene, out_width, out_height, params, delta_ms) rebuilds a Wo x Ho image from the renderer's W x H
 * colour (W x H = the frame size; Wo >= W and Ho >= H) and first-hit guides of both sizes: a guide pixel costs one primary ray, a
 * colour pixel a whole path.  All arithmetic is fp32, one rounding per operation, in the order written; dot and sums run left to
 * right.  Row 0 = bottom, pixel x + y * width, as everywhere.
 * Inputs.  c = the source colour, float4[W * H]: params->source == 0 the framebuffer, == 1 the renderer's denoised target (the
 *   result of the last drt_renderer_denoise or drt_renderer_temporal_denoise).  gl = the guides of frame 1 for `cam` at W x H
 *   (exactly what drt_renderer_denoise uses).  gh = the guides of frame 1 for `cam` at Wo x Ho: bit for bit what
 *   drt_renderer_render_guides returns on a renderer resized to Wo x Ho (the camera's constants for a Wo x Ho image, seed =
 *   (X + Y * Wo) * 1).
 * Per output pixel P = (X, Y):
 * 1. The source position: fx = ((float)X * (float)W) / (float)Wo, x0 = floorf(fx), wx1 = fx - x0, wx0 = 1 - wx1; fy, y0, wy1, wy0
 *    alike from Y, H, Ho (the pixel-corner convention of uv = x / width that the renderer uses: output pixel X looks where source
 *    pixel fx looks).
 * 2. A tap is a source pixel q, both coordinates clamped into the image.  Its value v(q) = c(q).rgb when demodulate == 0, else per
 *    component c(q) / fmaxf(gl.albedo(q), albedo_floor).  It is VALID iff (gl.prim(q) < 0) == (gh.prim(P) < 0).  A valid tap where
 *    both are misses has e = 0; one where both are hits has
 *      e = |gh.normal(P) - gl.normal(q)|^2 * (1 / sigma_normal^2) + dz * dz,  dz = (gl.t(q) - gh.t(P)) * (1 / (sigma_depth * gh.t(P))),
 *    and, when demodulate == 0, e = e + |gh.albedo(P) - gl.albedo(q)|^2 * (1 / sigma_albedo^2)  (squared distances summed over x, y, z).
 * 3. Stage 1, four taps: j = 0, 1 (outer), i = 0, 1 (inner) at (x0 + i, y0 + j), b = wx_i * wy_j.  A tap is ACCEPTED iff it is valid,
 *    b > 0 and e <= 16.  Over the accepted taps in tap order, from 0: w = b * expf(-e), S += w, A += v * w.  If any tap was accepted,
 *    o = A / S.  No expf decides a branch: which stage a pixel takes is reproducible bit for bit.
 * 4. Stage 2, when no tap was accepted: the 4x4 window dy = -1..2 (outer), dx = -1..2 (inner) around (x0, y0), clamped.  The first
 *    valid tap whose e is not NaN is taken, and a later valid tap replaces it iff its e < the taken one's (strict: the first tap wins
 *    a tie, a NaN e never wins).  o = v(q) of the tap taken.
 * 5. Stage 3, when stage 2 took no tap (no tap of the window was valid, or every valid one's e was NaN): o = v(q) at q = (x0 + (wx1 >
 *    0.5f), y0 + (wy1 > 0.5f)), clamped.
 * 6. out(P) = (o, 1) when demodulate == 0, else per component o * fmaxf(gh.albedo(P), albedo_floor), alpha 1.
 * Demodulation interpolates colour / albedo and puts the full-resolution albedo back, so that texture detail could come out at the
 * output's resolution; the albedo term of e is then left out (a texture edge is no reason to reject a tap).  It is OFF by default:
 * the colour is display-referred (every sample tone-mapped and gamma-corrected, so c grows like the square root of the albedo, not
 * like the albedo) and a pixel on a silhouette mixes surfaces while its guide sees one, so the division over-corrects dark texels
 * and edge pixels by up to 1 / albedo_floor.  Measured with the restatement on the CPU oracle, 80 x 60 at 64 spp -> 160 x 120 against
 * 512 spp, MSE relative to plain bilinear: cornell_box 0.339 without and 168 with demodulation, uv_texture_test 0.270 and 634.
 * With Wo == W, Ho == H and demodulate == 0 the result has the source's rgb bits.
 * The result lands in a renderer-owned float4[Wo * Ho], allocated by the first call, again when the output size changes, freed by
 * resize and destroy; drt_renderer_read_upscaled_rgba32f (dst_floats >= Wo * Ho * 4) and drt_renderer_device_upscaled (NULL before
 * the first call) read it.  Blocking; *delta_ms = device time of both guide passes + the kernel.  The accumulation buffer, the
 * framebuffer, the sample count, the counters, kernel info and span, the temporal history, the motion snapshot and the denoised
 * target are not touched.
 * DRT_ERR_INVALID: a NULL argument, no frame size, an output smaller than the frame in either axis or of more than 2^31 pixels,
 * source outside 0..1, source == 1 before any denoise call, demodulate outside 0..1, a sigma or floor that is not finite or not > 0,
 * a pending drt_renderer_render_batch_async batch, a too short dst, a read before the first call.  DRT_ERR_UNSUPPORTED: a sharded
 * renderer (world > 1), a tree deeper than 64 levels.
 * drt_debug_upscale runs the kernel alone on host arrays (colour float4[W * H], guides_lo drt_guide[W * H], guides_hi drt_guide[Wo *
 * Ho], out float4[Wo * Ho]; copied in and out, `source` ignored), for tests that make up their guides.
 * Out of scope: temporal accumulation at output resolution and jitter-aware sample reuse (every frame's source pixels are the
 * same W x H grid: the upscaler adds no detail that the guides do not carry); drt_group and sharded renderers. */
typedef struct drt_upscale_params {
    int32_t source;          /* 0 the framebuffer, 1 the denoised target; default 0 */
    int32_t demodulate;      /* 0 / 1, default 0 (see above) */
    float   sigma_normal, sigma_depth, sigma_albedo;   /* default 0.1, 0.05, 0.1 */
    float   albedo_floor;    /* default 0.01 */
} drt_upscale_params;
void          drt_default_upscale_params(drt_upscale_params *out);
int           drt_renderer_upscale(drt_renderer *r, const drt_camera *cam, const drt_scene *scene, uint32_t out_width, uint32_t out_height,
                                   const drt_upscale_params *p, float *delta_ms);
int           drt_renderer_read_upscaled_rgba32f(drt_renderer *r, float *dst, size_t dst_floats);      /* out_width*out_height*4 */
void         *drt_renderer_device_upscaled(drt_renderer *r);              /* device float4[out_width*out_height], NULL before the first call */
int           drt_debug_upscale(int32_t device, const float *colour, const drt_guide *guides_lo, const drt_guide *guides_hi, uint32_t width,
                                uint32_t height, uint32_t out_width, uint32_t out_height, const drt_upscale_params *p, float *out);

/* ---- path-traced radiance of arbitrary rays (new; the reference shades only its one camera's pixels) ----
 * drt_renderer_camera_rays writes rays[c * width * height + x + y * width] (row 0 = bottom) for every camera c < n_cams and pixel:
 * RayGen's primary ray of that pixel in frame `frame_index`, the rule of the guides (uv = ((float)x / width) * 2 - 1, ((float)y /
 * height) * 2 - 1, seed0 = (x + y * width) * frame_index in uint32, Camera::GetRay with jitter and defocus, the camera's constants
 * for a width x height image); `seed` is the seed state AFTER GetRay, `exposure` the camera's.  The renderer's frame size is not
 * used: any width x height works.  One launch per 32 cameras.
 * drt_renderer_radiance runs RayGen's path loop (RayGen.cuh:88-169) for one sample per ray, started from make_ray(org, dir) and
 * seed `seed`: the renderer's current settings (bounce limit, sunlight, sky, tone mapping, gamma) and material model (emissive,
 * specular, transmission, as the renderer renders them), the tone curve with the ray's `exposure`.  accumulate == 0: out[i] =
 * (c, 1); else out[i].rgb += c (one fp32 add per component, the renderer's accum += c), alpha untouched.  So
 * radiance(camera_rays(cam, W, H, f)) is the renderer's frame-f sample of every pixel, and their sum over frames 1..n divided by n
 * is what ResizeBuffer(W, H), a reset and n renders leave in the framebuffer.  out is float4[n].
 * Both calls take device pointers on the renderer's device (16-byte aligned); hip_stream NULL = the renderer's stream; they only
 * enqueue, in order with the renderer's ray queries and guide passes (the same event).  radiance uploads the scene as rendering
 * does and uses the renderer's refitted copy if there is one.  Neither touches the framebuffer, the accumulation, the sample
 * count, the counters, kernel info or kernel span, so a sharded renderer may call them.  n == 0 is a successful no-op.
 * DRT_ERR_INVALID: a NULL, misaligned, host or other-device pointer, frame_index 0, a zero width, height or n_cams, 2^31 rays or
 * more, a pending drt_renderer_render_batch_async batch.  DRT_ERR_UNSUPPORTED: render_mode DEBUGMODE (debug views stay the
 * framebuffer's), a tree deeper than 64 levels. */
typedef struct drt_path_ray { float org[3]; uint32_t seed; float dir[3]; float exposure; } drt_path_ray;   /* 32 B */
int           drt_renderer_camera_rays(drt_renderer *r, const drt_camera *cams, uint32_t n_cams, uint32_t width, uint32_t height,
                                       uint32_t frame_index, drt_path_ray *rays, void *hip_stream);
int           drt_renderer_radiance(drt_renderer *r, const drt_scene *scene, const drt_path_ray *rays, float *out, uint32_t n,
                                    int32_t accumulate, void *hip_stream);

/* ---- adaptive sampling: spend each call's samples where the noise is (new; the reference gives every pixel one sample per frame) ----
 * drt_renderer_render_adaptive(r, cam, scene, params, info) spends `budget` samples on the frame, more of them where the pixels are
 * noisier, and keeps a per-pixel state from call to call.  Every sample is a sample the uniform renderer would take: the k-th
 * sample a pixel ever receives is its sample of frame k, and the samples are summed in frame order.  A pixel that has received n
 * samples therefore holds, bit for bit, what drt_renderer_read_accum shows at that pixel after a reset and n drt_renderer_render
 * calls with the same camera, scene and settings.  Pixel p = x + y * width, row 0 = bottom, as everywhere.
 * Per-pixel state (allocated by the first call; freed by resize, re-shard, destroy, drt_renderer_adaptive_reset and
 *   drt_renderer_reset, after which the next call starts from nothing; without a state drt_renderer_reset does what it always did):
 *   sum (three fp32: the running colour sum), n (uint32: the samples so far), m1 = sum of Y and m2 = sum of Y * Y in fp32 with Y =
 *   lum(c) of a sample's colour c (lum as defined above: 0.2126f c.r + 0.7152f c.g + 0.0722f c.b), every * and + rounded on its own,
 *   left to right as written.
 * Weight of a pixel, all fp32, one rounding per operation:  n < 2: the weight is unknown, q = 16777215.  Otherwise
 *   mean = m1 / n,  var = fmaxf(m2 / n - mean * mean, 0),  w = sqrtf(var / n) / (mean + luma_floor)    (n converted to fp32)
 *   (the standard error of the mean luminance relative to the mean: radiance is not negative, so neither is w).
 *   If target_error > 0 and w <= target_error: q = 0, the pixel is CONVERGED.  Else s = w * 65536.0f and
 *   q = s < 16777215.0f ? (uint32)s : 16777215  (written so that a NaN or infinite w takes the cap); q == 0 here is converged too.
 * Counts, all integer arithmetic:  Q = sum of q (uint64),  extra = budget - min_spp * pixels,  active = the pixels with q > 0.
 *   A converged pixel gets 0 samples when target_error > 0 and min_spp otherwise; an active pixel gets
 *   min(max_spp, min_spp + (uint32)((uint64)extra * q / Q)).  If Q == 0 and target_error == 0 every pixel gets min(max_spp, min_spp +
 *   extra / pixels).  The counts never sum to more than budget; what the floors and max_spp drop is not redistributed.  On the first
 *   call every pixel is unknown, all q are equal and the call is uniform: no pilot pass is needed.  A consequence of the floors: where
 *   extra * q < Q for every pixel -- min_spp == 0 and a budget below one sample per pixel on a state whose weights are all equal,
 *   the first call included -- every count is 0: the call succeeds with samples == 0, the state is as it was (allocated and zero on
 *   a first call: n == 0 everywhere) and the image is sum / n of it, (0, 0, 0, 1) where n == 0.  The next call is planned as if this
 *   one had not been made.
 * Samples.  A pixel with state count n and call count c receives samples k = 1..c: sample k is the radiance (drt_renderer_radiance:
 *   the current settings and material model) of Camera::GetRay for that pixel in frame n + k -- uv = ((float)x / width) * 2 - 1,
 *   ((float)y / height) * 2 - 1, seed = (x + y * width) * (n + k) in uint32, the camera's constants for the frame size, exactly
 *   drt_renderer_camera_rays' rule.  They are folded in that order: sum += c_k (one fp32 add per component), m1 += Y, m2 += Y * Y;
 *   then n += c.
 * Image.  sum / (float)n per component with alpha 1, (0, 0, 0, 1) where n == 0, written for EVERY pixel to the framebuffer (the
 *   bound one after drt_renderer_bind_buffers): drt_renderer_read_rgba32f, the denoisers, the upscaler and the GL target see it
 *   without change.  A later drt_renderer_render overwrites the framebuffer as it always did.
 * The accumulation buffer, the sample count, the counters, kernel info and span, the temporal history, the denoised and the upscaled
 * target are not touched.  Blocking.  info (may be NULL): samples = the sum of the counts, active_pixels, max_count = the largest
 * count, ms = the device time of the call.  When the samples of a call need more than the renderer's per-launch sample memory (48
 * bytes per sample; DRT_SAMPLE_MB), they are traced in contiguous pixel ranges, which changes no bit.
 * drt_renderer_read_adaptive: which 0 = float4 {sum, bits of n}, 1 = float4 {m1, m2, bits of the last call's q, bits of its count}
 * per pixel, width * height * 16 bytes; drt_renderer_device_adaptive: the same arrays on the device, NULL before the first call.
 * drt_debug_adaptive_plan runs the counts and their exclusive prefix sum alone on host arrays (q, counts, offsets: uint32[pixels];
 * `thresholded` stands for target_error > 0, params->target_error is not read; Q_out may be NULL), for tests that make up q.
 * drt_debug_adaptive_weights runs the weights stage on made-up state records (state0, state1: float4[pixels] laid out as
 * drt_renderer_read_adaptive's which 0 and 1; only the bits of n, m1 and m2 are read) inside the whole plan, as a call runs it with
 * these params: q[pixels] = the weights, *Q_out = their sum, *active_out = the pixels with q > 0 (either may be NULL), for tests
 * that make up moments no render produces.
 * DRT_ERR_INVALID: a NULL argument (info excepted), no frame size, a pending drt_renderer_render_batch_async batch, min_spp >
 * max_spp, max_spp < 1, a budget below min_spp * pixels or of 2^31 samples or more, a target_error not finite or < 0, a luma_floor
 * not finite or not > 0, `which` outside 0..1, a too short dst, a read before the first call.  DRT_ERR_UNSUPPORTED: a sharded
 * renderer (world > 1), render_mode DEBUGMODE, a tree deeper than 64 levels.
 * Out of scope: adaptive sampling inside the frame loop's own kernels; drt_group and sharded renderers; feeding the temporal
 * filter's variance into the weights; redistributing what the floors drop; a linear (pre-tone-curve) target. */
typedef struct drt_adaptive_params { uint32_t budget;      /* samples this call; >= min_spp * pixels, < 2^31 */
                                     uint32_t min_spp, max_spp;       /* per call; default 1, 64; min <= max, max >= 1 */
                                     float target_error, luma_floor;  /* default 0 (off), 0.01; finite, >= 0 resp. > 0 */ } drt_adaptive_params;
typedef struct drt_adaptive_info   { uint32_t samples, active_pixels, max_count; float ms; } drt_adaptive_info;
void          drt_default_adaptive_params(drt_adaptive_params *out);           /* budget 0 = 4 * pixels at call time */
int           drt_renderer_render_adaptive(drt_renderer *r, const drt_camera *cam, const drt_scene *scene, const drt_adaptive_params *p,
                                           drt_adaptive_info *info);
int           drt_renderer_adaptive_reset(drt_renderer *r);               /* drop the state; the next call is uniform again */
int           drt_renderer_read_adaptive(drt_renderer *r, int32_t which, void *dst, size_t dst_bytes);
void         *drt_renderer_device_adaptive(drt_renderer *r, int32_t which);     /* device float4[width*height], NULL before the first call */
int           drt_debug_adaptive_plan(int32_t device, const uint32_t *q, uint32_t pixels, const drt_adaptive_params *p, int32_t thresholded,
                                      uint32_t *counts, uint32_t *offsets, uint64_t *Q_out);
int           drt_debug_adaptive_weights(int32_t device, const float *state0, const float *state1, uint32_t pixels,
                                         const drt_adaptive_params *p, uint32_t *q, uint64_t *Q_out, uint32_t *active_out);

/* ---- BVH refit for moving geometry (new; the reference rebuilds) ----
 * A refit keeps the tree's topology, node order and triangle order and recomputes the boxes bottom-up from new vertex positions.
 * drt_scene_get_triangle_order: out[k] = the load index of triangle k in drt_scene_get_triangles order (= the prim of ray queries
 * and guides): the index it had in load / drt_scene_set_geometry order (what a drt_mesh range addresses).  Identity after a load,
 * permuted by every build exactly as the triangles are.  Returns the count written (at most cap).
 * drt_scene_refit: positions = float[n_tris][3][3] in LOAD order (drt_scene_set_geometry's de-indexed layout); normals the same
 * shape, or NULL to keep the stored vertex normals.  Every triangle is assembled again as the loader assembles it (positions,
 * normals when given, face normal turned towards the averaged vertex normal, centroid; UVs and material stay).  Every node's box
 * comes from the EXACT extent of its subtree: lo / hi = min / max over its vertices (an interior node's = min / max of its
 * children's exact lo / hi, not of their stored boxes), stored as the builder stores it: bmin = lo, bmax = lo + (hi - lo) in fp32.
 * A zero bound takes the order-independent sign (-0 < +0 in min and max), as drt_scene_build_bvh_device.  The revision moves, so
 * renderers upload the scene again.  DRT_ERR_INVALID: no BVH, NULL positions, a non-finite value (checked before anything is
 * written: the scene is unchanged).
 * drt_renderer_refit: the same refit applied to THIS renderer's device copy of `scene` (uploaded first if it holds another):
 * TriHot records, InnerNode child boxes and the root box equal, bit for bit, what the host refit with the same arguments packs
 * (the NaN face normal of a zero-area triangle, which no traversal reads, may carry another payload).  positions / normals are
 * device pointers on the renderer's device, in load order; normals NULL = those of this renderer's last refit that gave them since
 * the upload, else the scene's.  Every later render, query and guide pass of this renderer uses the refitted copy until the scene's
 * revision moves or another scene is uploaded (both upload the host state again and drop the refit); other renderers and the host
 * scene are untouched.  hip_stream NULL = the renderer's stream; the refit waits on the device for the renderer's queries and
 * guide passes in flight and its stream, then blocks until done (the root box travels back to the host); *delta_ms = device time.
 * The accumulation buffer, framebuffer, sample count, counters, kernel info and kernel span are not touched: reset after moving
 * geometry, as after a camera move.  DRT_ERR_INVALID: a NULL / host / other-device pointer or one whose allocation ends short of n_tris * 36 bytes, a pending
 * drt_renderer_render_batch_async batch, no BVH, a non-finite value (the device copy is then dropped: the next use uploads the
 * host state).  DRT_ERR_UNSUPPORTED: a tree deeper than 64 levels. */
int           drt_scene_get_triangle_order(const drt_scene *s, int32_t *out, int32_t cap);
int           drt_scene_refit(drt_scene *s, const float *positions, const float *normals);
int           drt_renderer_refit(drt_renderer *r, const drt_scene *scene, const float *positions, const float *normals, float *delta_ms,
                                 void *hip_stream);
/* Read-backs for the tests: the host pack of the scene (InnerNode[] and TriHot[] records of csrc/device_scene.hpp, root bmin, bmax)
 * and the renderer's current device copy of them (blocking; DRT_ERR_INVALID when it holds no scene).  A NULL destination is
 * skipped; DRT_ERR_INVALID when one is too small. */
int           drt_debug_pack_scene(const drt_scene *s, void *inner, size_t inner_bytes, void *tri_hot, size_t hot_bytes, float root_box[6]);
int           drt_debug_read_device_scene(drt_renderer *r, void *inner, size_t inner_bytes, void *tri_hot, size_t hot_bytes, float root_box[6]);

/* ---- multi-GPU sharding (new; the reference is single-device) ---- */
/* This renderer owns the rows y with (y / stripe_rows) % world == rank, stored compactly in stripe order.
 * RNG seeds use the GLOBAL pixel index, so any partition reproduces the single-device image bit for bit. */
int           drt_renderer_set_shard(drt_renderer *r, uint32_t stripe_rows, uint32_t rank, uint32_t world);
/* Use caller-owned device buffers (e.g. torch tensors) instead of internal ones; NULL restores internal. */
int           drt_renderer_bind_buffers(drt_renderer *r, void *device_accum, void *device_rgba);
int           drt_renderer_set_stream(drt_renderer *r, void *hip_stream);     /* hipStream_t, NULL = default stream */
int           drt_renderer_set_counting(drt_renderer *r, int32_t enable);     /* exact work counters (slower kernel) */
int           drt_renderer_get_counters(drt_renderer *r, drt_counters *out);
int           drt_renderer_kernel_info(const drt_renderer *r, char *buf, size_t cap);  /* name/variant of the last kernel */
/* Hint: the caller keeps n launches in flight on this device (several renderers, each on its own stream, driven through
 * drt_renderer_render_batch_async).  Small launches are then given a share of the workgroup slots so that they overlap instead
 * of queueing behind each other: 1/n while n is below the number of the runtime's hardware queues (GPU_MAX_HW_QUEUES, 4 by
 * default), else one over half that number -- streams that share a queue take turns -- or 1 / min(n, DRT_POOL_SHARE_MAX) with
 * that variable in the environment.  GPU_MAX_HW_QUEUES is read once per process, by the first drt_renderer_create, as the
 * runtime reads it once when it starts: set it before the first HIP call or not at all.  Default 1 = every launch sized to
 * fill the GPU on its own.  Results do not depend on it: every sample is
 * handed out exactly once whatever the grid, and the image is bit for bit the one a lone launch computes. */
int           drt_renderer_set_frames_in_flight(drt_renderer *r, int32_t n);
/* Execution time of the tracing kernel(s) of the last batch that drt_renderer_wait / a blocking render completed, as
 * the kernel itself measured it (first wave in .. last wave out on the device's constant-rate clock).  Unlike the stream
 * events behind *delta_ms it does not include time the launch spent queued behind other streams' work.  0 for the
 * pixel_walk kernel. */
int           drt_renderer_kernel_span(const drt_renderer *r, float *ms);
/* Tracing-kernel launches of the last batch (a batch whose samples exceed the per-launch sample buffer is split). */
int32_t       drt_renderer_launch_count(const drt_renderer *r);
/* rank-0 side of the gather: `gathered` = world shards of padded_rows rows each (as written by the ranks' device_rgba),
 * `image` = full width*height float4.  Runs on `hip_stream`. */
int           drt_assemble_shards(const void *gathered, void *image, uint32_t width, uint32_t height,
                                  uint32_t stripe_rows, uint32_t world, uint32_t padded_rows, void *hip_stream);
/* ---- several GPUs of one node behind one object (one process, N devices) ------------------------------
 * Each device renders its 8-row stripes of the frame (drt_renderer_set_shard; seeds use the global pixel index, so the image
 * is bit-identical to the one-GPU image) on its own stream; the stripes are then gathered into device `devices[0]`'s full
 * RGBA32F image over RCCL -- grouped ncclSend / ncclRecv, one pair per peer moving its whole shard into a staging buffer on
 * devices[0], then one assemble pass; one xGMI link per peer.  RCCL is loaded (dlopen) only when a group of more than one
 * device is created.
 * Same contract as the renderer otherwise: frame index from 1, no-op at max_samples, blocking render returns wall ms.
 * Environment, read by drt_group_create (defaults: unset):
 *   DRT_GROUP_GATHER=stripes   one send / receive pair per 8-row stripe, received at its rows of the image (no assemble pass).
 *   DRT_GROUP_FORCE_RCCL=1     a group of ONE device also gathers through RCCL, sending its shard to itself.
 *   DRT_RCCL_LIB=<path>        test hook: the RCCL entry points are bound from that library instead of librccl.so.1 (one
 *                              table per path; a group keeps the one it was created with).
 *   DRT_GROUP_SHARE_DEVICE=1   test hook, honoured only with DRT_RCCL_LIB: a device may appear more than once (a renderer and
 *                              a stream per entry, all on that GPU).  Otherwise a repeated device is refused (NULL,
 *                              drt_last_error "a device appears twice in the group"): RCCL itself never sees one. */
typedef struct drt_group drt_group;
drt_group    *drt_group_create(const int32_t *devices, int32_t n_devices);     /* NULL on failure (drt_last_error) */
void          drt_group_destroy(drt_group *g);
int32_t       drt_group_size(const drt_group *g);
drt_renderer *drt_group_renderer(drt_group *g, int32_t index);                /* the device's renderer (settings, counters, kernel info) */
int           drt_group_resize(drt_group *g, uint32_t width, uint32_t height);
int           drt_group_set_settings(drt_group *g, const drt_settings *s);
int           drt_group_reset(drt_group *g);
int           drt_group_render_batch(drt_group *g, const drt_camera *cam, const drt_scene *scene, uint32_t n_frames, float *delta_ms);
int           drt_group_render_batch_async(drt_group *g, const drt_camera *cam, const drt_scene *scene, uint32_t n_frames);
int           drt_group_wait(drt_group *g, float *delta_ms);
uint32_t      drt_group_sample_count(const drt_group *g);
void         *drt_group_device_rgba(drt_group *g);                             /* float4[width*height] on devices[0] */
int           drt_group_read_rgba32f(drt_group *g, float *dst, size_t dst_floats);
/* Stripe k of `rank` in a `world`-way split: offset in the rank's compact shard, offset in the full image, length -- in floats
 * of an RGBA32F frame.  Returns 0 when the rank has no k-th stripe.  (What the gather's send / receive offsets are made of.) */
int           drt_shard_stripe(uint32_t width, uint32_t height, uint32_t stripe_rows, uint32_t rank, uint32_t world, uint32_t k,
                               uint64_t *src_offset_floats, uint64_t *dst_offset_floats, uint64_t *count_floats);
/* Self-check of the kernels' reciprocal (device_math.hpp exact_rcp) against IEEE 1.0f/x over all 2^32 float bit patterns. */
int           drt_debug_check_rcp(int32_t device, uint64_t *mismatches, uint64_t *fast_path_count);
int           drt_debug_check_sqrt(int32_t device, uint64_t *mismatches, uint64_t *fast_path_count);   /* exact_sqrt vs sqrtf */
/* Host: decode an image file held in memory (PNG, or baseline JPEG) exactly as the loader does for embedded glTF images
 * (Scene.cu:93-114 -> Texture.cu:21-30: native channel count, row 0 first).  `out` may be NULL to query the size only. */
int           drt_debug_decode_image(const uint8_t *file, size_t file_bytes, drt_texture_info *info, uint8_t *out, size_t cap);
/* Device leaf functions on arrays, for known-answer tests against tests/golden/kat_ref.npz.
 * which: 0 unit vec (in u32 seed; out vec3,seed,tries), 1 unit sphere (same), 2 slab (in orig3,dir3,min3,max3; out f32),
 * 3 triangle (in orig3,dir3,v0,v1,v2; out t,U,V,W,hit), 4 camera ray (in u,v,seed; out orig3,dir3,seed; needs cam,width,height),
 * 5 unit disk (in seed; out x,y,seed), 6 closest-hit frame (in orig3,dir3,t,face_normal3; out position3,normal3,front_face).
 * Two forms of one computation side by side (they must agree bit for bit): 7 normalize and the bounce sampler's normalize for
 * components in [-1, 1] (in vec3; out vec3,vec3), 8 their inverse lengths (in dot(v,v) in [0, 3]; out f32,f32). */
int           drt_debug_kat(int32_t device, int32_t which, const void *in, size_t in_bytes, void *out, size_t out_bytes, uint32_t n,
                            const drt_camera *cam, uint32_t width, uint32_t height);
/* Every 32-bit value on a cycle of the RNG hash (Random.cu:6-11) no longer than max_len: (value, length) pairs. */
int           drt_debug_hash_cycles(int32_t device, uint32_t max_len, uint32_t *pairs_out, uint32_t cap_pairs, uint32_t *found);
/* The wave_queue launch packagings (workgroup size, stack entry bytes, triangles per step) this renderer has timed so far, as
 * JSON text: one plan per (kernel, scene shape, view class) with its candidates, their trials and best ns per sample, and
 * the index of the one kept (-1 = still measuring).  All candidates compute the same image. */
int           drt_debug_wave_queue_plans(const drt_renderer *r, char *buf, size_t cap);
/* path_pool kernel statistics of a renderer created with DRT_POOL_STATS=1 in the environment: per queue (N, T0..T3, B, E, R, S)
 * {batches, paths served, shader-clock ticks}, then ticks spent claiming, idle polls, lost claims, wave ticks, claims given up,
 * their ticks, idle ticks. */
int           drt_debug_pool_stats(drt_renderer *r, uint64_t out[40], int32_t reset);
uint32_t      drt_shard_rows(uint32_t height, uint32_t stripe_rows, uint32_t rank, uint32_t world);

#ifdef __cplusplus
}
#endif
#endif
