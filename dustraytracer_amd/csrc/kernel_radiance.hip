// kernel_radiance.hip -- path-traced radiance of caller-chosen rays for gfx950 (drt_renderer_radiance), and the renderer's
// primary rays of many cameras (drt_renderer_camera_rays).
//
// Reference: RayGen's path loop (Shaders/RayGen.cuh:88-169, restated in oracle/drt_oracle.c ray_gen) for one sample, started
// from make_ray(org, dir) and the seed state `seed` instead of Camera::GetRay: per bounce i, TraceRay (closest hit at
// (-1, FLT_MAX), AnyHit alpha), seed += i, sky on a miss, else the opt-in emissive term, the albedo or texel into the
// throughput, the sun's shadow ray through traverseBVH_raytest, then the next direction (diffuse, or the opt-in mirror and
// dielectric lobes); the tone curve with the ray's exposure and gamma at the end.  The leaf arithmetic is the renderer's
// (device_math.hpp / device_access.hpp), so a radiance query fed with camera_rays' output is the renderer's sample bit for bit.
//
// Grid, claim and stack: query_frame.hpp.  One path per lane; every trip of a wave's loop is one traversal step of each busy
// lane (closest-hit or shadow, per lane), and a lane whose traversal is over shades in the same trip and starts its next
// traversal (shadow ray, next bounce) or writes its result and goes idle.  Stack entries {ref, entry distance},
// kRqLdsLevelsClosest levels in LDS (the closest-hit query's layout).
// Builds: SUN (the shadow ray and the continuation ray it holds back: 6 more registers), ALPHA (AnyHit reads the texture),
// EXT (the material model); the lean build reads neither.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "device_scene.hpp"
#include "device_access.hpp"
#include "query_frame.hpp"
#include "radiance.hpp"

namespace drt {

namespace {

// waves per SIMD each build is compiled for (VGPR budget: 8 -> 64, 7 -> 72): the full build spills at 64
template <bool SUN, bool ALPHA, bool EXT>
constexpr int radiance_waves() { return (SUN && ALPHA && EXT) ? 7 : 8; }

template <bool SUN, bool ALPHA, bool EXT>
__global__ __launch_bounds__(kRqThreads, (radiance_waves<SUN, ALPHA, EXT>())) void radiance_kernel(const SceneView sc, const FrameParams fp,
                                                                                                 const RadianceArgs a) {
    constexpr int K = kRqLdsLevelsClosest;
    __shared__ uint32_t s_ref[K][kRqThreads];
    __shared__ float s_dist[K][kRqThreads];
    const int tid = threadIdx.x;
    const uint32_t gthread = blockIdx.x * kRqThreads + tid;
    const StackLane st = {tid, gthread, gridDim.x * kRqThreads, a.frame.stack_levels, a.frame.stack_hbm};
    uint32_t shard = home_shard(gthread);
    int shards_empty = 0;

    int rid = -1;                                            // this lane's path, -1 = idle
    Ray ray;
    f3 throughput = mk3(1, 1, 1), light = mk3(0, 0, 0);
    uint32_t seed = 0;
    int bounce = 0;                                          // RayGen's i
    bool shadow = false;                                     // SUN: the lane traces the shadow ray of bounce i
    bool last = false;                                       // SUN: the path ends once the shadow ray is done
    f3 next_o = mk3(0, 0, 0), next_d = mk3(0, 0, 0);         // SUN: the continuation ray, held back behind the shadow ray
    float best_t = FLT_MAX, best_u = 0.f, best_v = 0.f;      // closest hit so far (prim -1 = none)
    int best_prim = -1;
    bool occluded = false;
    bool done = false;                                       // the path is over: write it
    uint32_t sp = 0;

    // the closest-hit traversal of `ray` starts (TraceRay.cu:15-18: the root with its entry distance, culled at its pop)
    auto start_closest = [&]() {
        best_t = FLT_MAX; best_prim = -1; best_u = 0.f; best_v = 0.f; sp = 0;
        if (sc.root_ref != kNoNode) { s_ref[0][tid] = sc.root_ref; s_dist[0][tid] = slab_intersect(ld3(sc.root_min), ld3(sc.root_max), ray); sp = 1; }
    };

    for (;;) {
        // ---- refill: claim paths for the idle lanes (wave-uniform) ----
        const uint64_t idle = __ballot(rid < 0);
        if (claim_due(shards_empty, idle, a.frame)) {
            const bool was_idle = rid < 0;
            const Claimed c = claim_take(shard, shards_empty, rid, idle, a.frame);
            shard = c.shard; shards_empty = c.shards_empty; rid = c.rid;
            if (was_idle && rid >= 0) {
                // a new path: drt_path_ray = org, seed, dir, exposure (two 16-byte loads); RayGen.cuh:80-88
                const float4 *r = reinterpret_cast<const float4 *>(a.rays) + 2 * (size_t)(uint32_t)rid;
                const float4 o = r[0], d = r[1];
                ray = make_ray(mk3(o.x, o.y, o.z), mk3(d.x, d.y, d.z));
                seed = __float_as_uint(o.w);
                throughput = mk3(1, 1, 1); light = mk3(0, 0, 0);
                bounce = 0; shadow = false; occluded = false;
                done = fp.bounce_limit < 0;                  // the loop `for (i = 0; i <= bounces; i++)` does not run
                if (!done) start_closest();
            }
        }
        if (claim_drained(shards_empty, rid)) break;

        // ---- one traversal step per busy lane: closest hit (BVHTraversal.cuh:14-73) or, SUN, the shadow test (:76-134) ----
        if (rid >= 0 && !done && sp > 0 && !occluded) {
            float dist;
            const uint32_t ref = stack_pop(s_ref, s_dist, st, sp, dist);
            bool visit = true;
            if (!(SUN && shadow)) {
                if (!(-1.0f < dist && dist < FLT_MAX)) visit = false;                      // :38 interval (-1, FLT_MAX)
                else if (best_prim >= 0 && best_t < dist) visit = false;               // :41
            }
            if (visit) {
                if (ref & kLeafBit) {
                    const LeafRange leaf = sc.leaves[ref & ~kLeafBit];
                    for (int i = leaf.start; i < leaf.start + leaf.count; i++) {        // :46-57 / :107-115
                        const TriTest tri = load_tri(sc.tri_hot, i);
                        float t, u, v;
                        const bool h = tri_intersect_flat(ray, tri.v0, tri.e1, tri.e2, t, u, v);
                        if (SUN && shadow) {
                            if (h && (!ALPHA || any_hit(sc, i, mk3(1.0f - u - v, u, v)))) { occluded = true; break; }
                        } else if (h && t < best_t) {
                            if (ALPHA && !any_hit(sc, i, mk3(1.0f - u - v, u, v))) continue;
                            best_t = t; best_prim = i; best_u = u; best_v = v;
                        }
                    }
                } else {
                    const ChildPair c = load_children(sc.inner, ref);
                    const float d1 = slab_intersect(c.min1, c.max1, ray);
                    const float d2 = slab_intersect(c.min2, c.max2, ray);
                    const bool sh = SUN && shadow;
                    const bool push1 = d1 >= 0 && (sh || d1 < best_t), push2 = d2 >= 0 && (sh || d2 < best_t);   // :63-70 / :122-129
                    push_far_first(s_ref, s_dist, st, sp, c.ref1, d1, push1, c.ref2, d2, push2);        // farther child first
                }
            }
        }

        // ---- a finished traversal: shade, and start the next one ----
        if (rid >= 0 && !done && (sp == 0 || occluded)) {
            if (SUN && shadow) {
                if (!occluded) light = light + ld3(fp.suncol) * throughput;                // RayGen.cuh:126-127
                occluded = false; shadow = false;
                if (last) done = true;
                else { ray = make_ray(next_o, next_d); ++bounce; start_closest(); }
            } else {
                seed += (uint32_t)bounce;                                                 // :91
                if (best_prim < 0) {                                                       // :99-108 Miss
                    light = light + sky_model(ray.dir, ld3(fp.sky_color)) * throughput * fp.sky_intensity;
                    done = true;
                } else {
                    const uint32_t prim = (uint32_t)best_prim;
                    const f3 uvw = mk3(1.0f - best_u - best_v, best_u, best_v);            // Intersection.cu:31
                    f3 position, normal;                                                   // ClosestHit.cuh:13-24
                    const bool front_face = closest_hit_frame(ray, best_t, ld3(sc.tri_hot[prim].fn), position, normal);
                    const TriCold cold = sc.tri_cold[prim];                                // :111-118
                    const MatDev mat = sc.mats[cold.material];
                    MatExt ext;
                    if (EXT) {
                        ext = sc.mats_ext[cold.material];
                        if (fp.ext_emissive) light = light + (ld3(ext.emissive) * fp.ext_emissive_scale) * throughput;
                    }
                    if (mat.tex < 0) throughput = throughput * ld3(mat.albedo);
                    else throughput = throughput * tex_get_pixel(sc, sc.texs[mat.tex], interp_uv(cold, uvw));
                    const f3 origin = position + (normal * 0.001f);                        // :121
                    Ray sun_ray;
                    if (SUN) sun_ray = make_ray(origin, ld3(fp.sunpos) + random_unit_vec3(seed) * 1.5f);    // :124-125
                    // the next direction (:130-134, or the material model's lobes); nothing after the last bounce reads it
                    bool ends = bounce >= fp.bounce_limit;
                    f3 no = origin, nd = mk3(0, 0, 0);
                    if (!ends) {
                        const bool glass = EXT && fp.ext_transmission && ext.transmission != 0;
                        const bool mirror = EXT && !glass && fp.ext_specular && ext.metallic != 0;
                        f3 v = mk3(0, 0, 0), refl = mk3(0, 0, 0);
                        if (EXT && (glass || mirror)) { v = normalize(ray.dir); refl = v - normal * (2.0f * dot(v, normal)); }
                        if (EXT && glass) {                                                // Random.cu:26-40
                            const float cos_theta = fminf(dot(mk3(v.x * -1.f, v.y * -1.f, v.z * -1.f), normal), 1.0f);
                            const float ri = front_face ? 1.0f / ext.refractive_index : ext.refractive_index;
                            const float sin_theta = sqrtf(1.0f - cos_theta * cos_theta);
                            bool reflect = ri * sin_theta > 1.0f;
                            float r0 = (1 - ri) / (1 + ri);
                            r0 = r0 * r0;
                            const float om = 1 - cos_theta;
                            const float schlick = r0 + (1 - r0) * (((om * om) * (om * om)) * om);
                            if (!reflect) reflect = schlick > random_float(seed);
                            if (reflect) nd = refl;
                            else {
                                const f3 perp = (v + normal * cos_theta) * ri;
                                const f3 par = normal * (-sqrtf(fabsf(1.0f - dot(perp, perp))));
                                no = position - (normal * 0.001f); nd = perp + par;
                            }
                        } else {
                            const f3 fuzz = random_unit_sphere_vec3(seed);
                            if (EXT && mirror) {                                           // mirror lobe, fuzzed by the roughness
                                nd = refl + fuzz * ext.roughness;
                                if (!(dot(nd, normal) > 0.0f)) ends = true;                // scattered into the surface: absorbed
                            } else {
                                nd = normal + fuzz;                                        // :133-134
                            }
                        }
                    }
                    if (SUN) {
                        ray = sun_ray; shadow = true; last = ends; next_o = no; next_d = nd;
                        sp = 0;                                                            // :95-103 the root, unless d < 0
                        if (sc.root_ref != kNoNode && !(slab_intersect(ld3(sc.root_min), ld3(sc.root_max), ray) < 0)) { s_ref[0][tid] = sc.root_ref; sp = 1; }
                    } else if (ends) {
                        done = true;
                    } else {
                        ray = make_ray(no, nd); ++bounce; start_closest();
                    }
                }
            }
        }

        // ---- finished paths: the tone curve (:165-169) and the result ----
        if (rid >= 0 && done) {
            const float exposure = reinterpret_cast<const float4 *>(a.rays)[2 * (size_t)(uint32_t)rid + 1].w;
            if (fp.tone_mapping) light = uncharted2_filmic(light, exposure);
            if (fp.gamma_correction) light = gamma_correction(light);
            float4 *o = a.out + (uint32_t)rid;
            if (a.accumulate) {
                float4 acc = *o;
                acc.x = acc.x + light.x; acc.y = acc.y + light.y; acc.z = acc.z + light.z;     // RenderKernel.cu:29
                *o = acc;
            } else {
                *o = make_float4(light.x, light.y, light.z, 1.0f);
            }
            rid = -1; done = false; sp = 0; occluded = false; shadow = false;
        }
    }
}

// RayGen.cuh:65-85 for one pixel of one camera: uv, seed = (x + y * width) * frame, Camera::GetRay (jitter, defocus)
__global__ __launch_bounds__(256) void camera_rays_kernel(const CameraRaysArgs a) {
    const uint32_t pixels = a.width * a.height;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n_cams * pixels) return;
    const uint32_t c = i / pixels, p = i - c * pixels;
    const uint32_t x = p % a.width, y = p / a.width;
    const CamConst &cc = a.cams[c];
    FrameParams fp;
    for (int k = 0; k < 3; k++) {
        fp.cam_pos[k] = cc.cam_pos[k]; fp.fwd_focus[k] = cc.fwd_focus[k]; fp.horizontal[k] = cc.horizontal[k];
        fp.vertical[k] = cc.vertical[k]; fp.disk_u[k] = cc.disk_u[k]; fp.disk_v[k] = cc.disk_v[k];
    }
    fp.defocus = cc.defocus;
    f2 screen_uv;
    screen_uv.x = ((float)x / (float)a.width) * 2 - 1;
    screen_uv.y = ((float)y / (float)a.height) * 2 - 1;
    uint32_t seed = x + y * a.width;
    seed *= a.frame;
    const Ray r = camera_get_ray(fp, screen_uv, seed);
    float4 *o = reinterpret_cast<float4 *>(a.rays) + 2 * (size_t)i;
    o[0] = make_float4(r.orig.x, r.orig.y, r.orig.z, __uint_as_float(seed));
    o[1] = make_float4(r.dir.x, r.dir.y, r.dir.z, cc.exposure);
}

template <bool SUN, bool ALPHA, bool EXT>
hipError_t launch_radiance_t(const SceneView &sc, const FrameParams &fp, const RadianceArgs &a, int num_cus, hipStream_t stream) {
    const uint32_t blocks = query_blocks(a.frame.n, num_cus, radiance_waves<SUN, ALPHA, EXT>());
    hipLaunchKernelGGL((radiance_kernel<SUN, ALPHA, EXT>), dim3(blocks), dim3(kRqThreads), 0, stream, sc, fp, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_camera_rays(const CameraRaysArgs &a, hipStream_t stream) {
    const uint64_t n = (uint64_t)a.n_cams * a.width * a.height;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(camera_rays_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_radiance(const SceneView &sc, const FrameParams &fp, bool alpha, const RadianceArgs &a, int num_cus, hipStream_t stream) {
    if (a.frame.n == 0) return hipSuccess;
    const bool sun = fp.enable_sunlight != 0, ext = fp.ext_emissive || fp.ext_specular || fp.ext_transmission;
    const int v = (sun ? 4 : 0) | (alpha ? 2 : 0) | (ext ? 1 : 0);
    switch (v) {
    case 0: return launch_radiance_t<false, false, false>(sc, fp, a, num_cus, stream);
    case 1: return launch_radiance_t<false, false, true>(sc, fp, a, num_cus, stream);
    case 2: return launch_radiance_t<false, true, false>(sc, fp, a, num_cus, stream);
    case 3: return launch_radiance_t<false, true, true>(sc, fp, a, num_cus, stream);
    case 4: return launch_radiance_t<true, false, false>(sc, fp, a, num_cus, stream);
    case 5: return launch_radiance_t<true, false, true>(sc, fp, a, num_cus, stream);
    case 6: return launch_radiance_t<true, true, false>(sc, fp, a, num_cus, stream);
    default: return launch_radiance_t<true, true, true>(sc, fp, a, num_cus, stream);
    }
}

}  // namespace drt
