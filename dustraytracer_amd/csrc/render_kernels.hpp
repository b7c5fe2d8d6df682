// render_kernels.hpp -- launch wrappers of render_kernels.hip (the seam that replaces InvokeRenderKernel,
// Core/Kernel/RenderKernel.cuh:12-14; grid/block shape is an internal choice here).
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <vector>

#include "device_scene.hpp"
#include "pool_share.hpp"

namespace drt {

constexpr size_t kLdsSceneBytes = 40 * 1024;     // stage the traversal data in LDS when it is at most this big

// Which tracing kernel a render batch runs, and which build of it.  choose_tracer (drt_capi.cpp) decides once per batch; the
// launchers derive nothing from the settings again, only what depends on the launch's shape (path_pool's deep-stack build 32,
// wave_queue's measured packaging).
enum class Tracer { none, pixel_walk, wave_queue, path_pool };
struct TracerChoice {
    Tracer family = Tracer::none;
    int pool_flags = 0;        // path_pool: 1 statistics, 2 sun, 4 alpha, 8 hbm-scene, 16 material model (path_pool_kernel<FLAGS>)
    int wq_mode = 0;           // wave_queue: 0 lean, 1 general, 2 counting, 3 lean+alpha, 4 lean+sun, 5 lean+alpha+sun
    bool wq_lds_scene = false; // wave_queue: the traversal data is staged in LDS
    int stack = 0;             // pixel_walk: traversal stack entries per lane (8, 16, 32 or 64)
};

// What the last tracing-kernel launch looked like (drt_renderer_kernel_info)
struct LaunchShape { int stack_levels = 0, levels_in_lds = 0, groups_per_cu = 0, lds_kib = 0, threads = 0, paths = 0, entry_bytes = 8, tris = 2; };

// Environment switches, read once when a renderer is created; path_pool's 0 / -1 = the launcher's default
struct Tuning {
    Tracer kernel = Tracer::path_pool;                                          // DRT_KERNEL=wave_queue / pixel_walk
    size_t pool_scene_bytes = kLdsSceneBytes, lds_scene_bytes = kLdsSceneBytes; // DRT_POOL_SCENE_KB, DRT_LDS_SCENE_KB: largest lds-scene of path_pool, wave_queue
    bool pool_hbm = true, pool_verbose = false, t_class_set = false;            // DRT_POOL_HBM=0, DRT_POOL_VERBOSE, DRT_POOL_T_CLASSES="a,b,c" (bounds of T0..T2):
    uint32_t t_class[3] = { 0, 0, 0 };
    int threads = 0, paths = 0, stack_lds = 0, min_fill = 48, patience = 8, n_loop = 8, n_min_lanes = 16, n_fuse_loop = 8, n_fuse_min = 24,
        cold_lds_kb = -1, share_grid = 1, dir_tries = 4;                        // DRT_POOL_THREADS / _PATHS / _STACK_LDS / ...: path_pool's shape
    int share_max = 0, hw_queues = 4;                                           // DRT_POOL_SHARE_MAX: launches that run side by side (0 = pool_share_max of the hint and hw_queues: GPU_MAX_HW_QUEUES as the process started with it, or DRT_POOL_HW_QUEUES)
    unsigned long long *stats = nullptr;                                        // DRT_POOL_STATS=1: device u64[40] of path_pool's statistics builds
    bool wq_only_small = false, wq_only_wide = false, wq_tris_wide = true;      // DRT_WG_THREADS=256, DRT_STACK_REF16=0, DRT_TRIS_WIDE=0: wave_queue's packagings
    int max_blocks_per_cu = 1 << 30, chunks_per_wg = 0;                         // DRT_MAX_BLOCKS_PER_CU, DRT_CHUNKS_PER_WG (0: by frames in flight)
};

// pixel_walk: only in builds with -DDRT_WITH_PIXEL_WALK (`make pixel-walk`: the tests' cross-check library)
bool pixel_walk_built_in();
hipError_t launch_render(const SceneView &scene, const FrameParams &frame, const TracerChoice &choice, bool count_work, hipStream_t stream);

// wave_queue (kernel_wave_queue.hip): persistent waves + tile queue + phase voting.
// which packaging of a wave_queue launch is fastest is measured, once per (kernel, scene shape, view class); one cache per renderer
struct WqVariant { int threads, entry_bytes, tris, per_cu; };
struct WqPlan { uint64_t key = 0; std::vector<WqVariant> cands; std::vector<double> ns_per_sample; std::vector<int> trials; int chosen = -1; };
struct WaveQueueCache { std::vector<WqPlan> plans; uint64_t batch_key = 0; int batch_cand = -1; double batch_samples = 0; };
void wave_queue_report(WaveQueueCache &cache, float span_ms);
WqVariant measured_choice(WaveQueueCache &cache, uint64_t key, double samples, const std::function<std::vector<WqVariant>()> &candidates);
// `samples` must hold wave_queue_sample_bytes(frame) bytes (one float4 per pixel and frame of the launch); the launch
// runs the tracing kernel and then the ordered resolve kernel on `stream`.
size_t wave_queue_sample_bytes(const FrameParams &frame);
hipError_t launch_wave_queue(const SceneView &scene, const FrameParams &frame, int bvh_depth, const TracerChoice &choice, const Tuning &tune,
                             unsigned int *chunk_counter, void *samples, int num_cus, hipStream_t stream, LaunchShape *shape, WaveQueueCache &cache);

hipError_t launch_resolve(const FrameParams &frame, void *samples, hipStream_t stream);
size_t wave_queue_scene_lds_bytes(const SceneView &scene);

// The work-queue heads a launch draws from: one block of kPoolSampleShards counters, kPoolSampleShardStride words (128 bytes)
// apart (path_pool: sample ids sharded over them, so that a whole chip's waves do not serialise on one address; wave_queue
// uses the first word only).  The renderer hands out zeroed blocks.
#ifndef DRT_SAMPLE_SHARDS
#define DRT_SAMPLE_SHARDS 16          // (a power of two; -DDRT_SAMPLE_SHARDS=1 in EXTRA: the single counter of rounds 1-2, for A/B runs)
#endif
constexpr int kPoolSampleShards = DRT_SAMPLE_SHARDS, kPoolSampleShardStride = 32, kQueueHeadBlockWords = kPoolSampleShards * kPoolSampleShardStride;

// path_pool (kernel_path_pool.hip): path state parked in LDS, phase-homogeneous batches of 64 paths.  `status` is a device word
// the kernel sets when it had to abort (never hangs).
// path_pool_fits: the smallest pool of the lds-scene build (scene_lds_bytes of traversal data next to it) or of the hbm-scene build
// fits the CU's LDS under a tree of bvh_depth levels.
bool path_pool_fits(const SceneView &scene, int bvh_depth, size_t scene_lds_bytes, bool hbm_scene);
void path_pool_leaf_classes(const std::vector<LeafRange> &leaves, uint32_t out[3]);
struct PoolScratch { void *aux = nullptr, *aux_slot = nullptr, *aux_light = nullptr, *aux_next = nullptr, *aux_stack = nullptr; size_t slots = 0, next_slots = 0, stack_slots = 0; };     // HBM part of the path state, owned by the renderer
// t_safe_dir: pool_safe_dir (pool_index.hpp) of the largest |edge component| among the scene's triangles as they stand in device memory; 0 when that is not known.
hipError_t launch_path_pool(const SceneView &scene, const FrameParams &frame, int bvh_depth, const TracerChoice &choice, const uint32_t t_class[3], float t_safe_dir, const Tuning &tune,
                            PoolScratch &scratch, unsigned int *sample_counter, void *samples, unsigned int *status, int num_cus, hipStream_t stream, LaunchShape *shape);

// debug: d_out2[0] += #floats in [first_bits, first_bits+count) where exact_rcp != 1.0f/x (which 0) or exact_sqrt != sqrtf (which 1),
// d_out2[1] += #floats on the fast path
hipError_t launch_check_rcp(int which, uint32_t first_bits, unsigned long long count, unsigned long long *d_out2, hipStream_t stream);

// debug: all values on pcg_hash cycles of length <= max_len; d_out = [count, (value, length) x cap_pairs]
hipError_t launch_hash_cycles(uint32_t max_len, uint32_t *d_out, uint32_t cap_pairs, hipStream_t stream);

// debug: device leaf functions on arrays (which: 0 unit vec, 1 unit sphere, 2 slab, 3 triangle, 4 camera ray, 5 unit disk)
hipError_t launch_kat(int which, const void *d_in, void *d_out, uint32_t n, const FrameParams &frame, hipStream_t stream);

hipError_t launch_assemble(const void *gathered, void *image, uint32_t width, uint32_t height, uint32_t stripe_rows,
                           uint32_t world, uint32_t padded_rows, hipStream_t stream);

}  // namespace drt
