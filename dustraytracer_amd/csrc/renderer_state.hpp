// renderer_state.hpp -- what the translation units of the C ABI share (drt_capi.cpp, drt_capi_filters.cpp, drt_capi_adaptive.cpp, drt_capi_section.cpp, drt_capi_contour.cpp, drt_capi_topology.cpp, drt_capi_intersect.cpp, drt_capi_surface.cpp, drt_capi_ambient.cpp, drt_capi_winding.cpp): the renderer's state,
// the owners of its device memory, pinned memory and events, error reporting, the steps several entry points take.  Not exported.
#pragma once
#include "../../include/drt.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "device_scene.hpp"
#include "render_kernels.hpp"
#include "denoise.hpp"
#include "temporal.hpp"
#include "radiance.hpp"
#include "adaptive.hpp"
#include "refit.hpp"
#include "winding.hpp"
#include "scene_host.hpp"

#pragma GCC visibility push(hidden)

namespace drt {

int fail(int code, const std::string &msg);       // sets drt_last_error() for this thread, returns `code`

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(DRT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));        \
    } while (0)

// Device memory with one owner: released by release(), by the next alloc() / upload() and with the owner
template <class T>
struct DeviceArray {
    T *ptr = nullptr;
    size_t count = 0;
    DeviceArray() = default;
    DeviceArray(const DeviceArray &) = delete; DeviceArray &operator=(const DeviceArray &) = delete;
    ~DeviceArray() { release(); }
    size_t bytes() const { return count * sizeof(T); }
    hipError_t upload(const std::vector<T> &host) {
        hipError_t e = alloc(host.size());
        if (e == hipSuccess && !host.empty()) e = hipMemcpy(ptr, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice);
        return e;
    }
    hipError_t alloc(size_t n) {                 // uninitialised
        release();
        hipError_t e = hipMalloc((void **)&ptr, std::max<size_t>(n, 1) * sizeof(T));
        if (e != hipSuccess) { ptr = nullptr; return e; }
        count = n;
        return e;
    }
    hipError_t alloc_zeroed(size_t n) {
        hipError_t e = alloc(n);
        return e == hipSuccess ? hipMemset(ptr, 0, std::max<size_t>(n, 1) * sizeof(T)) : e;
    }
    void release() { if (ptr) (void)hipFree(ptr); ptr = nullptr; count = 0; }
};

// All of a group of equally long arrays or none: a failure releases every member, so the next call allocates again
template <class... Arrays>
hipError_t alloc_group(size_t n, Arrays &...arrays) {
    hipError_t e = hipSuccess;
    ((e = e == hipSuccess ? arrays.alloc(n) : e), ...);
    if (e != hipSuccess) (arrays.release(), ...);
    return e;
}

struct PinnedWords {                             // page-locked host memory
    unsigned long long *ptr = nullptr;
    PinnedWords() = default;
    PinnedWords(const PinnedWords &) = delete; PinnedWords &operator=(const PinnedWords &) = delete;
    ~PinnedWords() { if (ptr) (void)hipHostFree(ptr); }
    hipError_t alloc(size_t n) { return hipHostMalloc((void **)&ptr, n * sizeof *ptr, hipHostMallocDefault); }
};

struct Event {                                   // created by the first create(), which later ones leave alone
    hipEvent_t ev = nullptr;
    Event() = default;
    Event(const Event &) = delete; Event &operator=(const Event &) = delete;
    ~Event() { if (ev) (void)hipEventDestroy(ev); }
    hipError_t create(unsigned flags = hipEventDefault) { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, flags); }
    operator hipEvent_t() const { return ev; }
};

}  // namespace drt

struct drt_scene {
    drt::HostScene host;
};

struct drt_renderer {
    template <class T> using DeviceArray = drt::DeviceArray<T>;
    using Event = drt::Event;
    int device = 0;
    drt_settings settings;
    uint32_t width = 0, height = 0;
    uint32_t frame_index = 1;                 // m_FrameIndex, Renderer.hpp:41
    uint32_t stripe_rows = 1, rank = 0, world = 1, local_rows = 0;
    DeviceArray<float> accum, rgba;           // internal buffers
    float *ext_accum = nullptr, *ext_rgba = nullptr;      // drt_renderer_bind_buffers: the caller's, not ours
    hipStream_t stream = nullptr;
    Event ev_start, ev_stop;
    bool counting = false;
    bool pending = false;                     // an asynchronous render was enqueued and not waited for yet
    DeviceArray<unsigned long long> counters; // drt_counters as its 64-bit words
    static constexpr int kMaxSpans = 64;
    // One 32-byte record per tracing-kernel launch: {max(~first wave in), max(last wave out), status bits, -}.  The records come
    // zeroed from a ring (one memset per kRecords launches); those of a batch are copied to pinned host memory on the stream, in
    // front of ev_stop, so that drt_renderer_wait reads spans and status without another trip to the device.
    static constexpr int kRecords = 1024;
    DeviceArray<unsigned long long> records;  // device: kRecords x 4 words
    drt::PinnedWords records_host;            // pinned: the kMaxSpans records of the last batch
    int records_used = 0, batch_first_record = 0;
    int spans_used = 0;                       // launches of the last batch that have a record
    int launches_last = 0;                     // tracing-kernel launches of the last batch (a batch is split by the sample budget)
    float span_ms = 0.f;                       // sum of those spans, filled by drt_renderer_wait
    int wall_clock_khz = 100000;
    static constexpr int kCounters = 256;
    DeviceArray<unsigned int> tile_counter;   // work queue heads of the tracing kernels: kCounters zeroed blocks (kQueueHeadBlockWords each), one per launch, re-zeroed
    int counters_used = 0;                    // in one memset when all are spent (no memset in front of every launch)
    DeviceArray<float4> samples;              // wave_queue: one float4 per (pixel, frame) of a launch
    size_t sample_budget = (size_t)1 << 30;   // frames of one batch are split so that a launch needs at most this much
    int num_cus = 256;
    int frames_in_flight = 1;                 // drt_renderer_set_frames_in_flight
    drt::Tuning tune;                         // the environment switches, read by drt_renderer_create
    drt::TracerChoice choice;                 // the tracing kernel of the last batch (choose_tracer) ...
    drt::LaunchShape shape;                   // ... and the shape of its last launch
    drt::WaveQueueCache wq_cache;             // measured choice among wave_queue's launch packagings
    drt::PoolScratch pool_scratch;
    uint32_t pool_t_class[3] = { 0, 0, 0 };   // leaf-size classes of the uploaded scene (path_pool's T queues)
    float pool_safe_dir = 0.0f;               // pool_safe_dir (pool_index.hpp) of the uploaded triangles' largest |edge component|; 0 once a refit has rewritten them on the device
    bool scene_has_alpha = false;
    int vote_node = 12, vote_shade = 44, vote_dir = 4, vote_spec = 8;
    int leaf_chain = -1;                              // DRT_LEAF_CHAIN: -1 = by tree depth (<= 4 levels), 0 / 1 = forced
    int vote_tail_node = 4, vote_tail_shade = 36;    // once the queue is empty (DRT_VOTE_TN / DRT_VOTE_TS): pops stop waiting for company   // wave_queue phase-voting thresholds (DRT_VOTE_N/S/R/P override)
    // device copy of the scene last rendered
    const drt_scene *uploaded_scene = nullptr;
    uint64_t uploaded_revision = 0;
    DeviceArray<drt::InnerNode> d_inner;
    DeviceArray<drt::LeafRange> d_leaves;
    DeviceArray<drt::TriHot> d_hot;
    DeviceArray<drt::TriCold> d_cold;
    DeviceArray<drt::MatDev> d_mats;
    DeviceArray<drt::MatExt> d_mats_ext;
    drt_material_model material_model = { 0, 0, 1.0f, 0 };       // emissive, specular, emissive_scale, transmission
    DeviceArray<drt::TexDev> d_texs;
    DeviceArray<uint8_t> d_texels;
    drt::SceneView view;
    int bvh_depth = 0;
    // batched ray queries (drt_renderer_trace_rays / _occluded): claim heads, HBM stack levels, and the event after the last
    // query launch -- the next query waits for it on its own stream (they share heads and stack), a scene re-upload on the host
    Event ev_query;
    hipStream_t query_stream = nullptr;
    bool query_recorded = false;
    DeviceArray<unsigned int> rq_heads;
    DeviceArray<uint32_t> rq_stack;
    // drt_renderer_plane_sections: the worklists of the wave-per-plane kernel (section.hpp: two lists of n_leaves words per wave of
    // the grid), grown on demand as rq_stack is; leaves_ascending = the uploaded tree's leaves, child 1 first, hold ascending
    // triangle ranges (the kernel's lists are sorted only then)
    DeviceArray<uint32_t> section_work;
    int section_waves = 0;                     // DRT_SECTION_WAVES: at most this many waves per launch (0 = no cap)
    bool leaves_ascending = true;
    // drt_renderer_chain_sections: the uploaded scene's edge adjacency (made by the first call after an upload, dropped with the scene
    // copy) and the scratch of kernel_contour.hip (contour.hpp: contour_scratch_words), grown on demand as section_work is
    DeviceArray<int32_t> d_adj;
    bool adj_built = false;
    bool adjacency_host = false;               // DRT_ADJACENCY=host: the table is the host's sort, uploaded (unset, or any other value: kernel_adjacency.hip)
    int adjacency_route = 0;                   // drt_renderer_adjacency_route: 0 = no table yet, 1 = made on the host, 2 = on the device
    DeviceArray<uint32_t> contour_work;
    // mesh topology (drt_capi_topology.cpp): what depends on the adjacency alone is made by the first call after an upload and lives as
    // long as d_adj does -- the shell labels, the counts {shells, open, bad half-edges} on the device and on the host, the ascending
    // list of boundary half-edges -- and the scratch of kernel_topology.hip (topology.hpp), grown on demand as contour_work is;
    // topo_steps = labelling steps {enqueued, that did something, that hooked} of the last labelling
    bool topo_built = false;
    DeviceArray<int32_t> topo_labels;
    DeviceArray<uint32_t> topo_counts, topo_boundary;
    uint32_t topo_counts_host[3] = { 0, 0, 0 };
    uint32_t topo_steps[3] = { 0, 0, 0 };
    DeviceArray<uint32_t> topo_work;
    drt::FilterKernel filter_kernel = drt::FilterKernel::automatic;      // DRT_FILTER_KERNEL=lds / taps: one a-trous kernel for every pass (unset, or any other value: launch_atrous's rule)
    int rq_refill_min = 16;                    // DRT_RQ_REFILL: idle lanes that make a wave claim new rays (64 = only when all are)
    // drt_renderer_denoise: frame 1's guides and the two float4 buffers the passes ping-pong between, allocated by the first call,
    // freed by resize; denoised = the one that holds the last result (-1: none yet)
    DeviceArray<drt_guide> dn_guides;
    DeviceArray<float4> dn_buf[2];
    int denoised = -1;
    Event ev_dn_start, ev_dn_stop;            // the timed span of a filter stage (stage_begin / stage_end)
    // drt_renderer_temporal_denoise: the ping-pong history (three float4 records per pixel and half), allocated by the first call,
    // freed by resize, destroy and drt_renderer_temporal_reset; tp_cur = the half the last call wrote (-1: no history), tp_cam =
    // that call's camera as a pinhole.  The filtered result lands in dn_buf.
    DeviceArray<float4> tp_hist[2][3];
    int tp_cur = -1;
    drt::PrevCamera tp_cam;
    // drt_renderer_refit: the uploaded scene's refit metadata (refit.hpp), built by the first refit after an upload and freed
    // with the scene copy; out = the root box and the error word the kernels leave
    bool rf_built = false;
    DeviceArray<int32_t> rf_order;
    DeviceArray<float4> rf_avg;
    DeviceArray<float> rf_ext;
    DeviceArray<drt::RefitLeaf> rf_leaves;
    DeviceArray<drt::RefitInner> rf_levels;
    DeviceArray<uint32_t> rf_height_begin;
    DeviceArray<float> rf_out;
    std::vector<uint32_t> rf_heights;
    int rf_top_nodes = drt::kRefitTopNodes;    // DRT_REFIT_TOP: 0 = one launch per height up to the root
    int rf_launches = 0;
    Event ev_rf_start, ev_rf_stop, ev_rf_dep;
    // drt_renderer_track_motion: mv_snap = the TriHot records as they were before the first refit since the last temporal call /
    // drt_renderer_motion_advance (valid while mv_armed; the buffer is kept for reuse, dropped with the scene copy),
    // mv_guides = drt_renderer_motion_vectors' guide buffer
    bool mv_track = false, mv_armed = false;
    DeviceArray<drt::TriHot> mv_snap;
    DeviceArray<drt_guide> mv_guides;
    // drt_renderer_upscale: us_guides = frame 1's guides at the frame size followed by those at the output size, us_out = the
    // upscaled image, float4[us_width * us_height]; allocated by the first call, again when the output size changes, freed by
    // resize and destroy (us_width == 0: no result yet)
    DeviceArray<drt_guide> us_guides;
    DeviceArray<float4> us_out;
    uint32_t us_width = 0, us_height = 0;
    // drt_renderer_render_adaptive: the per-pixel state (ad_state[0] = sum rgb and n, ad_state[1] = m1, m2, the last call's q and
    // count), the plan's arrays (weights, counts, offsets, the scan's block sums, the totals) and the ray list and sample buffer of
    // one pixel range; allocated by the first call (the last two grow with the largest range), freed by resize, re-shard,
    // destroy, drt_renderer_adaptive_reset and drt_renderer_reset (ad_state[0].ptr == nullptr: no state)
    DeviceArray<float4> ad_state[2];
    DeviceArray<uint32_t> ad_q, ad_counts, ad_offsets, ad_block_sums;
    DeviceArray<drt::AdaptiveTotals> ad_totals;
    DeviceArray<drt_path_ray> ad_rays;
    DeviceArray<float4> ad_samples;
    // surface lookups and sampling (drt_capi_surface.cpp): sf_normals = the host scene's vertex normals, float[n_tris][3][3] in tree
    // order, and sf_order = the load index of every triangle, both made by the first lookup after an upload and dropped with the scene
    // copy, as the topology labels are; the table and the scratch of a sample call (sf_cdf: n_tris words, sf_blocks: one per workgroup
    // of the scan, sf_amax: one word), grown on demand and recomputed by every call
    bool sf_built = false;
    DeviceArray<float> sf_normals;
    DeviceArray<int32_t> sf_order;
    DeviceArray<unsigned long long> sf_cdf, sf_blocks;
    DeviceArray<uint32_t> sf_amax;
    // ambient occlusion (drt_capi_ambient.cpp): the 64-bit claim heads of kernel_ambient.hip (the tile count of a call can pass 2^32;
    // kRqShards heads, ambient.hpp's kAoHeadStride words apart, zeroed on the stream before every launch) -- the HBM stack is rq_stack --
    // and the two counters of the counting build (drt_debug_ambient_stats)
    DeviceArray<unsigned long long> ao_heads, ao_stats;
    bool ao_stats_on = false;
    // generalised winding numbers (drt_capi_winding.cpp): one 32-byte moment per tree node (winding.hpp) and the sums a parent adds up,
    // made on the stream of the first winding call after an upload or a refit (wn_valid), kept until the next one, dropped with the
    // scene copy; the passes read the refit plan (rf_leaves, rf_levels, rf_heights)
    DeviceArray<drt::WindingMoment> wn_moments;
    DeviceArray<float4> wn_sums;
    bool wn_valid = false;
    // vertex welding, vertex normals and smoothing (drt_capi_weld.cpp): the scratch of kernel_weld.hip (weld.hpp), grown on demand as
    // sf_cdf is and recomputed by every call -- the table of corner indices, a word per corner, a word per workgroup of the scan; the
    // 64-bit fixed-point sums (and the counts behind them), the words of the maxima, the two position buffers the steps ping-pong between
    DeviceArray<uint32_t> wd_table, wd_rep, wd_blocks, wd_max;
    DeviceArray<unsigned long long> wd_acc;
    DeviceArray<float> wd_pos[2];
    // mesh simplification (drt_capi_simplify.cpp): the scratch of kernel_simplify.hip (simplify.hpp) beyond what it shares with the
    // welding calls above (the table, the representatives, the block totals, the maximum, the 64-bit sums) -- a key per vertex and a
    // member count per cluster
    DeviceArray<uint32_t> sp_key, sp_cnt;
    // mesh subdivision (drt_capi_subdivide.cpp): the scratch of kernel_subdivide.hip (subdivide.hpp) beyond what the adjacency of its
    // faces takes from the welding calls above -- that adjacency's own outputs (the twins, the edge of every half-edge, the
    // representative of every edge), the word E with Loop's two counts per vertex behind it, and Loop's second set of 64-bit sums
    // (the first lies in wd_acc)
    DeviceArray<int32_t> sd_adj, sd_edge, sd_half_edge;
    DeviceArray<uint32_t> sd_cnt;
    DeviceArray<unsigned long long> sd_acc;

    drt_renderer() = default;
    ~drt_renderer() {                          // the members release what they own, on this device
        (void)hipSetDevice(device);
        if (tune.stats) (void)hipFree(tune.stats);
        for (void *p : { pool_scratch.aux, pool_scratch.aux_slot, pool_scratch.aux_light, pool_scratch.aux_next, pool_scratch.aux_stack })
            if (p) (void)hipFree(p);
    }
    float *cur_accum() const { return ext_accum ? ext_accum : accum.ptr; }
    float *cur_rgba() const { return ext_rgba ? ext_rgba : rgba.ptr; }
    void free_scene() {
        d_inner.release(); d_leaves.release(); d_hot.release(); d_cold.release();
        d_mats.release(); d_mats_ext.release(); d_texs.release(); d_texels.release();
        rf_order.release(); rf_avg.release(); rf_ext.release(); rf_leaves.release(); rf_levels.release();
        rf_height_begin.release(); rf_out.release();
        rf_built = false;
        mv_snap.release();
        mv_armed = false;
        d_adj.release();
        adj_built = false;
        adjacency_route = 0;
        topo_labels.release(); topo_counts.release(); topo_boundary.release();
        topo_built = false;
        sf_normals.release(); sf_order.release();
        sf_built = false;
        wn_moments.release(); wn_sums.release();
        wn_valid = false;
        uploaded_scene = nullptr;
    }
    void free_upscale() {
        us_guides.release(); us_out.release();
        us_width = us_height = 0;
    }
    void free_denoise() {
        dn_guides.release(); dn_buf[0].release(); dn_buf[1].release();
        denoised = -1;
    }
    void free_temporal() {
        for (auto &half : tp_hist)
            for (auto &b : half) b.release();
        tp_cur = -1;
    }
    void free_adaptive() {
        ad_state[0].release(); ad_state[1].release();
        ad_q.release(); ad_counts.release(); ad_offsets.release(); ad_block_sums.release(); ad_totals.release();
        ad_rays.release(); ad_samples.release();
    }
    void free_stages() {                       // resize and re-shard: every stage's buffers are of the old frame
        free_denoise(); free_temporal(); mv_guides.release(); free_upscale(); free_adaptive();
    }
};

namespace drt {

// ------------------------------------------------------------------ steps that several entry points take (drt_capi.cpp)
int upload_scene(drt_renderer *r, const drt_scene *scene);       // ... and refuse a tree deeper than the traversal stacks
CamConst camera_const(const drt_camera *cam, float width, float height);
void fill_frame_params(const drt_renderer *r, const drt_camera *cam, FrameParams &fp, uint32_t width = 0, uint32_t height = 0);
bool on_renderer_device(const drt_renderer *r, const void *p);
// Ray queries, guide passes and radiance queries share claim heads and an HBM stack.  query_order: stream `s` waits for the last
// of them if that ran on another stream; query_recorded: the work just enqueued on `s` is the last of them; traversal_scratch: the
// stack for the uploaded tree (grown only once the query in flight is over) and, with `heads`, the claim heads zeroed on `s`.
int query_order(drt_renderer *r, hipStream_t s);
int query_recorded(drt_renderer *r, hipStream_t s);
int traversal_scratch(drt_renderer *r, hipStream_t s, bool occluded, bool heads);
// The opening every batched query's entry point shares (query_frame.hpp kernels), in the order the checks are documented in.
//   query_open   n < 2^31, no batch pending, the device, every operand that is not null on it, the scene uploaded, the stream chosen
//                and ordered behind the last query, the scratch for a stack of 4-byte (`occluded`) or 8-byte entries, the heads zeroed.
//                noun: "at most 2^31 - 1 <noun> per call"; names: "<names> must be device memory on the renderer's device".
//                An entry point with checks of its own before it (modes, capacities) makes those and calls this.
//   query_begin  for an entry point whose operands are all required: the handles, n == 0, the pointers, their alignment, then
//                query_open.  True: go on, on stream *s.  False: the call is over and returns *rc -- DRT_OK for n == 0, else the
//                error.  Use: `hipStream_t s; int rc; if (!query_begin(..., &s, &rc)) return rc;`
int query_open(drt_renderer *r, const drt_scene *scene, uint32_t n, std::initializer_list<const void *> operands, const char *noun,
               const char *names, void *hip_stream, bool occluded, hipStream_t *s);
struct QueryOperand { const void *p; size_t align; };
struct QueryWords { const char *null_msg, *align_msg, *noun, *names; };
bool query_begin(drt_renderer *r, const drt_scene *scene, uint32_t n, std::initializer_list<QueryOperand> ops, const QueryWords &w,
                 void *hip_stream, bool occluded, hipStream_t *s, int *rc);
// the levels a traversal stack is sized for: the uploaded tree's depth
uint32_t query_stack_levels(const drt_renderer *r);
// the frame of a launch over n queries, after query_open / traversal_scratch: tree depth, refill threshold, heads, HBM stack
QueryFrame query_frame(const drt_renderer *r, uint32_t n);
// The uploaded scene's edge adjacency in d_adj (drt_capi_adjacency.cpp), made by the first call after an upload on stream `s`, which
// the caller has ordered with the query in flight: by kernel_adjacency.hip from the host scene's positions, or by the host's sort
int scene_adjacency(drt_renderer *r, const drt_scene *scene, hipStream_t s);
// The uploaded scene's refit plan on the device (refit.hpp: the leaves, the interior nodes by height), made once per upload
int refit_metadata(drt_renderer *r, const drt_scene *scene);
// What a call on a finished frame starts with: a frame size, no pending batch, not sharded (`who`, e.g. "the denoiser needs", opens
// the message; nullptr = the caller calls whole_frame later), the renderer's device selected, no stale HIP error
int stage_open(drt_renderer *r, const char *who);
int whole_frame(const drt_renderer *r, const char *who);
int read_back(drt_renderer *r, const float *src, int comps, float *dst, size_t dst_floats);
// The timed span of a stage on the renderer's stream (drt_capi_filters.cpp): stage_begin opens it, stage_end closes it, waits and
// stores the device time
int stage_begin(drt_renderer *r);
int stage_end(drt_renderer *r, float *delta_ms);

}  // namespace drt

#pragma GCC visibility pop
