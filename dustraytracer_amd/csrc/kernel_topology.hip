// kernel_topology.hip -- mesh topology (include/drt.h "mesh topology"): the shell of every triangle, the loops of the boundary
// half-edges, and the per-triangle measure terms.  Labels and loops are integers read off the edge adjacency; no coordinate is read
// but by the terms.  One phase per launch; a phase reads what the launches before it wrote, and no workgroup waits for another one.
//
// Labelling (label[t] = the smallest triangle index of t's shell).  parent[t] <= t always, so following parents ends at a root
// (parent[r] == r) and never cycles; a link is only ever made between two triangles of one shell.  Steps of one kernel:
//   hook      one lane per half-edge h with a twin above it: the roots of the two triangles as the last jump step left them in label[]
//             (every tree is a star then, so these are exact), and atomicMin(parent[larger root], smaller root).  A root that several
//             twins hook keeps the smallest proposal; the others see different roots again in the next round.
//   jump      one lane per triangle: parent[t] = parent[parent[t]], in place (a racing read sees another ancestor, never a stranger),
//             label[t] = that ancestor.  A lane that still stands below a non-root asks for another jump step.
// What step k does follows from what step k - 1 did and whether it asked for more (mode[], more[]): a hook that hooked something is
// followed by jumps until every tree is a star, those by a hook, and a hook that hooked nothing is the end: then both triangles of
// every twin pair have one root, a shell has one root, and a root is at most each of its members and a member: the smallest.  Every
// later step returns at once.  The host enqueues steps in groups and looks at mode[] between them (topology.hpp: topo_max_steps).
//
// Loops.  The records are the boundary half-edges in ascending order (compacted by a two-level scan, as kernel_adaptive.hip scans its
// counts).  link: the rotation of drt.h about the record's end vertex, the record of the half-edge it ends at (binary search),
// succ[j] = m and atomicMin(pred[m], j); init / jump x R / tail / scan / scatter rank the paths and cycles as kernel_contour.hip does
// (pointer jumping along pred on 16-byte states, a cycle's start at its minimum, one flag per round that lets the rounds after the
// last busy one return at once), here with one range that is the whole list.
//
// Bounds on any table: a half-edge is checked against 3 * n_tris before it indexes adj; label and parent hold triangle indices; succ,
// pred and the states hold record indices below n_rec; a slot is written only below capacity and below n_rec.
#include <hip/hip_runtime.h>

#include "topology.hpp"

namespace drt {

namespace {

#define TP_DEV static __device__ __forceinline__

TP_DEV uint32_t relaxed_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
TP_DEV void relaxed_store(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// One flag for the next launch, not a count: a workgroup votes, and stores only while the flag still reads 0.  Ends with a barrier.
TP_DEV void vote(bool mine, uint32_t *flag) {
    const bool any = __syncthreads_or(mine) != 0;
    if (any && threadIdx.x == 0 && relaxed_load(flag) == 0u) relaxed_store(flag, 1u);
}

// ------------------------------------------------------------------------------------------------------------------ labelling
__global__ __launch_bounds__(kTopoThreads) void topo_label_init_kernel(const TopoLabelArgs a) {
    const uint32_t t = blockIdx.x * kTopoThreads + threadIdx.x;
    if (t >= a.n_tris) return;
    a.parent[t] = t;
    a.label[t] = (int32_t)t;
}

__global__ __launch_bounds__(kTopoThreads) void topo_label_step_kernel(const TopoLabelArgs a, uint32_t k) {
    uint32_t mode = kTopoHook;                           // step 0: every triangle is a star of its own
    if (k > 0) {
        const uint32_t did = a.mode[k - 1], more = a.more[k - 1];
        mode = did == kTopoDone ? kTopoDone : did == kTopoHook ? (more ? kTopoJump : kTopoDone) : (more ? kTopoJump : kTopoHook);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) a.mode[k] = mode;
    if (mode == kTopoDone) return;
    const uint32_t i = blockIdx.x * kTopoThreads + threadIdx.x;
    const uint32_t n_half = 3u * a.n_tris;
    bool ask = false;
    if (mode == kTopoHook) {
        if (i < n_half) {
            const int32_t twin = a.adj[i];
            if (twin > (int32_t)i && (uint32_t)twin < n_half) {              // each twin pair once, from its lower half-edge
                const uint32_t ru = (uint32_t)a.label[i / 3u], rv = (uint32_t)a.label[(uint32_t)twin / 3u];
                if (ru != rv) {
                    atomicMin(&a.parent[max(ru, rv)], min(ru, rv));
                    ask = true;
                }
            }
        }
    } else if (i < a.n_tris) {
        const uint32_t p = relaxed_load(&a.parent[i]);
        const uint32_t gp = relaxed_load(&a.parent[p]);
        if (gp != p) relaxed_store(&a.parent[i], gp);
        a.label[i] = (int32_t)gp;
        ask = relaxed_load(&a.parent[gp]) != gp;
    }
    vote(ask, &a.more[k]);
}

// ------------------------------------------------------------------------------------------------------------------ scans
struct Sums { uint32_t x, y, z; };
TP_DEV void add(Sums &s, const Sums t) { s.x += t.x; s.y += t.y; s.z += t.z; }

TP_DEV uint32_t wave_inclusive(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(v, d, 64);
        if (lane >= d) v += up;
    }
    return v;
}

// The exclusive prefix of this lane's `mine` among the workgroup's lanes and the workgroup's sums.  Ends with a barrier.
TP_DEV Sums block_exclusive(Sums mine, Sums *s_wave, Sums *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Sums incl = { wave_inclusive(mine.x), wave_inclusive(mine.y), wave_inclusive(mine.z) };
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    Sums before = { 0u, 0u, 0u }, all = { 0u, 0u, 0u };
#pragma unroll
    for (int w = 0; w < kTopoThreads / 64; w++) {
        const Sums t = s_wave[w];
        if (w < wave) add(before, t);
        add(all, t);
    }
    __syncthreads();
    *total = all;
    const Sums r = { before.x + incl.x - mine.x, before.y + incl.y - mine.y, before.z + incl.z - mine.z };
    return r;
}

// The block sums become their own exclusive prefix sums, in place, and the three totals go to `totals`: one workgroup, in chunks
// with a carry
__global__ __launch_bounds__(kTopoThreads) void topo_scan_sums_kernel(uint32_t *block_sums, uint32_t n_blocks, uint32_t *totals) {
    __shared__ Sums s_wave[kTopoThreads / 64];
    Sums carry = { 0u, 0u, 0u };
    for (uint32_t chunk = 0; chunk < n_blocks; chunk += kTopoThreads) {
        const uint32_t b = chunk + threadIdx.x;
        Sums mine = { 0u, 0u, 0u };
        if (b < n_blocks) { mine.x = block_sums[3u * b]; mine.y = block_sums[3u * b + 1]; mine.z = block_sums[3u * b + 2]; }
        Sums total;
        const Sums before = block_exclusive(mine, s_wave, &total);
        if (b < n_blocks) {
            block_sums[3u * b] = carry.x + before.x;
            block_sums[3u * b + 1] = carry.y + before.y;
            block_sums[3u * b + 2] = carry.z + before.z;
        }
        add(carry, total);
    }
    if (threadIdx.x == 0 && totals) { totals[0] = carry.x; totals[1] = carry.y; totals[2] = carry.z; }
}

// ------------------------------------------------------------------------------------------------------------------ counts
// what half-edge h adds: {its triangle is a root (counted at edge 0), it is open, it is bad}
TP_DEV Sums count_term(const TopoCountArgs &a, uint32_t h) {
    Sums t = { 0u, 0u, 0u };
    if (h >= 3u * a.n_tris) return t;
    const uint32_t tri = h / 3u;
    if (h == 3u * tri && a.label[tri] == (int32_t)tri) t.x = 1u;
    const int32_t twin = a.adj[h];
    t.y = twin == -1 ? 1u : 0u;
    t.z = twin == -2 ? 1u : 0u;
    return t;
}

__global__ __launch_bounds__(kTopoThreads) void topo_count_sums_kernel(const TopoCountArgs a) {
    __shared__ Sums s_wave[kTopoThreads / 64];
    const uint32_t first = blockIdx.x * kTopoScanBlock + threadIdx.x * kTopoScanItems;
    Sums mine = { 0u, 0u, 0u };
#pragma unroll
    for (int k = 0; k < kTopoScanItems; k++) add(mine, count_term(a, first + k));
    Sums total;
    (void)block_exclusive(mine, s_wave, &total);
    if (threadIdx.x == 0) {
        a.block_sums[3u * blockIdx.x] = total.x;
        a.block_sums[3u * blockIdx.x + 1] = total.y;
        a.block_sums[3u * blockIdx.x + 2] = total.z;
    }
}

__global__ __launch_bounds__(kTopoThreads) void topo_compact_kernel(const TopoCountArgs a, uint32_t n_boundary) {
    __shared__ Sums s_wave[kTopoThreads / 64];
    const uint32_t first = blockIdx.x * kTopoScanBlock + threadIdx.x * kTopoScanItems;
    Sums v[kTopoScanItems], mine = { 0u, 0u, 0u };
#pragma unroll
    for (int k = 0; k < kTopoScanItems; k++) {
        v[k] = count_term(a, first + k);
        add(mine, v[k]);
    }
    Sums total;
    const Sums run = block_exclusive(mine, s_wave, &total);
    uint32_t pos = run.y + a.block_sums[3u * blockIdx.x + 1];
#pragma unroll
    for (int k = 0; k < kTopoScanItems; k++) {
        if (v[k].y && pos < n_boundary) a.boundary[pos] = first + k;
        pos += v[k].y;
    }
}

// ------------------------------------------------------------------------------------------------------------------ loops
__global__ __launch_bounds__(kTopoThreads) void topo_link_kernel(const TopoLoopArgs a) {
    const uint32_t j = blockIdx.x * kTopoThreads + threadIdx.x;
    if (j >= a.n_rec) return;
    const uint32_t n_half = 3u * a.n_tris;
    const uint32_t h = a.boundary[j];
    uint32_t link = kTopoFlag | 2u;
    if (h < n_half) {
        // drt.h "successor": rotate about the end vertex of h through the twins, to the half-edge that leaves it on the boundary
        uint32_t tri = h / 3u, e = h - 3u * tri;
        uint32_t g = 3u * tri + (e == 2u ? 0u : e + 1u);
        int32_t twin = a.adj[g];
        for (uint32_t guard = n_half; twin >= 0; guard--) {
            if ((uint32_t)twin >= n_half || guard == 0u) { twin = -2; break; }
            tri = (uint32_t)twin / 3u; e = (uint32_t)twin - 3u * tri;
            g = 3u * tri + (e == 2u ? 0u : e + 1u);
            twin = a.adj[g];
        }
        if (twin == -1) {
            uint32_t lo = 0, hi = a.n_rec;
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (a.boundary[mid] < g) lo = mid + 1;
                else hi = mid;
            }
            if (lo < a.n_rec && a.boundary[lo] == g) {
                link = lo;
                atomicMin(&a.pred[lo], j);       // (the rotation is injective: the minimum is the only writer of its word)
            }
        }
    }
    a.succ[j] = link;
}

__global__ __launch_bounds__(kTopoThreads) void topo_init_kernel(const TopoLoopArgs a) {
    const uint32_t j = blockIdx.x * kTopoThreads + threadIdx.x;
    if (j >= a.n_rec) return;
    const uint32_t link = a.succ[j];
    if (!(link & kTopoFlag) && a.pred[link] != j) a.succ[j] = kTopoFlag | 2u;      // succ and pred are exact inverses on any table
    const uint32_t p = a.pred[j];
    a.state[0][j] = p == kTopoNone ? make_uint4(j | kTopoFlag, 0u, j, 0u) : make_uint4(p, 0u, j, 0u);
}

__global__ __launch_bounds__(kTopoThreads) void topo_jump_kernel(const TopoLoopArgs a, int round) {
    if (round > 0 && a.moved[round] == 0u) return;       // the round before moved nothing: every later round returns here
    const uint32_t j = blockIdx.x * kTopoThreads + threadIdx.x;
    bool moved = false;
    if (j < a.n_rec) {
        const uint4 *from = a.state[round & 1];
        uint4 s = from[j];
        if (!(s.x & kTopoFlag)) {
            const uint4 far = from[s.x];
            const uint32_t step = 1u << round;          // the records between j and its ancestor
            if (far.x & kTopoFlag) {
                s = make_uint4(far.x, step + far.y, s.z, 0u);
                moved = true;
            } else {
                if (far.z < s.z) {
                    s.z = far.z; s.y = step + far.y;
                    moved = true;
                }
                s.x = far.x;
            }
        }
        a.state[(round + 1) & 1][j] = s;
    }
    vote(moved, &a.moved[round + 1]);
}

// What the jumping left of record j: its loop's first record, its rank in the loop, and whether the loop is closed
struct Ranked { uint32_t start, rank; bool closed; };
TP_DEV Ranked ranked(const uint4 s) {
    Ranked r;
    r.closed = !(s.x & kTopoFlag);
    r.start = r.closed ? s.z : (s.x & ~kTopoFlag);
    r.rank = s.y;
    return r;
}

__global__ __launch_bounds__(kTopoThreads) void topo_tail_kernel(const TopoLoopArgs a, const uint4 *state) {
    const uint32_t j = blockIdx.x * kTopoThreads + threadIdx.x;
    if (j >= a.n_rec) return;
    const Ranked r = ranked(state[j]);
    const uint32_t link = a.succ[j];
    if ((link & kTopoFlag) || (r.closed && link == r.start)) a.length[r.start] = r.rank + 1u;     // one writer per loop
}

// what record j adds to the scans: {its loop's length, 1, 1 if closed} at a loop's first record
TP_DEV Sums loop_term(const TopoLoopArgs &a, const uint4 *state, uint32_t j) {
    Sums t = { 0u, 0u, 0u };
    if (j >= a.n_rec) return t;
    const Ranked r = ranked(state[j]);
    if (r.start != j) return t;
    t.x = a.length[j];
    t.y = 1u;
    t.z = r.closed ? 1u : 0u;
    return t;
}

__global__ __launch_bounds__(kTopoThreads) void topo_loop_sums_kernel(const TopoLoopArgs a, const uint4 *state) {
    __shared__ Sums s_wave[kTopoThreads / 64];
    const uint32_t first = blockIdx.x * kTopoScanBlock + threadIdx.x * kTopoScanItems;
    Sums mine = { 0u, 0u, 0u };
#pragma unroll
    for (int k = 0; k < kTopoScanItems; k++) add(mine, loop_term(a, state, first + k));
    Sums total;
    (void)block_exclusive(mine, s_wave, &total);
    if (threadIdx.x == 0) {
        a.block_sums[3u * blockIdx.x] = total.x;
        a.block_sums[3u * blockIdx.x + 1] = total.y;
        a.block_sums[3u * blockIdx.x + 2] = total.z;
    }
}

__global__ __launch_bounds__(kTopoThreads) void topo_offsets_kernel(const TopoLoopArgs a, const uint4 *state) {
    __shared__ Sums s_wave[kTopoThreads / 64];
    const uint32_t first = blockIdx.x * kTopoScanBlock + threadIdx.x * kTopoScanItems;
    uint32_t v[kTopoScanItems];
    Sums mine = { 0u, 0u, 0u };
#pragma unroll
    for (int k = 0; k < kTopoScanItems; k++) {
        v[k] = loop_term(a, state, first + k).x;
        mine.x += v[k];
    }
    Sums total;
    uint32_t run = block_exclusive(mine, s_wave, &total).x + a.block_sums[3u * blockIdx.x];
#pragma unroll
    for (int k = 0; k < kTopoScanItems; k++) {
        if (first + k < a.n_rec) a.pred[first + k] = run;       // (the predecessors are spent: the positions)
        run += v[k];
    }
}

__global__ __launch_bounds__(kTopoThreads) void topo_scatter_kernel(const TopoLoopArgs a, const uint4 *state) {
    const uint32_t j = blockIdx.x * kTopoThreads + threadIdx.x;
    if (j >= a.n_rec) return;
    const Ranked r = ranked(state[j]);
    const uint32_t link = a.succ[j];
    const uint32_t status = (link & kTopoFlag) ? (link & 7u) : 0u;
    const uint32_t first = a.pred[r.start], length = a.length[r.start];
    const uint32_t pos = first + r.rank;
    if (pos >= first && pos < a.n_rec && pos < a.capacity)
        reinterpret_cast<uint4 *>(a.slots)[pos] = make_uint4(a.boundary[j], first, length, (r.closed ? 1u : 0u) | (status << 1));
}

// ------------------------------------------------------------------------------------------------------------------ terms
// drt.h "measure terms": float64, every product and sum rounded on its own (-ffp-contract=off), no square root
__global__ __launch_bounds__(kTopoThreads) void topo_terms_kernel(const TriHot *tris, uint32_t n_tris, double *terms) {
    const uint32_t t = blockIdx.x * kTopoThreads + threadIdx.x;
    if (t >= n_tris) return;
    const float4 *q = reinterpret_cast<const float4 *>(tris + t);
    const float4 a = q[0], b = q[1];
    const float last = reinterpret_cast<const float *>(&q[2])[0];
    const double v0x = a.x, v0y = a.y, v0z = a.z;
    const double e1x = a.w, e1y = b.x, e1z = b.y;
    const double e2x = b.z, e2y = b.w, e2z = last;
    const double cx = e1y * e2z - e1z * e2y;
    const double cy = e1z * e2x - e1x * e2z;
    const double cz = e1x * e2y - e1y * e2x;
    const double w = (v0x * cx + v0y * cy) + v0z * cz;
    double2 *out = reinterpret_cast<double2 *>(terms) + 2 * (size_t)t;
    out[0] = make_double2(cx, cy);
    out[1] = make_double2(cz, w);
}

dim3 lanes(uint32_t n) { return dim3((n + kTopoThreads - 1) / kTopoThreads); }

}  // namespace

hipError_t launch_topo_label_init(const TopoLabelArgs &a, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(a.mode, 0, 2 * ((size_t)topo_max_steps(a.n_tris) + 1) * sizeof(uint32_t), stream);      // mode and more
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(topo_label_init_kernel, lanes(a.n_tris), dim3(kTopoThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_topo_label_steps(const TopoLabelArgs &a, uint32_t first, uint32_t count, hipStream_t stream) {
    for (uint32_t k = first; k < first + count; k++)
        hipLaunchKernelGGL(topo_label_step_kernel, lanes(3u * a.n_tris), dim3(kTopoThreads), 0, stream, a, k);
    return hipGetLastError();
}

hipError_t launch_topo_counts(const TopoCountArgs &a, hipStream_t stream) {
    const uint32_t n_blocks = topo_scan_blocks(3u * a.n_tris);
    hipLaunchKernelGGL(topo_count_sums_kernel, dim3(n_blocks), dim3(kTopoThreads), 0, stream, a);
    hipLaunchKernelGGL(topo_scan_sums_kernel, dim3(1), dim3(kTopoThreads), 0, stream, a.block_sums, n_blocks, a.counts);
    return hipGetLastError();
}

hipError_t launch_topo_compact(const TopoCountArgs &a, uint32_t n_boundary, hipStream_t stream) {
    hipLaunchKernelGGL(topo_compact_kernel, dim3(topo_scan_blocks(3u * a.n_tris)), dim3(kTopoThreads), 0, stream, a, n_boundary);
    return hipGetLastError();
}

hipError_t launch_topo_loops(const TopoLoopArgs &a, hipStream_t stream) {
    const int rounds = topo_log2_ceil(a.n_rec);
    const dim3 block(kTopoThreads);
    const dim3 grid = lanes(a.n_rec);
    const uint32_t n_blocks = topo_scan_blocks(a.n_rec);
    hipError_t e = hipMemsetAsync(a.moved, 0, (kTopoMaxRounds + 1) * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(a.pred, 0xff, (size_t)a.n_rec * sizeof(uint32_t), stream);       // no predecessor
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(topo_link_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(topo_init_kernel, grid, block, 0, stream, a);
    for (int k = 0; k < rounds; k++) hipLaunchKernelGGL(topo_jump_kernel, grid, block, 0, stream, a, k);
    const uint4 *state = a.state[rounds & 1];
    hipLaunchKernelGGL(topo_tail_kernel, grid, block, 0, stream, a, state);
    hipLaunchKernelGGL(topo_loop_sums_kernel, dim3(n_blocks), block, 0, stream, a, state);
    hipLaunchKernelGGL(topo_scan_sums_kernel, dim3(1), block, 0, stream, a.block_sums, n_blocks, a.counts);
    if (a.slots && a.capacity) {
        hipLaunchKernelGGL(topo_offsets_kernel, dim3(n_blocks), block, 0, stream, a, state);
        hipLaunchKernelGGL(topo_scatter_kernel, grid, block, 0, stream, a, state);
    }
    return hipGetLastError();
}

hipError_t launch_topo_terms(const TriHot *tris, uint32_t n_tris, double *terms, hipStream_t stream) {
    hipLaunchKernelGGL(topo_terms_kernel, lanes(n_tris), dim3(kTopoThreads), 0, stream, tris, n_tris, terms);
    return hipGetLastError();
}

}  // namespace drt
