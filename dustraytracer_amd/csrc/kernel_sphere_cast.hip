// kernel_sphere_cast.hip -- batched sphere casts for gfx950: the first contact of a sphere moving along a segment with the mesh
// (drt_renderer_sphere_cast).  The reference has no such query; include/drt.h states the rule, and every line below that computes
// a value cites the part of it that it implements.
//
//   triangle   the centre enters the triangle's offset volume = the union of seven overlapping convex shapes: the prism over the
//              face, a whole cylinder round each edge, a whole sphere at each vertex.  Each shape has a containment branch
//              (the centre starts inside: tau = 0, feature + 8) and an entry branch (a quotient of two positive numbers); the
//              triangle's candidate is the minimum of t = tmin + tau over the seven, strict <, in feature order
//   box        the node's box inflated by r, slab-tested with inv_dir: visited iff enter <= exit, exit >= tmin, enter <= best
//   traversal  best = tmax; a popped entry is dropped unless enter <= best; a leaf's triangles in order, a candidate wins on
//              t < best or t == best with a smaller triangle index; an interior node pushes the farther child first
//
// Grid, claim and stack: query_frame.hpp.  One cast per lane; stack entries {ref, enter}, kRqLdsLevelsClosest levels in LDS.
//
// The triangle test fits the ray queries' 64 VGPRs (8 waves per SIMD), so the grid is theirs.  The square root and the quotient
// of a shape are computed only by the lanes whose cheap conditions hold (approaching, disc >= 0).
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "device_scene.hpp"
#include "device_access.hpp"
#include "sphere_cast.hpp"
#include "query_frame.hpp"

namespace drt {

namespace {

// drt.h "traversal": the box inflated by r on every side against the ray (o, inv_dir); fminf / fmaxf drop a NaN operand (0 * inf)
DRT_DEV bool inflated_slab(f3 bmin, f3 bmax, float r, f3 o, f3 inv_dir, float tmin, float best, float &enter) {
    const f3 t0 = (sub_scalar(bmin, r) - o) * inv_dir;
    const f3 t1 = (add_scalar(bmax, r) - o) * inv_dir;
    const f3 lo = mk3(fminf(t0.x, t1.x), fminf(t0.y, t1.y), fminf(t0.z, t1.z));
    const f3 hi = mk3(fmaxf(t1.x, t0.x), fmaxf(t1.y, t0.y), fmaxf(t1.z, t0.z));
    enter = fmaxf(fmaxf(lo.x, lo.y), lo.z);
    const float exit = fminf(fminf(hi.x, hi.y), hi.z);
    return enter <= exit && exit >= tmin && enter <= best;
}

// A shape's candidate against the triangle's: drt.h takes the shapes in feature order and replaces on a strict <, which is "the
// smallest t, and among equal t the lowest feature"; said that way, the shapes can be computed in any order (sweep_triangle goes
// vertex by vertex, so that only one vertex's differences are live at a time).
DRT_DEV void take(float t, int f, bool inside, float &tt, int &feat) {
    if (t < tt || (t == tt && f < (feat & 7))) { tt = t; feat = inside ? f + 8 : f; }
}

// drt.h "edges": the whole cylinder of radius r round the line (a, e), cut to the axial range [0, ee].  m = s - a, md = dot(m, d),
// c = dot(m, m) - r2 are the values of the vertex at a.  The discriminant comes from x = cross(d, e) and the triple product
// dot(m, x): B B - A Cq in exact arithmetic, without the cancellation that grows with the distance of the start.
DRT_DEV void edge_candidate(f3 m, float md, float c, f3 e, float ee, f3 d, float r2, float tmin, int f, float &tt, int &feat) {
    const float me = dot(m, e), de = dot(d, e);
    const float Cq = ee * c - me * me;
    const bool inside = Cq <= 0.0f;
    bool ok = inside;
    float tau = 0.0f;
    if (!inside) {
        const f3 x = cross(d, e);
        const float det = dot(m, x);
        const float A = dot(x, x), B = ee * md - de * me;
        if (A > 0.0f && B < 0.0f) {
            const float disc = ee * (A * r2 - det * det);
            if (disc >= 0.0f) { tau = Cq / (exact_sqrt(disc) - B); ok = true; }
        }
    }
    if (ok) {
        const float ax = me + tau * de, t = tmin + tau;
        if (ee > 0.0f && ax >= 0.0f && ax <= ee) take(t, f, inside, tt, feat);
    }
}

// drt.h "vertices": the whole sphere of radius r at the vertex.  m = s - p, b = dot(m, d), c = dot(m, m) - r2; the discriminant
// b b - dd c as dd r2 - |cross(m, d)|^2.
DRT_DEV void vertex_candidate(f3 m, float b, float c, f3 d, float dd, float r2, float tmin, int f, float &tt, int &feat) {
    const bool inside = c <= 0.0f;
    bool ok = inside;
    float tau = 0.0f;
    if (!inside && dd > 0.0f && b < 0.0f) {
        const f3 x = cross(m, d);
        const float disc = dd * r2 - dot(x, x);
        if (disc >= 0.0f) { tau = c / (exact_sqrt(disc) - b); ok = true; }
    }
    if (ok) {
        take(tmin + tau, f, inside, tt, feat);
    }
}

// drt.h "per triangle": the smallest t = tmin + tau over the seven shapes (+inf: none) and its feature
DRT_DEV float sweep_triangle(f3 s, f3 d, float dd, float r, float r2, float tmin, f3 v0, f3 e1, f3 e2, int &feat) {
    float tt = __builtin_inff();
    feat = -1;
    const float d11 = dot(e1, e1), d22 = dot(e2, e2), d12 = dot(e1, e2);
    const f3 m0 = s - v0;
    {   // face (feature 0)
        const f3 n = cross(e1, e2);
        const float k = r * exact_sqrt(dot(n, n));
        const float h = dot(n, m0), dn = dot(n, d);
        const float ah = __builtin_fabsf(h);
        const bool inside = ah <= k;
        if (inside || (h > 0.0f && dn < 0.0f) || (h < 0.0f && dn > 0.0f)) {
            const float tau = inside ? 0.0f : (ah - k) / __builtin_fabsf(dn);
            const f3 q = m0 + d * tau;
            const float q1 = dot(q, e1), q2 = dot(q, e2);
            const float nu = d22 * q1 - d12 * q2, nv = d11 * q2 - d12 * q1, den = d11 * d22 - d12 * d12;
            const float t = tmin + tau;
            if (den > 0.0f && nu >= 0.0f && nv >= 0.0f && nu + nv <= den && t < tt) { tt = t; feat = inside ? 8 : 0; }
        }
    }
    {   // the shapes at p0: edges 1 and 2, vertex 4
        const float b0 = dot(m0, d), c0 = dot(m0, m0) - r2;
        edge_candidate(m0, b0, c0, e1, d11, d, r2, tmin, 1, tt, feat);
        edge_candidate(m0, b0, c0, e2, d22, d, r2, tmin, 2, tt, feat);
        vertex_candidate(m0, b0, c0, d, dd, r2, tmin, 4, tt, feat);
    }
    {   // at p1: edge 3, vertex 5
        const f3 m1 = s - (v0 + e1), e3 = e2 - e1;
        const float b1 = dot(m1, d), c1 = dot(m1, m1) - r2;
        edge_candidate(m1, b1, c1, e3, dot(e3, e3), d, r2, tmin, 3, tt, feat);
        vertex_candidate(m1, b1, c1, d, dd, r2, tmin, 5, tt, feat);
    }
    {   // at p2: vertex 6
        const f3 m2 = s - (v0 + e2);
        vertex_candidate(m2, dot(m2, d), dot(m2, m2) - r2, d, dd, r2, tmin, 6, tt, feat);
    }
    return tt;
}

// drt.h "result": (u, v) of the contact on the winning triangle from the centre cc = o + d t, by the feature touched
DRT_DEV void contact_uv(f3 cc, f3 v0, f3 e1, f3 e2, int f, float &u, float &v) {
    const f3 q = cc - v0;
    const float d11 = dot(e1, e1), d22 = dot(e2, e2);
    if (f == 0) {
        const float d12 = dot(e1, e2), q1 = dot(q, e1), q2 = dot(q, e2);
        const float nu = d22 * q1 - d12 * q2, nv = d11 * q2 - d12 * q1, den = d11 * d22 - d12 * d12;
        u = nu / den; v = nv / den;
    } else if (f == 1) {
        u = fminf(fmaxf(dot(q, e1) / d11, 0.0f), 1.0f); v = 0.0f;
    } else if (f == 2) {
        u = 0.0f; v = fminf(fmaxf(dot(q, e2) / d22, 0.0f), 1.0f);
    } else if (f == 3) {
        const f3 e3 = e2 - e1;
        const float w = fminf(fmaxf(dot(q - e1, e3) / dot(e3, e3), 0.0f), 1.0f);
        u = 1.0f - w; v = w;
    } else {
        u = f == 5 ? 1.0f : 0.0f; v = f == 6 ? 1.0f : 0.0f;
    }
}

__global__ __launch_bounds__(kRqThreads, kRqWavesPerSimd) void sphere_cast_kernel(const SceneView sc, const SphereCastArgs a) {
    constexpr int K = kRqLdsLevelsClosest;
    __shared__ uint32_t s_ref[K][kRqThreads];
    __shared__ float s_enter[K][kRqThreads];
    const int tid = threadIdx.x;
    const uint32_t gthread = blockIdx.x * kRqThreads + tid;
    const StackLane st = {tid, gthread, gridDim.x * kRqThreads, a.frame.stack_levels, a.frame.stack_hbm};
    uint32_t shard = home_shard(gthread);
    int shards_empty = 0;

    int rid = -1;                                            // this lane's cast, -1 = idle
    f3 o = mk3(0.f, 0.f, 0.f), d = o, inv_dir = o, s = o;
    float tmin = 0.f, r = 0.f, dd = 0.f;
    float best = 0.f;                                        // the first contact so far (prim -1 = none: best = tmax)
    int best_prim = -1, best_feat = -1;
    uint32_t sp = 0;

    for (;;) {
        // ---- refill: claim casts for the idle lanes (wave-uniform) ----
        const uint64_t idle = __ballot(rid < 0);
        if (claim_due(shards_empty, idle, a.frame)) {
            const bool was_idle = rid < 0;
            const Claimed c = claim_take(shard, shards_empty, rid, idle, a.frame);
            shard = c.shard; shards_empty = c.shards_empty; rid = c.rid;
            if (was_idle && rid >= 0) {
                // a new cast: two 16-byte loads (drt_ray = org, tmin, dir, tmax) and its radius
                const float4 *q = reinterpret_cast<const float4 *>(a.rays) + 2 * (size_t)(uint32_t)rid;
                const float4 q0 = q[0], q1 = q[1];
                o = mk3(q0.x, q0.y, q0.z); d = mk3(q1.x, q1.y, q1.z);
                tmin = q0.w;
                r = a.radii[(uint32_t)rid];
                inv_dir = mk3(exact_rcp(d.x), exact_rcp(d.y), exact_rcp(d.z));
                s = o + d * tmin;                                                       // the start centre
                dd = dot(d, d);
                best = q1.w; best_prim = -1; best_feat = -1; sp = 0;
                // a negative or NaN radius, a NaN in the origin or the direction: a miss that visits nothing (the slab test would drop a
                // NaN axis; a NaN tmin or tmax fails it on its own)
                const bool valid = r >= 0.0f && o.x == o.x && o.y == o.y && o.z == o.z && d.x == d.x && d.y == d.y && d.z == d.z;
                if (sc.root_ref != kNoNode && valid) {
                    float enter;
                    if (inflated_slab(ld3(sc.root_min), ld3(sc.root_max), r, o, inv_dir, tmin, best, enter)) {
                        s_ref[0][tid] = sc.root_ref; s_enter[0][tid] = enter; sp = 1;
                    }
                }
            }
        }
        if (claim_drained(shards_empty, rid)) break;

        // ---- one traversal step per busy lane ----
        if (rid >= 0 && sp > 0) {
            float enter;
            const uint32_t ref = stack_pop(s_ref, s_enter, st, sp, enter);
            if (enter <= best) {
                if (ref & kLeafBit) {
                    const LeafRange leaf = sc.leaves[ref & ~kLeafBit];
                    const float r2 = r * r;
                    for (int i = leaf.start; i < leaf.start + leaf.count; i++) {
                        const TriTest tri = load_tri(sc.tri_hot, i);
                        int feat;
                        const float t = sweep_triangle(s, d, dd, r, r2, tmin, tri.v0, tri.e1, tri.e2, feat);
                        // t < tmax is t < best here (best <= tmax); a NaN never wins
                        if (t < best || (t == best && i < best_prim)) { best = t; best_prim = i; best_feat = feat; }
                    }
                } else {
                    const ChildPair c = load_children(sc.inner, ref);
                    float en1, en2;
                    const bool push1 = inflated_slab(c.min1, c.max1, r, o, inv_dir, tmin, best, en1);
                    const bool push2 = inflated_slab(c.min2, c.max2, r, o, inv_dir, tmin, best, en2);
                    push_far_first(s_ref, s_enter, st, sp, c.ref1, en1, push1, c.ref2, en2, push2);        // farther child first
                }
            }
        }

        // ---- finished lanes write their result and go idle ----
        if (rid >= 0 && sp == 0) {                                  // (rid < n: the claim never hands out more)
            // a miss carries the ray's own tmax word: read again here, not held in a register through the traversal
            const float tmax = reinterpret_cast<const float *>(a.rays)[8 * (size_t)(uint32_t)rid + 7];
            float4 o0 = make_float4(tmax, __int_as_float(-1), 0.f, 0.f), o1 = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
            if (best_prim >= 0) {
                // (u, v) and the point are those of the winning (prim, feature, t), computed once
                const TriTest tri = load_tri(sc.tri_hot, best_prim);
                float u, v;
                contact_uv(o + d * best, tri.v0, tri.e1, tri.e2, best_feat & 7, u, v);
                const f3 p = (tri.v0 + tri.e1 * u) + tri.e2 * v;
                o0 = make_float4(best, __int_as_float(best_prim), u, v);
                o1 = make_float4(p.x, p.y, p.z, __int_as_float(best_feat));
            }
            float4 *out = reinterpret_cast<float4 *>(a.out) + 2 * (size_t)(uint32_t)rid;
            out[0] = o0; out[1] = o1;
            rid = -1; best_prim = -1;
        }
    }
}

}  // namespace

hipError_t launch_sphere_cast(const SceneView &sc, const SphereCastArgs &args, int num_cus, hipStream_t stream) {
    if (args.frame.n == 0) return hipSuccess;
    const uint32_t blocks = query_blocks(args.frame.n, num_cus);
    hipLaunchKernelGGL(sphere_cast_kernel, dim3(blocks), dim3(kRqThreads), 0, stream, sc, args);
    return hipGetLastError();
}

}  // namespace drt
