// section.hpp -- launch seam of kernel_section.hip (plane sections, the segments where each plane cuts the mesh: include/drt.h
// drt_renderer_plane_sections), the sizing of its grid and scratch, the host's check of the leaf order, and the query's routines: the
// load of a drt_plane, its validity, the signed value, the node cull and the cut of one triangle.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device_scene.hpp"
#ifdef __HIP__
#include "device_math.hpp"
#endif
#include "ray_query.hpp"
#include "section_order.hpp"

namespace drt {

constexpr int kSectionThreads = 256;            // 4 waves per workgroup; a wave never talks to another one
constexpr int kSectionBoundWavesPerSimd = 5;    // the launch bound: room for the 80 VGPRs of mode LIST without a spill ...
constexpr int kSectionWavesPerSimd = 6;         // ... and what 80 VGPRs attain: the wave slots the persistent grid is sized by
// Worklist scratch of one launch: 2 * n_leaves words per wave.  256 MiB holds the two lists of every wave slot of the chip
// (256 CUs x 4 SIMDs x 6 = 6144 waves) up to 5461 leaves, and still 64 waves -- one per plane of a small batch -- at half a million
// leaves (about ten million triangles at the default leaf target); it is about a tenth of a percent of the card's 288 GB, and a
// larger budget would only buy waves for trees whose planes already list tens of thousands of segments each.
constexpr size_t kSectionScratchBudget = (size_t)256 << 20;

struct SectionArgs {
    const void *planes;          // drt_plane[n] (16 B, 16-B aligned)
    const uint32_t *offsets;     // n + 1 words: plane i owns out[offsets[i] .. offsets[i + 1]), clamped to out_capacity (LIST only)
    void *out;                   // drt_section[out_capacity] (32 B, 16-B aligned); null when out_capacity == 0
    uint32_t *counts;            // n words or null: LIST every cut triangle of the plane, ANY 0 or 1
    uint32_t out_capacity;
    uint32_t n;                  // < 2^31
    uint32_t waves;              // waves of the grid that work: section_waves()
    uint32_t list_words;         // words of ONE worklist = max(n_leaves, 1); a wave owns work[2 * list_words * wave ..)
    unsigned int *heads;         // kRqHeadWords zeroed words (the ray queries' sharded claim heads)
    uint32_t *work;              // waves * 2 * list_words words
};

inline size_t section_bytes_per_wave(uint32_t n_leaves) { return (size_t)2 * std::max<uint32_t>(n_leaves, 1u) * sizeof(uint32_t); }
// waves of a launch: min(n, the chip's wave slots, budget / bytes per wave, the DRT_SECTION_WAVES cap if one is set), at least one
inline uint32_t section_waves(uint32_t n, int num_cus, uint32_t n_leaves, int env_cap) {
    size_t w = (size_t)std::max(1, num_cus) * 4 * kSectionWavesPerSimd;
    w = std::min<size_t>(w, n);
    w = std::min<size_t>(w, kSectionScratchBudget / section_bytes_per_wave(n_leaves));
    if (env_cap > 0) w = std::min<size_t>(w, (size_t)env_cap);
    return (uint32_t)std::max<size_t>(w, 1);
}

// (section_order.hpp: section_leaves_ascending, the host's check that the kernel's lists come out sorted)

// any_mode: DRT_SECTION_ANY (the work ends at the first chunk of leaves with a cut triangle) or DRT_SECTION_LIST
hipError_t launch_section(const SceneView &scene, bool any_mode, const SectionArgs &args, hipStream_t stream);

#ifdef __HIP__                                      // device code: the .hip translation units only
struct SectionPlane { f3 n; float d; };
DRT_DEV SectionPlane section_load_plane(const void *planes, uint32_t i) {
    const float4 a = reinterpret_cast<const float4 *>(planes)[i];
    SectionPlane p;
    p.n = mk3(a.x, a.y, a.z); p.d = a.w;
    return p;
}

// drt.h "query": valid iff all four words satisfy fabsf(x) <= FLT_MAX
DRT_DEV bool section_valid(const SectionPlane &p) {
    return fabsf(p.n.x) <= 3.402823466e+38f && fabsf(p.n.y) <= 3.402823466e+38f && fabsf(p.n.z) <= 3.402823466e+38f &&
           fabsf(p.d) <= 3.402823466e+38f;
}

// drt.h "signed value": s(x) = dot(n, x) - d
DRT_DEV float section_signed(const SectionPlane &p, f3 x) { return dot(p.n, x) - p.d; }

// drt.h "node cull": cmin[j] = n[j] >= 0 ? bmin[j] : bmax[j], cmax[j] the other one; passes iff s(cmin) < 0 && s(cmax) >= 0
DRT_DEV bool section_cull_passes(const SectionPlane &p, f3 bmin, f3 bmax) {
    const bool px = p.n.x >= 0.f, py = p.n.y >= 0.f, pz = p.n.z >= 0.f;
    const f3 cmin = mk3(px ? bmin.x : bmax.x, py ? bmin.y : bmax.y, pz ? bmin.z : bmax.z);
    const f3 cmax = mk3(px ? bmax.x : bmin.x, py ? bmax.y : bmin.y, pz ? bmax.z : bmin.z);
    return section_signed(p, cmin) < 0.f && section_signed(p, cmax) >= 0.f;
}

// drt.h "segment", cut(a, b) with lo the below one and hi the above one: t = s_lo / (s_lo - s_hi), lo + (hi - lo) * t per component
DRT_DEV f3 section_cut(f3 lo, float s_lo, f3 hi, float s_hi) {
    const float t = s_lo / (s_lo - s_hi);
    return mk3(lo.x + (hi.x - lo.x) * t, lo.y + (hi.y - lo.y) * t, lo.z + (hi.z - lo.z) * t);
}

// c ? a : b per component (selects on registers: a ternary on the whole struct goes through memory)
DRT_DEV f3 section_pick(bool c, f3 a, f3 b) { return mk3(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z); }

// drt.h "triangle test": the classes of the three vertices of the stored (v0, e1, e2); cut iff they are not all the same
struct SectionTri { f3 v0, v1, v2; float s0, s1, s2; bool cut; };
DRT_DEV SectionTri section_test(const SectionPlane &p, f3 v0, f3 e1, f3 e2) {
    SectionTri t;
    t.v0 = v0; t.v1 = v0 + e1; t.v2 = v0 + e2;
    t.s0 = section_signed(p, t.v0); t.s1 = section_signed(p, t.v1); t.s2 = section_signed(p, t.v2);
    const bool a0 = t.s0 >= 0.f, a1 = t.s1 >= 0.f, a2 = t.s2 >= 0.f;
    t.cut = a0 != a1 || a1 != a2;
    return t;
}

// drt.h "segment" and "record" of a cut triangle: the apex k is the vertex alone in its class, P = cut(k, k+1), Q = cut(k, k+2);
// apex above: P -> Q, apex below: Q -> P; code = k + 4 * (apex above).  The record is two 16-byte words: (p, prim), (q, code).
DRT_DEV void section_record(const SectionTri &t, int prim, float4 &w0, float4 &w1) {
    const bool a0 = t.s0 >= 0.f, a1 = t.s1 >= 0.f, a2 = t.s2 >= 0.f;
    const int k = a1 == a2 ? 0 : (a0 == a2 ? 1 : 2);
    const bool k0 = k == 0, k1 = k == 1;
    const f3 vk = section_pick(k0, t.v0, section_pick(k1, t.v1, t.v2)), va = section_pick(k0, t.v1, section_pick(k1, t.v2, t.v0)),
             vb = section_pick(k0, t.v2, section_pick(k1, t.v0, t.v1));
    const float sk = k0 ? t.s0 : (k1 ? t.s1 : t.s2), sa = k0 ? t.s1 : (k1 ? t.s2 : t.s0), sb = k0 ? t.s2 : (k1 ? t.s0 : t.s1);
    const bool above = sk >= 0.f;
    // lo is the below one of the two and hi the above one: the apex is hi when it is above
    const f3 P = section_cut(section_pick(above, va, vk), above ? sa : sk, section_pick(above, vk, va), above ? sk : sa);
    const f3 Q = section_cut(section_pick(above, vb, vk), above ? sb : sk, section_pick(above, vk, vb), above ? sk : sb);
    const f3 from = section_pick(above, P, Q), to = section_pick(above, Q, P);
    w0 = make_float4(from.x, from.y, from.z, __int_as_float(prim));
    w1 = make_float4(to.x, to.y, to.z, __int_as_float(k + (above ? 4 : 0)));
}
#endif

}  // namespace drt
