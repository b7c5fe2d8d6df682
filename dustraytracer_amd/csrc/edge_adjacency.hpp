// edge_adjacency.hpp -- the edge adjacency of a triangle list by bit-equal positions (include/drt.h drt_scene_edge_adjacency and
// drt_tri_edge_adjacency): one routine over positions in memory, whatever record they sit in.  Header-only and free of the rest of the
// library, so that a stand-alone program can run it under a sanitizer (tests/cpp/edge_adjacency_check.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace drt {

// Half-edge h = 3 t + e runs from vertex e to vertex (e + 1) % 3 of triangle t.  The half-edges are sorted by their unordered pair
// of endpoint positions (the three words of each, compared as integers); a group of two that run in opposite directions is a pair
// of twins, a group of one a boundary edge (-1), everything else -2 -- three or more, two the same way, both ends the same position.
// Vertex e of triangle t is the three floats at first + t * tri_stride + e * vertex_stride (strides in bytes).
inline std::vector<int32_t> edge_adjacency_of(const void *first, size_t tri_stride, size_t vertex_stride, size_t n) {
    struct HalfEdge { uint32_t lo[3], hi[3]; int32_t h; bool forward; };      // forward: it runs from lo to hi
    const unsigned char *base = static_cast<const unsigned char *>(first);
    std::vector<int32_t> adj(3 * n, -2);
    std::vector<HalfEdge> edges;
    edges.reserve(3 * n);
    for (size_t t = 0; t < n; t++)
        for (int e = 0; e < 3; e++) {
            uint32_t a[3], b[3];
            std::memcpy(a, base + t * tri_stride + (size_t)e * vertex_stride, 12);
            std::memcpy(b, base + t * tri_stride + (size_t)((e + 1) % 3) * vertex_stride, 12);
            const int c = std::memcmp(a, b, 12) == 0 ? 0 : (std::lexicographical_compare(a, a + 3, b, b + 3) ? -1 : 1);
            if (c == 0) continue;                                          // both ends the same position: -2
            HalfEdge he;
            std::memcpy(he.lo, c < 0 ? a : b, 12);
            std::memcpy(he.hi, c < 0 ? b : a, 12);
            he.h = (int32_t)(3 * t + e);
            he.forward = c < 0;
            edges.push_back(he);
        }
    auto key_less = [](const HalfEdge &x, const HalfEdge &y) {
        for (int k = 0; k < 3; k++)
            if (x.lo[k] != y.lo[k]) return x.lo[k] < y.lo[k];
        for (int k = 0; k < 3; k++)
            if (x.hi[k] != y.hi[k]) return x.hi[k] < y.hi[k];
        return false;
    };
    std::sort(edges.begin(), edges.end(), key_less);
    for (size_t i = 0; i < edges.size();) {
        size_t j = i + 1;
        while (j < edges.size() && !key_less(edges[i], edges[j])) j++;
        if (j - i == 1) adj[(size_t)edges[i].h] = -1;
        else if (j - i == 2 && edges[i].forward != edges[i + 1].forward) {
            adj[(size_t)edges[i].h] = edges[i + 1].h;
            adj[(size_t)edges[i + 1].h] = edges[i].h;
        }
        i = j;
    }
    return adj;
}

}  // namespace drt
