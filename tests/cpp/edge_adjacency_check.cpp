// edge_adjacency_check.cpp -- a stand-alone run of csrc/edge_adjacency.hpp, the routine behind drt_scene_edge_adjacency and
// drt_tri_edge_adjacency, over heap buffers of exactly the size it may read: tight [n][3][3] positions, the 48-byte drt_tri layout and
// the 128-byte drt_triangle layout (positions at byte 16, 32 bytes apart).  It needs nothing of the library, so it can be built with a
// sanitizer as it stands:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/edge_adjacency_check.cpp -o check && ./check
// tests/test_curve_abi.py builds it plainly and runs it.  Prints "ok <tables checked>" and returns 0, or says what differs and returns 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../dustraytracer_amd/csrc/edge_adjacency.hpp"

namespace {

using Mesh = std::vector<float>;      // 9 floats per triangle

int checked = 0;

// the table of `mesh` through the three layouts; they must agree
std::vector<int32_t> table(const Mesh &mesh) {
    const size_t n = mesh.size() / 9;
    std::unique_ptr<float[]> tight(new float[9 * n + (n ? 0 : 1)]);
    if (n) std::memcpy(tight.get(), mesh.data(), 36 * n);
    const std::vector<int32_t> a = drt::edge_adjacency_of(n ? tight.get() : nullptr, 36, 12, n);
    // drt_tri: v[3][3] + three pad words; the last record ends with its ninth float, so a read of the pad is out of bounds
    const size_t tri_bytes = n ? 48 * (n - 1) + 36 : 0;
    std::unique_ptr<unsigned char[]> tris(new unsigned char[tri_bytes + 1]);
    for (size_t t = 0; t < n; t++) std::memcpy(tris.get() + 48 * t, mesh.data() + 9 * t, 36);
    const std::vector<int32_t> b = drt::edge_adjacency_of(tris.get(), 48, 12, n);
    // drt_triangle: vertex e's position at 16 + 32 e; the buffer ends with the last position read
    const size_t big_bytes = n ? 128 * (n - 1) + 16 + 64 + 12 : 0;
    std::unique_ptr<unsigned char[]> big(new unsigned char[big_bytes + 1]);
    std::memset(big.get(), 0xff, big_bytes + 1);
    for (size_t t = 0; t < n; t++)
        for (int e = 0; e < 3; e++) std::memcpy(big.get() + 128 * t + 16 + 32 * e, mesh.data() + 9 * t + 3 * e, 12);
    const std::vector<int32_t> c = drt::edge_adjacency_of(big.get() + 16, 128, 32, n);
    if (a != b || a != c || a.size() != 3 * n) { std::printf("the layouts disagree on %zu triangles\n", n); std::exit(1); }
    checked++;
    return a;
}

void expect(const char *what, const Mesh &mesh, const std::vector<int32_t> &want) {
    const std::vector<int32_t> got = table(mesh);
    if (got != want) {
        std::printf("%s:", what);
        for (int32_t v : got) std::printf(" %d", v);
        std::printf("\n");
        std::exit(1);
    }
}

void add(Mesh &m, const float *a, const float *b, const float *c) {
    m.insert(m.end(), a, a + 3); m.insert(m.end(), b, b + 3); m.insert(m.end(), c, c + 3);
}

}  // namespace

int main() {
    const float p[4][3] = { { 0, 0, 0 }, { 1, 0, 0 }, { 1, 1, 0 }, { 0, 1, 0 } };
    const float up[3] = { 0, 0, 1 }, down[3] = { 0, 0, -1 }, minus_zero[3] = { -0.0f, 0, 0 };
    expect("no triangles", Mesh(), {});
    Mesh one; add(one, p[0], p[1], p[2]);
    expect("one triangle", one, { -1, -1, -1 });
    Mesh quad; add(quad, p[0], p[1], p[2]); add(quad, p[0], p[2], p[3]);
    expect("quad", quad, { -1, -1, 3, 2, -1, -1 });
    Mesh flipped; add(flipped, p[0], p[1], p[2]); add(flipped, p[0], p[3], p[2]);          // the shared edge runs the same way twice
    expect("flipped quad", flipped, { -1, -1, -2, -1, -1, -2 });
    Mesh book; add(book, down, up, p[1]); add(book, down, up, p[3]); add(book, up, down, p[2]);
    expect("book", book, { -2, -1, -1, -2, -1, -1, -2, -1, -1 });
    Mesh needle; add(needle, p[0], p[0], p[1]);                                            // an edge whose two ends are the same position
    expect("zero-length edge", needle, { -2, 2, 1 });                                      // (its other two edges are each other's twins)
    Mesh signs; add(signs, p[0], p[1], p[2]); add(signs, minus_zero, p[2], p[3]);          // -0.0 is not +0.0: no twin
    expect("signed zero", signs, { -1, -1, -1, -1, -1, -1 });
    // a closed fan round an axis, 3 000 triangles in two caps: every half-edge has a twin and the table is an involution
    const int n = 1500;
    std::vector<float> rim(3 * n);
    for (int i = 0; i < n; i++) { rim[3 * i] = (float)(i % 50) - 25.f; rim[3 * i + 1] = (float)(i / 50) - 15.f; rim[3 * i + 2] = (float)((i * 7) % 13) * 0.125f; }
    // (distinct points, joined into a cycle i -> i + 1: the caps share every rim edge)
    Mesh closed;
    const float top[3] = { 0.5f, 0.5f, 40.f }, bottom[3] = { 0.5f, 0.5f, -40.f };
    for (int i = 0; i < n; i++) {
        const float *a = &rim[3 * i], *b = &rim[3 * ((i + 1) % n)];
        add(closed, top, a, b);
        add(closed, bottom, b, a);
    }
    const std::vector<int32_t> adj = table(closed);
    for (size_t h = 0; h < adj.size(); h++)
        if (adj[h] < 0 || (size_t)adj[h] >= adj.size() || adj[(size_t)adj[h]] != (int32_t)h || (size_t)adj[h] == h) {
            std::printf("closed fan: half-edge %zu has %d\n", h, adj[h]);
            return 1;
        }
    std::printf("ok %d\n", checked);
    return 0;
}
