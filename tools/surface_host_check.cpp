// surface_host_check.cpp -- the per-record routines of dustraytracer_amd/csrc/surface.hpp compiled, unchanged, for the host: a
// stand-alone program for tools/surface_host_check.py, which builds it with -fsanitize=address,undefined, feeds it a scene and
// references (hostile ones included) and compares what it writes with the numpy restatement.  Every array is allocated at its exact
// size, so a read outside the texel pool or any other array stops the program.
//   surface_host_check IN OUT
//   IN:  uint32 {n_tris, n_mats, n_texs, pool_bytes, n_refs, with_normals, n_samples, seed, first}, then TriHot[n_tris], TriCold[n_tris],
//        MatDev[n_mats], MatExt[n_mats], TexDev[n_texs], the pool, float[n_tris][9] (tree order), int32[n_tris], float[n_tris][9] (load
//        order), drt_hit[n_refs]
//   OUT: drt_surface[n_refs], uint64[n_tris], drt_hit[n_samples]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../dustraytracer_amd/csrc/surface.hpp"

using namespace drt;

template <class T>
static std::unique_ptr<T[]> read_array(std::FILE *f, size_t n) {
    std::unique_ptr<T[]> a(new T[n]);                     // exactly n: nothing to spare behind it
    if (n && std::fread(a.get(), sizeof(T), n, f) != n) { std::fprintf(stderr, "short input\n"); std::exit(2); }
    return a;
}

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    const auto head = read_array<uint32_t>(f, 9);
    const uint32_t n_tris = head[0], n_mats = head[1], n_texs = head[2], pool_bytes = head[3], n_refs = head[4], with_normals = head[5];
    const uint32_t n_samples = head[6], seed = head[7], first = head[8];
    const auto hot = read_array<TriHot>(f, n_tris);
    const auto cold = read_array<TriCold>(f, n_tris);
    const auto mats = read_array<MatDev>(f, n_mats);
    const auto ext = read_array<MatExt>(f, n_mats);
    const auto texs = read_array<TexDev>(f, n_texs);
    const auto pool = read_array<uint8_t>(f, pool_bytes);
    const auto own = read_array<float>(f, 9 * (size_t)n_tris);
    const auto order = read_array<int32_t>(f, n_tris);
    const auto normals = read_array<float>(f, 9 * (size_t)n_tris);
    const auto refs = read_array<SurfRef>(f, n_refs);
    std::fclose(f);

    SceneView sc = {};
    sc.tri_hot = hot.get(); sc.tri_cold = cold.get(); sc.mats = mats.get(); sc.mats_ext = ext.get(); sc.texs = texs.get(); sc.texels = pool.get();
    sc.n_tris = n_tris; sc.n_mats = n_mats; sc.n_texs = n_texs;
    SurfaceArgs a = {};
    a.own_normals = own.get(); a.load_index = order.get(); a.normals = with_normals ? normals.get() : nullptr;

    std::FILE *o = std::fopen(argv[2], "wb");
    if (!o) { std::perror(argv[2]); return 2; }
    for (uint32_t i = 0; i < n_refs; i++) {
        const SurfRecord rec = surface_lookup_one(sc, a, refs[i].prim, refs[i].u, refs[i].v);
        std::fwrite(&rec, sizeof rec, 1, o);
    }
    // the table, serially: amax, the exponent, the running sum
    std::unique_ptr<uint64_t[]> cdf(new uint64_t[n_tris]);
    uint32_t amax_bits = 0;
    for (uint32_t k = 0; k < n_tris; k++) amax_bits = std::max(amax_bits, surf_bits(surface_area2(hot[k])));
    uint64_t total = 0;
    for (uint32_t k = 0; k < n_tris; k++) {
        if (amax_bits) total += surface_weight(surface_area2(hot[k]), surface_exponent(amax_bits));
        cdf[k] = total;
    }
    std::fwrite(cdf.get(), sizeof(uint64_t), n_tris, o);
    for (uint32_t k = 0; k < n_samples; k++) {
        const SurfRef s = surface_sample_one(surf_pcg(seed), first + k, cdf.get(), n_tris);
        std::fwrite(&s, sizeof s, 1, o);
    }
    std::fclose(o);
    return 0;
}
