// ambient_host_check.cpp -- the tile arithmetic and the ray rule of dustraytracer_amd/csrc/ambient.hpp compiled, unchanged, for the
// host: a stand-alone program for tools/ambient_host_check.py, which builds it with -fsanitize=address,undefined and compares what it
// writes with the numpy restatement.
//   ambient_host_check tiles
//       walks the tiling of every S in 1 .. 4096 over several n (every lane of every tile for small n, the ends of the range for
//       n = 2^31 - 1 and 2^32 - 1): every (point, sample) pair exactly once, in range, the shards a partition of the tiles; prints
//       one line of totals.  Exit status 1 on a mismatch.
//   ambient_host_check rays IN OUT
//       IN:  uint32 {n, samples, seed, first}, then drt_ao_point[n]
//       OUT: per point and sample float {o[3], d[3]} and int32 bent terms [3]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../dustraytracer_amd/csrc/ambient.hpp"

using namespace drt;

static int fail(const char *what, uint32_t s, uint64_t n, uint64_t tile, uint32_t lane) {
    std::fprintf(stderr, "tiles: %s at S = %u, n = %llu, tile %llu, lane %u\n", what, s, (unsigned long long)n, (unsigned long long)tile, lane);
    return 1;
}

// every lane of tiles [t0, t1): marks seen[point * S + sample] where `seen` covers points [p0, p0 + points)
static int walk(const AoTiling &t, uint32_t n, uint64_t t0, uint64_t t1, std::vector<uint8_t> *seen, uint64_t p0, uint64_t &pairs) {
    for (uint64_t tile = t0; tile < t1; tile++)
        for (uint32_t lane = 0; lane < 64; lane++) {
            uint32_t point = 0, sample = 0;
            if (!ao_tile_lane(t, tile, lane, n, point, sample)) continue;
            if (point >= n || sample >= t.samples) return fail("out of range", t.samples, n, tile, lane);
            if ((lane & (t.seg - 1u)) == 0u && sample % 64u != 0u) return fail("a point's first lane is not its sample 0 (or 64 t)", t.samples, n, tile, lane);
            pairs++;
            if (seen) {
                if (point < p0 || (uint64_t)(point - p0) * t.samples + sample >= seen->size()) return fail("outside the window", t.samples, n, tile, lane);
                uint8_t &cell = (*seen)[(uint64_t)(point - p0) * t.samples + sample];
                if (cell) return fail("seen twice", t.samples, n, tile, lane);
                cell = 1;
            }
        }
    return 0;
}

static int check_tiles() {
    const uint32_t shards = 16;
    uint64_t tiles_walked = 0, pairs = 0;
    for (uint32_t s = 1; s <= kAoMaxSamples; s++) {
        const AoTiling t = ao_tiling(s);
        if (t.seg == 0 || (t.seg & (t.seg - 1u)) != 0 || t.seg > 64u || t.per_tile * t.seg > 64u) return fail("segment", s, 0, 0, 0);
        for (uint32_t n : { 1u, 3u, 5u, 63u, 64u, 65u, 257u }) {
            if (s > 130u && n > 5u) break;                    // (the tiling of S > 64 has one form: the long n only where the forms change)
            const uint64_t count = ao_tile_count(t, n);
            std::vector<uint8_t> seen((size_t)n * s, 0);
            uint64_t got = 0;
            if (walk(t, n, 0, count, &seen, 0, got)) return 1;
            if (got != (uint64_t)n * s) return fail("pairs missing", s, n, count, 0);
            // one more tile holds nothing
            uint64_t beyond = 0;
            if (walk(t, n, count, count + 1, nullptr, 0, beyond) || beyond) return fail("a tile beyond the count holds work", s, n, count, 0);
            tiles_walked += count; pairs += got;
        }
        // the ends of the range: 64-bit counts
        for (uint32_t n : { 0x7fffffffu, 0xffffffffu }) {
            const uint64_t count = ao_tile_count(t, n);
            const uint64_t want = t.per_tile > 1 ? ((uint64_t)n + t.per_tile - 1) / t.per_tile : (uint64_t)n * ((s + 63) / 64);
            if (count != want) return fail("count", s, n, count, 0);
            if (s == kAoMaxSamples && n == 0xffffffffu && count != ((uint64_t)1 << 38) - 64) return fail("count at the limit", s, n, count, 0);
            // the last tiles cover exactly the last points' samples
            const uint64_t last_tiles = t.per_point > 1 ? 2 * (uint64_t)t.per_point : 2;
            const uint64_t t0 = count - last_tiles;
            uint32_t p_first = 0, dummy = 0;
            if (!ao_tile_lane(t, t0, 0, n, p_first, dummy)) return fail("first lane of a tile idle", s, n, t0, 0);
            std::vector<uint8_t> seen((size_t)((uint64_t)n - p_first) * s, 0);
            uint64_t got = 0;
            if (walk(t, n, t0, count, &seen, p_first, got)) return 1;
            if (got != ((uint64_t)n - p_first) * s) return fail("pairs missing at the end", s, n, count, 0);
            uint64_t beyond = 0;
            if (walk(t, n, count, count + 2, nullptr, 0, beyond) || beyond) return fail("a tile beyond the count holds work", s, n, count, 0);
            // the shards partition [0, count)
            uint64_t at = 0;
            for (uint32_t k = 0; k < shards; k++) {
                if (ao_shard_begin(count, k, shards) != at) return fail("shards", s, n, k, 0);
                const uint64_t next = ao_shard_begin(count, k + 1, shards);
                if (next < at) return fail("shards", s, n, k, 0);
                at = next;
            }
            if (at != count) return fail("shards", s, n, shards, 0);
            tiles_walked += last_tiles; pairs += got;
        }
    }
    std::printf("tiles: S = 1 .. %u over n = 1, 3, 5 (63, 64, 65, 257 up to S = 130) and the ends of n = 2^31 - 1, 2^32 - 1: %llu tiles walked, %llu pairs, each once\n", kAoMaxSamples,
                (unsigned long long)tiles_walked, (unsigned long long)pairs);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "tiles")) return check_tiles();
    if (argc != 4 || std::strcmp(argv[1], "rays")) { std::fprintf(stderr, "usage: %s tiles | rays IN OUT\n", argv[0]); return 2; }
    std::FILE *f = std::fopen(argv[2], "rb");
    if (!f) { std::perror(argv[2]); return 2; }
    uint32_t head[4];
    if (std::fread(head, 4, 4, f) != 4) { std::fprintf(stderr, "short input\n"); return 2; }
    const uint32_t n = head[0], samples = head[1], seed = head[2], first = head[3];
    std::unique_ptr<AoPoint[]> pts(new AoPoint[n]);           // exactly n: nothing to spare behind it
    if (n && std::fread(pts.get(), sizeof(AoPoint), n, f) != n) { std::fprintf(stderr, "short input\n"); return 2; }
    std::fclose(f);
    std::FILE *o = std::fopen(argv[3], "wb");
    if (!o) { std::perror(argv[3]); return 2; }
    const uint32_t seed_hash = ao_pcg(seed);
    // in the tiles' order, through the tile arithmetic: every pair is written to its own place
    const AoTiling t = ao_tiling(samples);
    const uint64_t count = ao_tile_count(t, n);
    struct Rec { float o[3], d[3]; int32_t term[3]; };
    std::unique_ptr<Rec[]> recs(new Rec[(size_t)n * samples]);
    for (uint64_t tile = 0; tile < count; tile++)
        for (uint32_t lane = 0; lane < 64; lane++) {
            uint32_t point = 0, sample = 0;
            if (!ao_tile_lane(t, tile, lane, n, point, sample)) continue;
            Rec &r = recs[(size_t)point * samples + sample];
            ao_ray(pts[point], seed_hash, first + point, sample, r.o, r.d);
            for (int k = 0; k < 3; k++) r.term[k] = ao_live(pts[point].max_dist) ? ao_bent_term(r.d[k]) : -1;
        }
    std::fwrite(recs.get(), sizeof(Rec), (size_t)n * samples, o);
    std::fclose(o);
    return 0;
}
