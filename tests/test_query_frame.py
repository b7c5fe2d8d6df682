"""csrc/query_frame.hpp's host side compiled on its own, without a device: the split of n queries into the claim's shards, the
distance between their head counters, and the size of a launch.  What the kernels make of them: every tests/test_gpu_*.py of a
batched query, and tests/test_gpu_query_refill.py for the claim at other refill thresholds."""
import os
import subprocess

from tests.scenes import ROOT

PROGRAM = r"""
#include <cstdio>
#include "query_frame.hpp"
using namespace drt;

static_assert(shard_range(17u, 3u).begin == 3u && shard_range(17u, 3u).len == 1u, "shard_range is a constant expression");

int main() {
    const uint32_t sizes[] = { 0u, 1u, 15u, 16u, 17u, 255u, 256u, 257u, 0x7fffffffu };
    const int cus[] = { 0, 1, 256 };
    unsigned long long cases = 0, bad = 0;
    // the heads: kRqShards of them, a whole 128-byte line apart, inside the kRqHeadWords the renderer zeroes
    cases++;
    if (kRqShards != 16 || kRqShardStride * sizeof(unsigned int) != 128 || kRqHeadWords != kRqShards * kRqShardStride) bad++;
    for (uint32_t n : sizes) {
        // the 16 ranges are contiguous and disjoint, cover [0, n) exactly, and none is longer than n
        uint64_t next = 0;
        for (uint32_t s = 0; s < (uint32_t)kRqShards; s++) {
            const ShardRange r = shard_range(n, s);
            cases++;
            if (r.begin != next || r.len > n) bad++;
            next = (uint64_t)r.begin + r.len;
        }
        cases++;
        if (next != n) bad++;
        // query_blocks(n, cus) = min(ceil(n / 256), 8 * max(1, cus)), ray_query_max_blocks' max(1, num_cus)
        for (int c : cus) {
            const uint64_t ceil_n = ((uint64_t)n + 255u) / 256u, grid = 8ull * (uint64_t)(c < 1 ? 1 : c);
            cases++;
            if (query_blocks(n, c) != (ceil_n < grid ? ceil_n : grid) || grid != (uint64_t)ray_query_max_blocks(c)) bad++;
            // a kernel compiled for fewer waves per SIMD launches that many workgroups per CU, never more than the 8
            cases++;
            if (query_blocks(n, c, 5) != (ceil_n < grid * 5 / 8 ? ceil_n : grid * 5 / 8) || query_blocks(n, c, 9) != query_blocks(n, c)) bad++;
        }
    }
    std::printf("%llu %llu\n", cases, bad);
    return 0;
}
"""


def test_shard_ranges_stride_and_block_count(tmp_path):
    src = tmp_path / "frame.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "frame"
    # (the header includes the HIP runtime's declarations: a plain C++ compiler reads them with the platform macro set)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I" + os.path.join(ROOT, "dustraytracer_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    cases, bad = (int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split())
    assert cases == 1 + 9 * (16 + 1 + 3 * 2) and bad == 0, (cases, bad)
