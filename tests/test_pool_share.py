"""The grid of a path_pool launch that shares the device (csrc/pool_share.hpp), compiled on its own without a device: a launch is
given 1 / min(hint, launches that can run side by side) of the workgroup slots -- never more than it wants, never less than one
workgroup -- and the launches that reliably run side by side are the hint while it is below the runtime's hardware queue count, else
half the queues.  What the launcher makes of it on the device: tests/test_gpu_pool_share.py."""
import os
import subprocess

from tests.scenes import ROOT

PROGRAM = r"""
#include <cstdio>
#include "pool_share.hpp"
using namespace drt;

// the rule at compile time, on the figures of the metric workload: 512 slots, a launch that wants them all
static_assert(pool_shared_grid(512, 512, 4, 2) == 256, "four in flight, two run side by side: half each");
static_assert(pool_shared_grid(512, 512, 4, 3) == 171, "a third, rounded up");
static_assert(pool_shared_grid(512, 512, 4, 4) == 128, "four in flight, four run side by side: a quarter each, as before");
static_assert(pool_shared_grid(512, 512, 1, 3) == 512 && pool_shared_grid(512, 512, 4, 1) == 512, "nothing to share with");
// launches that run side by side: the hint below the queue count, half the queues from there on; no queue count = the runtime's 4
static_assert(pool_share_max(1, 4) == 1 && pool_share_max(2, 4) == 2 && pool_share_max(3, 4) == 3 && pool_share_max(4, 4) == 2 && pool_share_max(64, 4) == 2, "");
static_assert(pool_share_max(4, 8) == 4 && pool_share_max(7, 8) == 7 && pool_share_max(8, 8) == 4 && pool_share_max(64, 8) == 4, "");
static_assert(pool_share_max(4, 0) == 2 && pool_share_max(3, -5) == 3 && pool_share_max(0, 4) == 1 && pool_share_max(-3, 8) == 1, "");
static_assert(pool_share_max(1, 1) == 1 && pool_share_max(5, 1) == 1 && pool_share_max(2, 2) == 1 && pool_share_max(9, 3) == 1 && pool_share_max(40, 32) == 16, "");

int main() {
    // every hint and cap on small and odd slot counts: the grid is min(want, ceil(slots / min(hint, cap))), at least 1
    unsigned long long bad = 0, cases = 0;
    const unsigned long long slot_counts[] = { 1, 2, 3, 8, 511, 512 };
    for (unsigned long long slots : slot_counts)
        for (unsigned long long want = 0; want <= slots + 1; want += (slots > 8 ? 73 : 1))
            for (int hint = -1; hint <= 66; hint++)
                for (int cap = -1; cap <= 9; cap++) {
                    const unsigned long long h = hint < 1 ? 1 : hint, c = cap < 1 ? 1 : cap, n = h < c ? h : c;
                    unsigned long long expect = (slots + n - 1) / n;
                    if (want < expect) expect = want;
                    if (expect < 1) expect = 1;
                    const unsigned long long got = pool_shared_grid(want, slots, hint, cap);
                    cases++;
                    if (got != expect) bad++;
                    // the shares of the launches that can run cover the device
                    if (want >= slots && got * n < slots) bad++;
                }
    // the cap never exceeds the hint, never the queues below the null stream's, and is at least one
    for (int hint = -2; hint <= 70; hint++)
        for (int q = -2; q <= 40; q++) {
            const int h = hint < 1 ? 1 : hint, qq = q < 1 ? 4 : q, got = pool_share_max(hint, q);
            cases++;
            if (got < 1 || got > h || (qq > 1 && got > qq - 1) || got != (h < qq ? h : (qq > 1 ? qq / 2 : 1))) bad++;
        }
    std::printf("%llu %llu\n", cases, bad);
    return 0;
}
"""


def test_the_share_is_cut_by_what_can_run(tmp_path):
    src = tmp_path / "share.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "share"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "dustraytracer_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    cases, bad = subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()
    assert int(cases) > 10000 and int(bad) == 0, (cases, bad)
