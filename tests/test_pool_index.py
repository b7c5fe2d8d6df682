"""csrc/pool_index.hpp compiled on its own, without a device: the bound on a ray's direction under which a T step's
determinant stays inside the fast range of the reciprocal.  What the kernel makes of it: tests/test_gpu_issue_diet.py."""
import os
import subprocess

from tests.scenes import ROOT

PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include "pool_index.hpp"
using namespace drt;

static float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

int main() {
    std::mt19937 rng(20261020u);
    // the guard bound: 8 * D * E^2 <= 2^99 with the product evaluated in double, for D = pool_safe_dir(E); D is the LARGEST
    // such float up to the evaluation's own rounding (the next float up must exceed 2^99 * (1 - 2^-40)); 0 for a non-finite E
    unsigned long long g_cases = 0, g_bad = 0;
    const double two99 = std::ldexp(1.0, 99);
    auto guard = [&](float e) {
        const float d = pool_safe_dir(e);
        g_cases++;
        if (!(e <= 3.402823466e+38f)) { if (d != 0.0f) g_bad++; return; }
        if (!(d >= 0.0f) || !std::isfinite(d)) { g_bad++; return; }
        if (8.0 * (double)d * (double)e * (double)e > two99) g_bad++;
        if (d < 3.402823466e+38f && d > 0.0f) {
            const float up = std::nextafterf(d, INFINITY);
            if (!(8.0 * (double)up * (double)e * (double)e > two99 * (1.0 - std::ldexp(1.0, -40)))) g_bad++;
        }
    };
    const float extremes[] = { 0.0f, -0.0f, from_bits(1u), from_bits(0x007FFFFFu), from_bits(0x00800000u), 1e-30f, 0x1p-64f, 1.0f, 3.0f, 0x1p30f, 0x1p48f, 0x1p49f,
                               0x1p50f, 0x1p52f, 0x1p60f, 0x1p63f, 0x1p64f, 1e30f, 3.402823466e+38f, INFINITY, NAN };
    for (float e : extremes) guard(e);
    for (int i = 0; i < 2000000; i++) guard(from_bits(rng() & 0x7FFFFFFFu));        // every exponent, NaNs and infinity included
    std::printf("%llu %llu\n", g_cases, g_bad);
    return 0;
}
"""


def test_guard_bound(tmp_path):
    src = tmp_path / "index.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "index"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "dustraytracer_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    g_cases, g_bad = (int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=120).stdout.split())
    assert g_cases > 2_000_000 and g_bad == 0, (g_cases, g_bad)
