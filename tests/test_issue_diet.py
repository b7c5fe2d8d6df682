"""The slab test of the closest-hit traversal (csrc/device_math.hpp slab_entry_or_inf) against the same test without the
`texit < 0` compare that its clamp implies -- the form of tools/experiments/r13/issue_diet_all_items.patch, measured and not
shipped ("the issue diet") -- on the host: both are restated here in C++ with the device's semantics (fminf / fmaxf
drop a NaN operand as v_min_f32 / v_max_f32 do; one rounding per operation) and run over every combination of special and
ordinary per-axis slab distances.  Every use the traversal makes of the value comes out the same: `d < hit_t` for every hit_t a
path can have, and the order `d1 > d2` of two boxes wherever both are accepted.  The grid shows more: the two forms never differ
at all.  The entry distance is NaN only when every axis' pair of distances is NaN, and then so is the exit distance, whose
`< 0` is false -- the one case in which the dropped compare could have decided does not exist."""
import subprocess

PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cfloat>
#include <set>
#include <utility>

static unsigned bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }

// device_math.hpp slab_entry_or_inf from the per-axis distances on (t0 = (bmin - orig) * inv_dir, t1 = (bmax - orig) * inv_dir)
template <bool FULL_TEST>
static float slab(const float t0[3], const float t1[3]) {
    const float tmin[3] = { fminf(t0[0], t1[0]), fminf(t0[1], t1[1]), fminf(t0[2], t1[2]) };
    const float tmax[3] = { fmaxf(t1[0], t0[0]), fmaxf(t1[1], t0[1]), fmaxf(t1[2], t0[2]) };
    float tenter = fmaxf(fmaxf(tmin[0], tmin[1]), tmin[2]);
    const float texit = fminf(fminf(tmax[0], tmax[1]), tmax[2]);
    if (tenter < 0.0f) tenter = 0.0f;
    if (FULL_TEST) return (tenter > texit || texit < 0) ? INFINITY : tenter;
    return tenter > texit ? INFINITY : tenter;
}

int main() {
    unsigned one = 1u, dmax = 0x007FFFFFu;
    float denorm, denorm_max;
    std::memcpy(&denorm, &one, 4); std::memcpy(&denorm_max, &dmax, 4);
    const float v[] = { 0.0f, -0.0f, INFINITY, -INFINITY, NAN, denorm, -denorm, denorm_max, 1.0f, -1.0f, 0.5f, 3.0f, -2.0f, FLT_MAX, -FLT_MAX, 1e30f };
    const int n = sizeof v / sizeof v[0];
    const float hit_ts[] = { FLT_MAX, 1e30f, 3.0f, 1.0f, 0.75f, denorm, 1e-6f };
    unsigned long long cases = 0, bad = 0, differ = 0;
    std::set<std::pair<unsigned, unsigned>> outcomes;          // {full test, short test}, as bits
    int i[6];
    for (i[0] = 0; i[0] < n; i[0]++) for (i[1] = 0; i[1] < n; i[1]++) for (i[2] = 0; i[2] < n; i[2]++)
    for (i[3] = 0; i[3] < n; i[3]++) for (i[4] = 0; i[4] < n; i[4]++) for (i[5] = 0; i[5] < n; i[5]++) {
        const float t0[3] = { v[i[0]], v[i[1]], v[i[2]] }, t1[3] = { v[i[3]], v[i[4]], v[i[5]] };
        const float a = slab<true>(t0, t1), b = slab<false>(t0, t1);
        cases++;
        for (float h : hit_ts) if ((a < h) != (b < h)) bad++;            // the accepted set
        if (bits(a) != bits(b)) differ++;
        outcomes.insert({ bits(a), bits(b) });
    }
    // the order of two boxes, over every pair of outcomes: wherever both boxes are accepted by some hit_t, `d1 > d2` agrees
    unsigned long long pairs = 0;
    for (auto p : outcomes) for (auto q : outcomes) {
        float a1, b1, a2, b2;
        std::memcpy(&a1, &p.first, 4); std::memcpy(&b1, &p.second, 4); std::memcpy(&a2, &q.first, 4); std::memcpy(&b2, &q.second, 4);
        for (float h : hit_ts) {
            if (!(a1 < h && a2 < h)) continue;
            pairs++;
            if (!(b1 < h && b2 < h) || (a1 > a2) != (b1 > b2)) bad++;
        }
    }
    std::printf("%llu %llu %llu %llu %zu\n", cases, bad, differ, pairs, outcomes.size());
    return 0;
}
"""


def test_slab_entry_without_the_implied_compare(tmp_path):
    src = tmp_path / "slab.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "slab"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", str(src), "-o", str(exe)], check=True)
    cases, bad, differ, pairs, outcomes = (int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=300).stdout.split())
    assert cases == 16 ** 6 and bad == 0, (cases, bad)
    assert differ == 0         # (a NaN entry with an exit behind the origin would differ, +inf against NaN: min / max never produce it)
    assert pairs > 100 and outcomes >= 8, (pairs, outcomes)
