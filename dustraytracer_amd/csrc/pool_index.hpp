// pool_index.hpp -- a launch constant that takes per-triangle work off path_pool's vector ALU (kernel_path_pool.hip, the T step):
// the largest ray-direction component for which a triangle test's determinant cannot leave the fast range of the reciprocal.
// No device or HIP dependency: it compiles on its own (tests/test_pool_index.py).
#pragma once
#include <cstdint>

namespace drt {

// Triangle test (Intersection.cu:4-36): det = e1 . (dir x e2), three products of an edge component with a difference of two
// products of a direction component with an edge component.  With D >= every |dir component| and E >= every |edge component|,
// exact arithmetic bounds |det| by 3 * E * (2 * D * E) = 6 * D * E^2.  In fp32 every path from an input to det passes five
// roundings (dir * e2, the difference, * e1, two sums), each of which grows a bound by at most 1 + 2^-24, and every
// intermediate is bounded by the same expression, so |det| <= 6 * D * E^2 * (1 + 2^-24)^5 < 8 * D * E^2: the factor 8 in
// place of 6 pays for the rounding (and makes the bound a power of two times D * E^2).
// pool_safe_dir(E) is the largest float D with 8 * D * E^2 <= 2^99, rounded down: a lane whose ray has no direction component
// above it has |det| <= 2^99 for every staged triangle -- below the 2^100 at which the refined v_rcp_f32 stops being the
// correctly rounded quotient (device_math.hpp exact_rcp) -- and nothing on the way overflowed.  0 when E is not finite
// (no lane is safe: 0 < |component| for every ray with a direction, and NaN compares false); FLT_MAX for E == 0.
inline float pool_safe_dir(float max_edge) {
    const float flt_max = 3.402823466e+38f;
    if (!(max_edge <= flt_max)) return 0.0f;                    // inf, NaN
    const double e = (double)max_edge;
    if (e == 0.0) return flt_max;
    const double two99 = 633825300114114700748351602688.0;      // 2^99
    const double d = two99 / (8.0 * e * e);                     // (E^2 <= 2^256: finite in double; the quotient may round up)
    if (d >= (double)flt_max) return flt_max;
    float f = (float)d;                                         // round to nearest: may be above d, and d above the true quotient
    // step down until the inequality holds with the product evaluated in double (8 * f * e^2: f * e is exact to 2^-53, the
    // comparison below is the definition the kernel relies on, with 2^99 * (1 - 2^-50) as the double evaluation's own margin)
    const double limit = two99 * (1.0 - 0x1p-50);
    for (int k = 0; k < 4 && f > 0.0f && 8.0 * (double)f * e * e > limit; k++) {
        uint32_t u;
        __builtin_memcpy(&u, &f, 4);
        u -= 1u;
        __builtin_memcpy(&f, &u, 4);
    }
    if (8.0 * (double)f * e * e > limit) return 0.0f;
    return f;
}

}  // namespace drt
