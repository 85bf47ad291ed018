// decode_math.h -- the scalar arithmetic of the tag decode (reference src/detector.rs:42-122, src/image_util.rs:39-70), one
// definition each for the host tail (host_tail.cpp) and the decode kernels (tail_kernels.hip, decode_stages.hip): f32::round,
// Rust's `as u32`, the project's finite test and tag_affine.  Every file that includes it is compiled with -ffp-contract=off.
// The lane-group code built on these (sampler, rotation, code scan, tag store) is decode_lanes.h, device only.
#pragma once
#include <cstdint>

#include "libm_f32.h"

namespace agx {

// f32::round (half away from zero) without the call into libm the baseline x86-64 target makes of std::round (no SSE4.1
// rounding instruction): x - trunc(x) is exact in binary32, so the comparison with 0.5 decides exactly what roundf decides.
// Values of magnitude >= 2^23 (and NaN / inf) are their own rounding.  (The sign of a zero result may differ from roundf's --
// every use converts the result to an integer.  Compared with roundf on all 2^32 bit patterns: equal.)
AGX_HD float round_half_away(float x)
{
    if (!(__builtin_fabsf(x) < 8388608.0f)) return x;
    float t = (float)(int32_t)x;
    const float d = x - t;
    if (d >= 0.5f) t += 1.0f;
    else if (d <= -0.5f) t -= 1.0f;
    return t;
}
AGX_HD uint32_t f32_as_u32(float v)  // Rust `as u32`: saturating, NaN -> 0
{
    if (!(v > 0.0f)) return 0u;
    if (v >= 4294967296.0f) return 0xffffffffu;
    return (uint32_t)v;
}
// neither NaN nor an infinity.  A corner or a sample coordinate that is not finite is AGX_QUAD_OUTSIDE: the project's rule
AGX_HD bool f32_finite(float v) { return (f32_bits(v) & 0x7f800000u) != 0x7f800000u; }

// image_util.rs:39-70 (h = 2x3 affine, row-major): the least-squares affine map from the tag's corner grid (-m,-m), (-m,S), (S,S),
// (S,-m) to the image quad.  The source points are the corners of an axis-aligned square, so the normal equations diagonalise
// about its centre.  Evaluated in binary64, rounded once.
AGX_HD void tag_affine(const float quad_xy[8], int side_bits, float margin, float h[6])
{
    const double S = (double)((float)side_bits - 1.0f + margin), m = (double)margin;
    const double c = 0.5 * (S - m), a = 0.5 * (S + m);
    const double su[4] = {-a, -a, a, a}, sv[4] = {-a, a, a, -a};
    for (int axis = 0; axis < 2; ++axis) {
        double gu = 0, gv = 0, mean = 0;
        for (int p = 0; p < 4; ++p) {
            const double t = quad_xy[2 * p + axis];
            gu += su[p] * t;
            gv += sv[p] * t;
            mean += t;
        }
        const double hu = gu / (4.0 * a * a), hv = gv / (4.0 * a * a);
        h[3 * axis + 0] = (float)hu;
        h[3 * axis + 1] = (float)hv;
        h[3 * axis + 2] = (float)(mean / 4.0 - hu * c - hv * c);
    }
}

}  // namespace agx
