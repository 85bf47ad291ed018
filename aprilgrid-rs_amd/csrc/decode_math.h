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

AGX_HD bool f64_finite(double v)
{
    uint64_t u;
    memcpy(&u, &v, 8);
    return (u & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// image_util.rs:5-37 (h = 3x3, row-major): THE projective map from tag_affine's source square (-m,-m), (-m,S), (S,S), (S,-m) to
// the image quad.  The reference stacks the four correspondences into an 8 x 9 matrix and takes the SVD's last right-singular
// vector; with four points that matrix has a one-dimensional null space, so the vector is this map up to scale -- and the map
// through four points has a closed form: the unit square (0,0), (1,0), (1,1), (0,1) onto the quad,
//   X = (a u + b v + x0) / (g u + k v + 1),  Y = (d u + e v + y0) / (g u + k v + 1)
// with g, k the two quotients below, composed with the source square's normalisation u = (y + m) / L, v = (x + m) / L,
// L = S + m.  Binary64 with + - * / only (no sqrt, no libm, no iteration: host and device give the same bytes), rounded once.
// Scale: w = h6 c + h7 c + h8 at the square's centre c is 1 (the reference's unit norm with the SVD's arbitrary sign says
// nothing to a consumer); an exact parallelogram has g = k = 0 and the last row 0, 0, 1 -- tag_affine's shape.
// false, and h untouched: the closed form's denominator is zero or not finite; the centre's w is zero or not finite before
// scaling; or, after scaling, w at one of the four source corners is not > 0 -- a quad that is not strictly convex, or whose
// horizon crosses the tag.  (The corner values are those of the closed form itself: in the unit square's coordinates the
// denominator is 1, 1 + g, 1 + g + k, 1 + k at the corners and 1 + (g + k) / 2 at the centre.)
AGX_HD bool tag_homography(const float quad_xy[8], int side_bits, float margin, float h[9])
{
    const double S = (double)((float)side_bits - 1.0f + margin), m = (double)margin, L = S + m;
    const double x0 = quad_xy[0], y0 = quad_xy[1], x1 = quad_xy[2], y1 = quad_xy[3], x2 = quad_xy[4], y2 = quad_xy[5], x3 = quad_xy[6], y3 = quad_xy[7];
    const double dx1 = x1 - x2, dx2 = x3 - x2, sx = x0 - x1 + x2 - x3;
    const double dy1 = y1 - y2, dy2 = y3 - y2, sy = y0 - y1 + y2 - y3;
    const double den = dx1 * dy2 - dx2 * dy1;
    if (!f64_finite(den) || den == 0.0) return false;
    const double g = (sx * dy2 - dx2 * sy) / den, k = (dx1 * sy - sx * dy1) / den;
    const double wc = L * (1.0 + 0.5 * (g + k));
    if (!f64_finite(wc) || wc == 0.0) return false;
    const double r = 1.0 / wc;
    const double w1 = L * (1.0 + g) * r, w2 = L * (1.0 + g + k) * r, w3 = L * (1.0 + k) * r;
    if (!(L * r > 0.0) || !(w1 > 0.0) || !(w2 > 0.0) || !(w3 > 0.0)) return false;
    const double a = x1 - x0 + g * x1, b = x3 - x0 + k * x3, d = y1 - y0 + g * y1, e = y3 - y0 + k * y3;
    // (rows times L: x' = b x + a y + (a + b) m + x0 L, ..., w' = k x + g y + (g + k) m + L); + 0.0: no negative zero is stored
    h[0] = (float)(b * r + 0.0);
    h[1] = (float)(a * r + 0.0);
    h[2] = (float)(((a + b) * m + x0 * L) * r + 0.0);
    h[3] = (float)(e * r + 0.0);
    h[4] = (float)(d * r + 0.0);
    h[5] = (float)(((d + e) * m + y0 * L) * r + 0.0);
    h[6] = (float)(k * r + 0.0);
    h[7] = (float)(g * r + 0.0);
    h[8] = (float)(((g + k) * m + L) * r + 0.0);
    return true;
}

// The samples of one slot under the homography: u, v and w each h0 x + h1 y + h2 1.0f left to right in binary32, the point
// (u / w, v / w) by correctly rounded binary32 division.  A w that is not > 0 or not finite ends the slot (AGX_QUAD_OUTSIDE).
AGX_HD bool homography_w_ok(float w) { return w > 0.0f && f32_finite(w); }
AGX_HD float homography_w(const float h[9], float fx, float fy) { return h[6] * fx + h[7] * fy + h[8] * 1.0f; }
AGX_HD void homography_point(const float h[9], float fx, float fy, float w, float &px, float &py)
{
    px = (h[0] * fx + h[1] * fy + h[2] * 1.0f) / w;
    py = (h[3] * fx + h[4] * fy + h[5] * 1.0f) / w;
}

}  // namespace agx
