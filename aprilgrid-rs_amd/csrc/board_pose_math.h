// board_pose_math.h -- the board's pose (R, t: board -> camera) through a frame's tag table under the pinhole + radial-tangential
// lens model, one definition each for the host form (host_tail.cpp: board_pose) and the kernel (board_pose.hip: k_board_pose).
// Binary64, + - * / and the square roots named below, no contraction (every file that includes it is compiled with
// -ffp-contract=off), so both forms give the same bytes.  The reference has no such function.
//
// Camera (OpenCV's model; Kalibr's pinhole-radtan with k3 = 0).  THE ORDER OF OPERATIONS, for a board point (X, Y, 0):
//   Xc = R0 X + R1 Y + t0,  Yc = R3 X + R4 Y + t1,  Zc = R6 X + R7 Y + t2      (left to right);  Zc not > 0: no projection
//   x = Xc / Zc,  y = Yc / Zc,  r2 = x x + y y,  r4 = r2 r2,  r6 = r4 r2,  rad = 1 + k1 r2 + k2 r4 + k3 r6   (left to right)
//   xd = x rad + 2 p1 x y + p2 (r2 + 2 x x),   yd = y rad + p1 (r2 + 2 y y) + 2 p2 x y    (2 p1 x y = ((2 p1) x) y)
//   u = fx xd + cx,  v = fy yd + cy.
// A prediction without a projection is (NaN, NaN), a residual +inf, as in board_fit_math.h.
// Board points: board_fit_math.h's layout centred on the board's centre, times tag_size:
//   X = (c (1 + s) + ox[j] - Bw/2) tag_size,  Y = (r (1 + s) + oy[j] - Bh/2) tag_size,  so t is in tag_size's unit.
// Seed.  (1) Every inlier corner is undistorted: x0 = (u - cx) / fx, y0 = (v - cy) / fy, (x, y) = (x0, y0), then 8 times, no
// early exit: r2, rad as above, dx = 2 p1 x y + p2 (r2 + 2 x x), dy = p1 (r2 + 2 y y) + 2 p2 x y, x = (x0 - dx) / rad,
// y = (y0 - dy) / rad.  (2) The homography from board_fit_math.h's normalised board points (X' = X sb / tag_size) to (x, y):
// fit_accumulate's 44 sums in fit's order of summation, fit_system, fit_solve.  (3) With q = sb / tag_size, a = q (h0, h3, h6),
// b = q (h1, h4, h7), c = (h2, h5, 1):  lambda = 2 / (|a| + |b|), r1 = lambda a, r2 = lambda b, t = lambda c, all negated if
// t_z < 0; Gram-Schmidt: r1 / |r1|, r2 - (r1 . r2) r1 normalised, r3 = r1 x r2.  A norm that is zero or not finite, or a t that
// is not finite: AGX_FIT_SINGULAR.
// Square roots: the norms of the seed and of the Gram-Schmidt, nowhere else (pose_sqrt: the correctly rounded binary64 root).
// Refinement: Gauss-Newton on the pixel residual e = observed - projected, local update R <- R C(w), t <- t + dt,
//   C(w) = (I - [w/2]x)^-1 (I + [w/2]x) = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a),  a = w / 2.
// Jacobian of a correspondence (2 x 6, unknowns w then dt) = M [G | I]:  M = diag(fx, fy) D P  with D the 2 x 2 derivative of
// (xd, yd) by (x, y), drad = k1 + 2 k2 r2 + 3 k3 r4,  P = [1 0 -x; 0 1 -y] / Zc;  G = -R [P]x, whose columns for Z = 0 are
// Y c3, -X c3, X c2 - Y c1 (ci the columns of R).
// Sums: the 21 entries i <= j of J^T J row by row (each correspondence as ja[i] ja[j] + jb[i] jb[j], one addition into the
// sum), the 6 of J^T e, and the sum of |e|^2 -- POSE_SUMS = 28 doubles, added in board_fit_math.h's order: lane l of 64 takes the
// inlier rows l, l + 64, ... in increasing order, corners 0 .. 3; the tree l ^ 32, 16, 8, 4, 2, 1.  A correspondence without a
// projection, or whose |e|^2 is not below +inf, adds +inf to the last sum and nothing to the others.
// Solve: fit_solve_n<6>, board_fit_math.h's elimination and pivot test on the 6 x 7 system.
// Iterates of a round: iterate 0 is the round's starting pose (the seed in the first round, the last round's answer after);
// iterate i + 1 is iterate i updated.  A singular system ends the round at the iterates so far; at iterate 0 (iterations > 0)
// it is AGX_FIT_SINGULAR.  The round's answer is the iterate with the lowest finite sum of |e|^2, the earliest at equal bits
// (iterate 0 if none is finite); the sum of the last iterate is one more pass.  The answer's R goes through the Gram-Schmidt once.
//
// The second lens model, AGX_LENS_EQUIDISTANT (Kalibr's pinhole-equi, OpenCV's fisheye, Kannala-Brandt with four coefficients).
// Every function that reads the camera is a template on LENS; AGX_LENS_RADTAN is the statements above, unchanged.  The nine
// doubles are then fx, fy, cx, cy, k1, k2, k3, k4, 0: agx_camera's p1 holds k3, its p2 holds k4, its k3 must be 0.
//   x, y, r2 as above;  r = pose_sqrt(r2);  r2 < POSE_EQUI_SMALL_R2 (2^-13):  q = 1 - r2 (1/3 - r2 (1/5 - r2 (1/7 - r2 / 9))),
//   theta = r q;  else theta = pose_atan(r), q = theta / r;   t2 = theta theta, t4 = t2 t2, t6 = t4 t2, t8 = t4 t4,
//   D = 1 + k1 t2 + k2 t4 + k3 t6 + k4 t8  (left to right),  s = q D,  u = fx (s x) + cx,  v = fy (s y) + cy.
// The series' first dropped term is r2^5 / 11 < 3e-21 below the threshold; on the optical axis q = D = s = 1 and the pixel is
// (cx, cy) exactly, with no division.  Zc not > 0: no projection, as above (the model is not carried behind the camera).
// pose_atan(r), r >= 0 finite: + - * / only.  t = r, or 1 / r above 1;  k = (int)(8 t + 1/2), the nearest break point k / 8 of
// 0 .. 8 (0 where 8 t + 1/2 is not in [0, 9): r not a number);  z = (t - k/8) / (1 + t k/8), |z| <= 1/16;  p = z - z z2 (1/3 - z2 (1/5 - z2 (1/7 - z2 (1/9 - z2 (1/11 - z2 / 13)))));
// a = POSE_ATAN_TABLE[k] + p;  above 1 the answer is (pi/2 high - a) + pi/2 low.  Not correctly rounded: within 1e-14 of atan.
// Jacobian of (s x, s y) by (x, y):  D' = 1 + 3 k1 t2 + 5 k2 t4 + 7 k3 t6 + 9 k4 t8,  g = (ds/dr) / r = (D' / (1 + r2) - s) / r2,
// below the threshold its limit 2 (k1 - 1/3) + 4 (k2 - k1 + 1/5) r2;  d00 = s + x x g, d01 = d10 = x y g, d11 = s + y y g.  The
// chain from there to (R, t), the sums, the solve, the iterates and the rounds are the ones above.
// Seed's undistortion: x0, y0 as above, theta_d = pose_sqrt(x0 x0 + y0 y0);  theta = theta_d, then POSE_EQUI_THETA_STEPS (8)
// times, no early exit:  theta = theta - (theta D(theta) - theta_d) / D'(theta);  theta >= POSE_EQUI_THETA_MAX (1.5 rad, for
// the seed only: a pinhole ray must exist) becomes POSE_EQUI_THETA_MAX;  tan(theta) from a = theta / 8 by the series of the
// tangent through a^15 and POSE_EQUI_TAN_DOUBLINGS (3) times t = 2 t / (1 - t t);  (x, y) = (x0, y0) tan(theta) / theta_d
// (theta_d = 0: (x0, y0)).  A value that is not finite reaches the seed's norm checks: AGX_FIT_SINGULAR.
//
// The third lens model, AGX_LENS_DOUBLE_SPHERE (Usenko, Demmel, Cremers 2018; Kalibr's ds, Basalt's default).  The nine doubles
// are fx, fy, cx, cy, xi, alpha, 0, 0, 0: agx_camera's k1 holds xi, its k2 holds alpha; -1 < xi <= 1, 0 <= alpha <= 1, the last
// three exactly 0.  + - * / and pose_sqrt only: no atan, no series, no iteration.  THE ORDER OF OPERATIONS:
//   Xc, Yc, Zc as above;  r2 = Xc Xc + Yc Yc,  d1 = pose_sqrt(r2 + Zc Zc);  no projection unless d1 > 0 and Zc > -(w2 d1);
//   k = xi d1 + Zc,  d2 = pose_sqrt(r2 + k k),  den = alpha d2 + (1 - alpha) k,  mx = Xc / den,  my = Yc / den,
//   u = fx mx + cx,  v = fy my + cy.
// Zc <= 0 is no refusal: the model is carried behind the image plane, out to the cone Zc = -w2 d1 (inside it den > 0).
//   w1 = alpha / (1 - alpha) for alpha <= 0.5, else (1 - alpha) / alpha;   w2 = (w1 + xi) / pose_sqrt(2 w1 xi + xi xi + 1).
// w2 depends on the camera only.  pose_camera() computes it once per call, on the host, for the kernel and the host form alike,
// and hands the functions below a camera whose k3 (the ninth double, 0 in the caller's) holds it: no function below is given a
// double-sphere camera that did not come through pose_camera().  (The calibration, calib_math.h, moves the camera on the device:
// pose_camera() is callable there, and every iterate's camera goes through it.)
// Jacobian m = d(u, v) / d(Xc, Yc, Zc), in closed form (x = Xc / Zc does not exist where Zc <= 0):  a = xi / d1,  b = alpha / d2,
//   s = b (1 + k a) + (1 - alpha) a  (d den / d Xc = Xc s, d den / d Yc = Yc s),  dz = (a Zc + 1) (b k + (1 - alpha))  (d den / d Zc),
//   id = 1 / den;   m00 = fx id (1 - mx (Xc s)),  m01 = -(fx id (mx (Yc s))),  m02 = -(fx id (mx dz)),
//                   m10 = -(fy id (my (Xc s))),  m11 = fy id (1 - my (Yc s)),  m12 = -(fy id (my dz)).
// The chain from m to (R, t), the sums, the solve, the iterates and the rounds are the ones above.
// Seed's unprojection, closed form:  x0 = (u - cx) / fx,  y0 = (v - cy) / fy,  r2 = x0 x0 + y0 y0,  t = 1 - (2 alpha - 1) r2
//   (t < 0: the pixel is outside the unprojection's domain, which happens for alpha > 0.5 only),
//   mz = (1 - alpha alpha r2) / (alpha pose_sqrt(t) + (1 - alpha)),  n = mz mz + r2,
//   sc = (mz xi + pose_sqrt(mz mz + (1 - xi xi) r2)) / n,   ray = (sc x0, sc y0, sc mz - xi),   (x, y) = (ray_x, ray_y) / ray_z.
// The seed needs a pinhole ray, so it clamps (the seed only; the refinement runs through the forward model and has no such
// limit): unless t >= 0 and ray_z > 0 and x x + y y < POSE_TAN_THETA_MAX^2 (the ray is less than POSE_EQUI_THETA_MAX = 1.5 rad
// off the axis; a value that is not a number fails the tests too), (x, y) = (x0, y0) (POSE_TAN_THETA_MAX / pose_sqrt(r2)),
// (0, 0) where r2 is not > 0.  On the principal point r2 = 0, mz = 1, ray = ((1 + xi) 0, (1 + xi) 0, (1 + xi) - xi): (0, 0) with
// no division by r.
#pragma once
#include <cstdint>
#include <type_traits>

#include "../../include/aprilgrid_amd.h"
#include "board_fit_math.h"

namespace agx {

constexpr int POSE_SUMS = 28;  // 21 of J^T J (i <= j) + 6 of J^T e + the sum of |e|^2
constexpr uint32_t POSE_MAX_ITERATIONS = 64;
constexpr int POSE_UNDISTORT_STEPS = 8;
constexpr int POSE_EQUI_THETA_STEPS = 8;        // Newton steps on theta D(theta) = theta_d, from theta = theta_d
constexpr int POSE_EQUI_TAN_DOUBLINGS = 3;      // tan(theta) from the series of tan(theta / 8)
constexpr double POSE_EQUI_THETA_MAX = 1.5;     // the seed's clamp on theta, radians
constexpr double POSE_EQUI_SMALL_R2 = 0x1p-13;  // below it theta / r and (ds/dr) / r come from their series
// atan(k / 8), k = 0 .. 8, to the nearest binary64
constexpr double POSE_ATAN_TABLE[9] = {0.0,
                                       0.12435499454676144,
                                       0.24497866312686414,
                                       0.35877067027057225,
                                       0.4636476090008061,
                                       0.5585993153435624,
                                       0.6435011087932844,
                                       0.7188299996216245,
                                       0.7853981633974483};
constexpr double POSE_PIO2_HI = 1.5707963267948966, POSE_PIO2_LO = 6.123233995736766e-17;
constexpr double POSE_TAN_THETA_MAX = 14.101419947171719;  // tan(POSE_EQUI_THETA_MAX) to the nearest binary64: the double-sphere seed's clamp

struct Pose {
    double R[9];  // row major, board -> camera
    double t[3];
};

// the layout's geometry as the pose reads it (the image half of FitGeom is not used)
AGX_HD FitGeom pose_geom(uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio)
{
    return fit_geom(cols, rows, first_id, spacing_ratio, 1, 1);
}

AGX_HD double pose_sqrt(double v) { return __builtin_sqrt(v); }

// atan(r) for r >= 0, finite: + - * / only, the same statements for both compilers (within 1e-14 of atan, not correctly rounded)
AGX_HD double pose_atan(double r)
{
    const bool above = r > 1.0;
    const double t = above ? 1.0 / r : r;
    const double kf = t * 8.0 + 0.5;
    const int k = kf >= 0.0 && kf < 9.0 ? (int)kf : 0;  // (an r that is not a number reads entry 0 and stays not a number)
    const double b = (double)k * 0.125;
    const double z = (t - b) / (1.0 + t * b), z2 = z * z;
    const double p = z - z * z2 * (1.0 / 3.0 - z2 * (1.0 / 5.0 - z2 * (1.0 / 7.0 - z2 * (1.0 / 9.0 - z2 * (1.0 / 11.0 - z2 / 13.0)))));
    const double a = POSE_ATAN_TABLE[k] + p;
    return above ? (POSE_PIO2_HI - a) + POSE_PIO2_LO : a;
}

// D(theta) and D'(theta) of the equidistant model from theta^2 (agx_camera's p1 holds k3, its p2 holds k4)
AGX_HD void pose_equi_poly(const agx_camera &c, double t2, double &D, double &Dp)
{
    const double t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
    D = 1.0 + c.k1 * t2 + c.k2 * t4 + c.p1 * t6 + c.p2 * t8;
    Dp = 1.0 + 3.0 * c.k1 * t2 + 5.0 * c.k2 * t4 + 7.0 * c.p1 * t6 + 9.0 * c.p2 * t8;
}

// corner j of the layout's tag t (0 .. n_board - 1) in the board's frame, in tag_size's unit
AGX_HD void pose_board_point(const FitGeom &g, double tag_size, uint32_t t, int j, double &X, double &Y)
{
    const uint32_t r = t / g.cols, c = t - r * g.cols;
    const double ox = (j == 1 || j == 2) ? 1.0 : 0.0, oy = j >= 2 ? 1.0 : 0.0;
    X = ((double)c * g.pitch + ox - g.bx) * tag_size;
    Y = ((double)r * g.pitch + oy - g.by) * tag_size;
}

// what the projection of one board point leaves for its Jacobian
struct PosePoint {
    double x, y, zc, r2, r4, rad, u, v;
};
struct PosePointEqui {
    double x, y, zc, s, g, u, v;  // s = theta_d / r, g = (ds/dr) / r
};
struct PosePointDs {
    double xc, yc, zc, d1, k, d2, den, mx, my, u, v;
};
template <int LENS>
using PosePointOf = std::conditional_t<LENS == AGX_LENS_DOUBLE_SPHERE, PosePointDs, std::conditional_t<LENS == AGX_LENS_EQUIDISTANT, PosePointEqui, PosePoint>>;

// the camera as the functions below read it: the caller's, and under AGX_LENS_DOUBLE_SPHERE its k3 holds w2, the valid cone's
// Zc / d1 (once per call, on the host, for both forms; the caller's camera has passed pose_args_ok)
AGX_HD agx_camera pose_camera(int lens, const agx_camera &c)
{
    agx_camera o = c;
    if (lens == AGX_LENS_DOUBLE_SPHERE) {
        const double xi = c.k1, al = c.k2;
        const double w1 = al <= 0.5 ? al / (1.0 - al) : (1.0 - al) / al;
        o.k3 = (w1 + xi) / pose_sqrt(2.0 * w1 * xi + xi * xi + 1.0);
    }
    return o;
}

// false: no projection -- Zc is not > 0, or under AGX_LENS_DOUBLE_SPHERE the point is not inside the valid cone (q untouched beyond zc)
template <int LENS = AGX_LENS_RADTAN>
AGX_HD bool pose_project(const agx_camera &c, const Pose &p, double X, double Y, PosePointOf<LENS> &q)
{
    const double xc = p.R[0] * X + p.R[1] * Y + p.t[0];
    const double yc = p.R[3] * X + p.R[4] * Y + p.t[1];
    q.zc = p.R[6] * X + p.R[7] * Y + p.t[2];
    if constexpr (LENS == AGX_LENS_DOUBLE_SPHERE) {  // (k1 holds xi, k2 alpha, k3 pose_camera's w2)
        const double r2 = xc * xc + yc * yc, d1 = pose_sqrt(r2 + q.zc * q.zc);
        if (!(d1 > 0.0) || !(q.zc > -(c.k3 * d1))) return false;
        const double k = c.k1 * d1 + q.zc, d2 = pose_sqrt(r2 + k * k);
        const double den = c.k2 * d2 + (1.0 - c.k2) * k;
        q.xc = xc;
        q.yc = yc;
        q.d1 = d1;
        q.k = k;
        q.d2 = d2;
        q.den = den;
        q.mx = xc / den;
        q.my = yc / den;
        q.u = c.fx * q.mx + c.cx;
        q.v = c.fy * q.my + c.cy;
        return true;
    } else {
        if (!(q.zc > 0.0)) return false;
        const double x = xc / q.zc, y = yc / q.zc;
        if constexpr (LENS == AGX_LENS_EQUIDISTANT) {
            const double r2 = x * x + y * y, r = pose_sqrt(r2);
            const bool small = r2 < POSE_EQUI_SMALL_R2;
            double th, tr;  // theta, theta / r
            if (small) {
                tr = 1.0 - r2 * (1.0 / 3.0 - r2 * (1.0 / 5.0 - r2 * (1.0 / 7.0 - r2 / 9.0)));
                th = r * tr;
            } else {
                th = pose_atan(r);
                tr = th / r;
            }
            double D, Dp;
            pose_equi_poly(c, th * th, D, Dp);
            const double s = tr * D;
            q.x = x;
            q.y = y;
            q.s = s;
            q.g = small ? 2.0 * (c.k1 - 1.0 / 3.0) + 4.0 * (c.k2 - c.k1 + 1.0 / 5.0) * r2 : (Dp / (1.0 + r2) - s) / r2;
            q.u = c.fx * (s * x) + c.cx;
            q.v = c.fy * (s * y) + c.cy;
        } else {
            const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
            const double rad = 1.0 + c.k1 * r2 + c.k2 * r4 + c.k3 * r6;
            const double xd = x * rad + 2.0 * c.p1 * x * y + c.p2 * (r2 + 2.0 * x * x);
            const double yd = y * rad + c.p1 * (r2 + 2.0 * y * y) + 2.0 * c.p2 * x * y;
            q.x = x;
            q.y = y;
            q.r2 = r2;
            q.r4 = r4;
            q.rad = rad;
            q.u = c.fx * xd + c.cx;
            q.v = c.fy * yd + c.cy;
        }
        return true;
    }
}

// |e|^2 of one correspondence: +inf without a projection or where the value is not below +inf
template <int LENS = AGX_LENS_RADTAN>
AGX_HD double pose_error(const agx_camera &c, const Pose &p, double X, double Y, double uo, double vo, PosePointOf<LENS> &q, double &eu, double &ev)
{
    if (!pose_project<LENS>(c, p, X, Y, q)) return __builtin_inf();
    eu = uo - q.u;
    ev = vo - q.v;
    const double e = eu * eu + ev * ev;
    return e < __builtin_inf() ? e : __builtin_inf();
}

// tan(theta) for |theta| <= POSE_EQUI_THETA_MAX: the series of tan(theta / 8) through a^15, then three doublings
AGX_HD double pose_tan(double theta)
{
    const double a = theta / 8.0, a2 = a * a;
    double t = a + a * a2 * (1.0 / 3.0 + a2 * (2.0 / 15.0 + a2 * (17.0 / 315.0 + a2 * (62.0 / 2835.0 + a2 * (1382.0 / 155925.0 +
               a2 * (21844.0 / 6081075.0 + a2 * (929569.0 / 638512875.0)))))));
#pragma unroll
    for (int i = 0; i < POSE_EQUI_TAN_DOUBLINGS; ++i) t = 2.0 * t / (1.0 - t * t);
    return t;
}

// a pixel to normalised coordinates under the equidistant model: theta from theta_d by Newton, its tangent, the ray
AGX_HD void pose_undistort_equi(const agx_camera &c, double u, double v, double &x, double &y)
{
    const double x0 = (u - c.cx) / c.fx, y0 = (v - c.cy) / c.fy;
    const double td = pose_sqrt(x0 * x0 + y0 * y0);
    double th = td;
    for (int i = 0; i < POSE_EQUI_THETA_STEPS; ++i) {
        double D, Dp;
        pose_equi_poly(c, th * th, D, Dp);
        th = th - (th * D - td) / Dp;
    }
    if (th >= POSE_EQUI_THETA_MAX) th = POSE_EQUI_THETA_MAX;
    const double k = td > 0.0 ? pose_tan(th) / td : 1.0;
    x = x0 * k;
    y = y0 * k;
}

// a pixel to normalised coordinates under the double-sphere model: the closed-form unprojection, its pinhole ray, the seed's clamp
AGX_HD void pose_undistort_ds(const agx_camera &c, double u, double v, double &x, double &y)
{
    const double xi = c.k1, al = c.k2;
    const double x0 = (u - c.cx) / c.fx, y0 = (v - c.cy) / c.fy;
    const double r2 = x0 * x0 + y0 * y0;
    const double t = 1.0 - (2.0 * al - 1.0) * r2;
    const double mz = (1.0 - al * al * r2) / (al * pose_sqrt(t) + (1.0 - al));
    const double n = mz * mz + r2;
    const double sc = (mz * xi + pose_sqrt(mz * mz + (1.0 - xi * xi) * r2)) / n;
    const double rz = sc * mz - xi;
    x = sc * x0 / rz;
    y = sc * y0 / rz;
    if (t >= 0.0 && rz > 0.0 && x * x + y * y < POSE_TAN_THETA_MAX * POSE_TAN_THETA_MAX) return;
    const double k = r2 > 0.0 ? POSE_TAN_THETA_MAX / pose_sqrt(r2) : 0.0;
    x = x0 * k;
    y = y0 * k;
}

// a pixel to normalised coordinates: POSE_UNDISTORT_STEPS steps of the fixed-point iteration
template <int LENS = AGX_LENS_RADTAN>
AGX_HD void pose_undistort(const agx_camera &c, double u, double v, double &x, double &y)
{
    if constexpr (LENS == AGX_LENS_DOUBLE_SPHERE) return pose_undistort_ds(c, u, v, x, y);
    if constexpr (LENS == AGX_LENS_EQUIDISTANT) return pose_undistort_equi(c, u, v, x, y);
    const double x0 = (u - c.cx) / c.fx, y0 = (v - c.cy) / c.fy;
    x = x0;
    y = y0;
    for (int i = 0; i < POSE_UNDISTORT_STEPS; ++i) {
        const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
        const double rad = 1.0 + c.k1 * r2 + c.k2 * r4 + c.k3 * r6;
        const double dx = 2.0 * c.p1 * x * y + c.p2 * (r2 + 2.0 * x * x);
        const double dy = c.p1 * (r2 + 2.0 * y * y) + 2.0 * c.p2 * x * y;
        x = (x0 - dx) / rad;
        y = (y0 - dy) / rad;
    }
}

// the seed's sums: the four correspondences of one table row (id on the board, corners finite) into a lane's FIT_SUMS
template <int LENS = AGX_LENS_RADTAN>
AGX_HD void pose_seed_accumulate_row(const FitGeom &g, const agx_camera &c, double acc[FIT_SUMS], uint32_t id, const float xy[8])
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double xn, yn, x, y;
        fit_board_point(g, id - g.first_id, j, xn, yn);
        pose_undistort<LENS>(c, (double)xy[2 * j], (double)xy[2 * j + 1], x, y);
        fit_accumulate(acc, xn, yn, x, y);
    }
}

// columns 0 and 1 of R normalised and made orthogonal, column 2 their cross product; false: a norm that is zero or not finite
AGX_HD bool pose_gram_schmidt(double R[9])
{
    double a0 = R[0], a1 = R[3], a2 = R[6], b0 = R[1], b1 = R[4], b2 = R[7];
    const double na = pose_sqrt(a0 * a0 + a1 * a1 + a2 * a2);
    if (!f64_finite(na) || !(na > 0.0)) return false;
    a0 = a0 / na;
    a1 = a1 / na;
    a2 = a2 / na;
    const double d = a0 * b0 + a1 * b1 + a2 * b2;
    b0 = b0 - d * a0;
    b1 = b1 - d * a1;
    b2 = b2 - d * a2;
    const double nb = pose_sqrt(b0 * b0 + b1 * b1 + b2 * b2);
    if (!f64_finite(nb) || !(nb > 0.0)) return false;
    b0 = b0 / nb;
    b1 = b1 / nb;
    b2 = b2 / nb;
    R[0] = a0;
    R[3] = a1;
    R[6] = a2;
    R[1] = b0;
    R[4] = b1;
    R[7] = b2;
    R[2] = a1 * b2 - a2 * b1;
    R[5] = a2 * b0 - a0 * b2;
    R[8] = a0 * b1 - a1 * b0;
    return true;
}

// the seed: the homography h (normalised board points -> normalised image points) decomposed; false: AGX_FIT_SINGULAR
AGX_HD bool pose_from_homography(const FitGeom &g, double tag_size, const double h[8], Pose &p)
{
    const double q = g.sb / tag_size;
    const double a0 = h[0] * q, a1 = h[3] * q, a2 = h[6] * q, b0 = h[1] * q, b1 = h[4] * q, b2 = h[7] * q;
    const double na = pose_sqrt(a0 * a0 + a1 * a1 + a2 * a2), nb = pose_sqrt(b0 * b0 + b1 * b1 + b2 * b2);
    const double lam = 2.0 / (na + nb);  // (t_z = lambda h33 with h33 = 1: never negative, so the negation never happens here)
    if (!f64_finite(lam) || !(lam > 0.0)) return false;
    p.R[0] = lam * a0;
    p.R[3] = lam * a1;
    p.R[6] = lam * a2;
    p.R[1] = lam * b0;
    p.R[4] = lam * b1;
    p.R[7] = lam * b2;
    p.t[0] = lam * h[2];
    p.t[1] = lam * h[5];
    p.t[2] = lam;
    if (!f64_finite(p.t[0]) || !f64_finite(p.t[1])) return false;
    return pose_gram_schmidt(p.R);
}

// one correspondence into a lane's sums
// the 2 x 2 derivative of the distorted point by (x, y)
AGX_HD void pose_lens_jacobian(const agx_camera &c, const PosePoint &q, double &d00, double &d01, double &d10, double &d11)
{
    const double x = q.x, y = q.y;
    const double drad = c.k1 + 2.0 * c.k2 * q.r2 + 3.0 * c.k3 * q.r4;
    d00 = q.rad + 2.0 * x * x * drad + 2.0 * c.p1 * y + 6.0 * c.p2 * x;
    d01 = 2.0 * x * y * drad + 2.0 * c.p1 * x + 2.0 * c.p2 * y;
    d10 = 2.0 * x * y * drad + 2.0 * c.p1 * x + 2.0 * c.p2 * y;
    d11 = q.rad + 2.0 * y * y * drad + 6.0 * c.p1 * y + 2.0 * c.p2 * x;
}
AGX_HD void pose_lens_jacobian(const agx_camera &, const PosePointEqui &q, double &d00, double &d01, double &d10, double &d11)
{
    const double x = q.x, y = q.y;
    d00 = q.s + x * x * q.g;
    d01 = x * y * q.g;
    d10 = x * y * q.g;
    d11 = q.s + y * y * q.g;
}
// the double-sphere model's d(u, v) / d(Xc, Yc, Zc), directly (no x = Xc / Zc: Zc may be <= 0)
AGX_HD void pose_ds_jacobian(const agx_camera &c, const PosePointDs &q, double &m00, double &m01, double &m02, double &m10, double &m11, double &m12)
{
    const double a = c.k1 / q.d1, b = c.k2 / q.d2, c1 = 1.0 - c.k2;
    const double s = b * (1.0 + q.k * a) + c1 * a;
    const double dz = (a * q.zc + 1.0) * (b * q.k + c1);
    const double id = 1.0 / q.den, fi = c.fx * id, gi = c.fy * id;
    const double sx = q.xc * s, sy = q.yc * s;
    m00 = fi * (1.0 - q.mx * sx);
    m01 = -(fi * (q.mx * sy));
    m02 = -(fi * (q.mx * dz));
    m10 = -(gi * (q.my * sx));
    m11 = gi * (1.0 - q.my * sy);
    m12 = -(gi * (q.my * dz));
}

// the 2 x 6 Jacobian of a projected correspondence by (w, dt): ja[0 .. 6) the row of u, jb[0 .. 6) the row of v (one text for
// pose_accumulate and calib_math.h's calib_row)
template <int LENS = AGX_LENS_RADTAN>
AGX_HD void pose_jacobian_rows(const agx_camera &c, const Pose &p, const PosePointOf<LENS> &q, double X, double Y, double *ja, double *jb)
{
    double m00, m01, m02, m10, m11, m12;  // d(u, v) / d(Xc, Yc, Zc)
    if constexpr (LENS == AGX_LENS_DOUBLE_SPHERE) {
        pose_ds_jacobian(c, q, m00, m01, m02, m10, m11, m12);
    } else {
        const double x = q.x, y = q.y;
        double d00, d01, d10, d11;
        pose_lens_jacobian(c, q, d00, d01, d10, d11);
        m00 = c.fx * d00 / q.zc, m01 = c.fx * d01 / q.zc, m02 = -(m00 * x + m01 * y);
        m10 = c.fy * d10 / q.zc, m11 = c.fy * d11 / q.zc, m12 = -(m10 * x + m11 * y);
    }
    // G = -R [P]x for P = (X, Y, 0): columns Y c3, -X c3, X c2 - Y c1
    const double g00 = Y * p.R[2], g10 = Y * p.R[5], g20 = Y * p.R[8];
    const double g01 = -(X * p.R[2]), g11 = -(X * p.R[5]), g21 = -(X * p.R[8]);
    const double g02 = X * p.R[1] - Y * p.R[0], g12 = X * p.R[4] - Y * p.R[3], g22 = X * p.R[7] - Y * p.R[6];
    ja[0] = m00 * g00 + m01 * g10 + m02 * g20, ja[1] = m00 * g01 + m01 * g11 + m02 * g21, ja[2] = m00 * g02 + m01 * g12 + m02 * g22;
    ja[3] = m00, ja[4] = m01, ja[5] = m02;
    jb[0] = m10 * g00 + m11 * g10 + m12 * g20, jb[1] = m10 * g01 + m11 * g11 + m12 * g21, jb[2] = m10 * g02 + m11 * g12 + m12 * g22;
    jb[3] = m10, jb[4] = m11, jb[5] = m12;
}

template <int LENS = AGX_LENS_RADTAN>
AGX_HD void pose_accumulate(const agx_camera &c, const Pose &p, double acc[POSE_SUMS], double X, double Y, double uo, double vo)
{
    PosePointOf<LENS> q;
    double eu = 0.0, ev = 0.0;
    const double e = pose_error<LENS>(c, p, X, Y, uo, vo, q, eu, ev);
    acc[27] += e;
    if (!(e < __builtin_inf())) return;
    double ja[7], jb[7];
    pose_jacobian_rows<LENS>(c, p, q, X, Y, ja, jb);
    ja[6] = eu;
    jb[6] = ev;
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j, ++k) acc[k] += ja[i] * ja[j] + jb[i] * jb[j];
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] += ja[i] * ja[6] + jb[i] * jb[6];
}

// the four correspondences of one inlier row into a lane's sums
template <int LENS = AGX_LENS_RADTAN>
AGX_HD void pose_accumulate_row(const FitGeom &g, double tag_size, const agx_camera &c, const Pose &p, double acc[POSE_SUMS], uint32_t id,
                                const float xy[8])
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double X, Y;
        pose_board_point(g, tag_size, id - g.first_id, j, X, Y);
        pose_accumulate<LENS>(c, p, acc, X, Y, (double)xy[2 * j], (double)xy[2 * j + 1]);
    }
}

// the folded sums as the augmented matrix m [6][7] (both halves of J^T J)
AGX_HD void pose_system(const double acc[POSE_SUMS], double *m)
{
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j, ++k) {
            m[7 * i + j] = acc[k];
            m[7 * j + i] = acc[k];
        }
#pragma unroll
    for (int i = 0; i < 6; ++i) m[7 * i + 6] = acc[21 + i];
}

// R <- R C(w), t <- t + dt;  d = (w, dt)
AGX_HD void pose_update(Pose &p, const double d[6])
{
    const double a = d[0] / 2.0, b = d[1] / 2.0, c = d[2] / 2.0;
    const double n = a * a + b * b + c * c, den = 1.0 + n, k = 1.0 - n;
    const double C[9] = {(k + 2.0 * a * a) / den,       (2.0 * a * b - 2.0 * c) / den, (2.0 * a * c + 2.0 * b) / den,
                         (2.0 * a * b + 2.0 * c) / den, (k + 2.0 * b * b) / den,       (2.0 * b * c - 2.0 * a) / den,
                         (2.0 * a * c - 2.0 * b) / den, (2.0 * b * c + 2.0 * a) / den, (k + 2.0 * c * c) / den};
    double R[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[3 * i + j] = p.R[3 * i] * C[j] + p.R[3 * i + 1] * C[3 + j] + p.R[3 * i + 2] * C[6 + j];
#pragma unroll
    for (int i = 0; i < 9; ++i) p.R[i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) p.t[i] = p.t[i] + d[3 + i];
}

// the residual of one table row under the pose: the largest of its four corners' |e|^2 in pixels, binary64 rounded to binary32;
// *sum gets the four corners' sum in corner order
template <int LENS = AGX_LENS_RADTAN>
AGX_HD float pose_row_residual(const FitGeom &g, double tag_size, const agx_camera &c, const Pose &p, uint32_t id, const float xy[8], double *sum)
{
    double worst = 0.0, total = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double X, Y, eu, ev;
        PosePointOf<LENS> q;
        pose_board_point(g, tag_size, id - g.first_id, j, X, Y);
        const double e = pose_error<LENS>(c, p, X, Y, (double)xy[2 * j], (double)xy[2 * j + 1], q, eu, ev);
        total += e;
        if (e > worst) worst = e;
    }
    *sum = total;
    return (float)worst;
}

// the predicted corners of the layout's tag t, rounded to binary32; NaN, NaN without a projection
template <int LENS = AGX_LENS_RADTAN>
AGX_HD void pose_predict(const FitGeom &g, double tag_size, const agx_camera &c, const Pose &p, uint32_t t, float xy[8])
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double X, Y;
        PosePointOf<LENS> q;
        pose_board_point(g, tag_size, t, j, X, Y);
        if (pose_project<LENS>(c, p, X, Y, q)) {
            xy[2 * j] = (float)q.u;
            xy[2 * j + 1] = (float)q.v;
        } else {
            xy[2 * j] = xy[2 * j + 1] = f32_from_bits(0x7fc00000u);
        }
    }
}

// the best-iterate rule: does an iterate whose sum of |e|^2 is `cost` replace the best so far
AGX_HD bool pose_better(double cost, bool have, double best_cost) { return f64_finite(cost) && (!have || cost < best_cost); }

// what both forms refuse in the camera and the pose's own scalars (under AGX_LENS_EQUIDISTANT the ninth double is 0; under
// AGX_LENS_DOUBLE_SPHERE the seventh, eighth and ninth are exactly 0, -1 < xi <= 1 and 0 <= alpha <= 1)
#define AGX_LENS_CAMERA_RULE /* the lens and camera half of it, for every entry point's message */                                            \
    "lens_model AGX_LENS_RADTAN, AGX_LENS_EQUIDISTANT (its ninth double 0) or AGX_LENS_DOUBLE_SPHERE (xi in (-1, 1], alpha in [0, 1], its last " \
    "three doubles 0), every camera field finite with fx and fy > 0"
AGX_HD bool pose_args_ok(int lens, const agx_camera &c, double tag_size, uint32_t iterations)
{
    const bool ds = lens == AGX_LENS_DOUBLE_SPHERE && c.p1 == 0.0 && c.p2 == 0.0 && c.k3 == 0.0 && c.k1 > -1.0 && c.k1 <= 1.0 && c.k2 >= 0.0 && c.k2 <= 1.0;
    if (lens != AGX_LENS_RADTAN && !(lens == AGX_LENS_EQUIDISTANT && c.k3 == 0.0) && !ds) return false;
    const double v[9] = {c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2, c.k3};
    for (int i = 0; i < 9; ++i)
        if (!f64_finite(v[i])) return false;
    return c.fx > 0.0 && c.fy > 0.0 && f64_finite(tag_size) && tag_size > 0.0 && iterations <= POSE_MAX_ITERATIONS;
}

// The one place where a lens model that is known at run time picks a template argument: f(std::integral_constant<int, AGX_LENS_*>{}).
// A value that is neither of the other two is AGX_LENS_RADTAN (the entry points have refused everything else).
template <class F>
inline auto with_lens(int lens, F f)
{
    if (lens == AGX_LENS_DOUBLE_SPHERE) return f(std::integral_constant<int, AGX_LENS_DOUBLE_SPHERE>{});
    if (lens == AGX_LENS_EQUIDISTANT) return f(std::integral_constant<int, AGX_LENS_EQUIDISTANT>{});
    return f(std::integral_constant<int, AGX_LENS_RADTAN>{});
}

}  // namespace agx
