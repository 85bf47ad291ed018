// calib_math.h -- the camera's nine doubles from a batch of tag tables (agx_calibrate_enqueue): Levenberg-damped Gauss-Newton on
// the pixel residual over the camera and every usable frame's pose, the poses eliminated frame by frame (the Schur complement of
// bundle adjustment).  One definition each for the kernels (calibrate.hip) and the host form (calibrate_host.cpp).
// The projection, its Jacobian by the pose, the pose's update and the elimination are board_pose_math.h's and board_fit_math.h's
// and are not restated.  Binary64, + - * / and pose_sqrt only, no contraction (-ffp-contract=off), so both forms give the same bytes.
//
// A correspondence's row has CALIB_COLS = 15 columns: the 9 of the camera in agx_camera's order (calib_param_jacobian<LENS>, in
// closed form from what pose_project<LENS> left), then the 6 of the pose (pose_jacobian_rows<LENS>: w, dt).  ja is the row of u,
// jb the row of v, e = observed - projected.
//   radial-tangential  fx: xd (recomputed by the projection's statement), cx: 1, k1 k2 k3: fx x r2, fx x r4, fx x r6,
//                      p1: fx 2xy | fy (r2 + 2yy), p2: fx (r2 + 2xx) | fy 2xy               (the same for v with fy, y, yd)
//   equidistant        fx: s x, k_i: fx x (theta / r) theta^(2i), the ninth 0; theta / r is the projection's (its series
//                      below POSE_EQUI_SMALL_R2)
//   double sphere      fx: mx, xi: -(fx mx / den) ((alpha k / d2 + (1 - alpha)) d1), alpha: -(fx mx / den) (d2 - k), 7..9: 0
// Per frame, over the inlier rows: U (9 x 9, the 45 entries i <= j), W (9 x 6), V (6 x 6, 21), gc = Jc^T e (9), gp = Jp^T e (6)
// and the sum of |e|^2 -- CALIB_SUMS = 136 doubles.  Every sum is added in board_fit_math.h's order: lane l of 64 takes the
// rows l, l + 64, .. in table order, corners 0 .. 3, each correspondence as ja[i] ja[j] + jb[i] jb[j] (one addition into the sum);
// the tree l ^ 32, 16, 8, 4, 2, 1.  The sums are independent of one another, so they may be taken in parts (calib_accumulate<LENS,
// PART>: 0 = U, |e|^2; 1 = W's rows 0 .. 4, gp; 2 = W's rows 5 .. 8, gc; 3 = V) -- the kernel makes one pass over its staged rows
// per part (the 136 sums and the row do not fit one lane's registers), the host form does too.
// A correspondence without a projection, or whose |e|^2 is not below +inf, adds +inf to the last sum and nothing to the others.
// Then, calib_frame_system: V's and U's diagonals times (1 + damping); a held camera column i has row and column i of U and row i
// of W set to 0, U_ii = 1, gc_i = 0.  V Y = W^T and V z = gp by fit_solve_multi<6, 10>: fit_solve_n's elimination, tie rule and
// pivot rule on the 6 x 16 augmented matrix [V | W^T | gp].  The frame's block: S_f = U - W Y (entries i <= j; each as
// ((U_ij - W_i0 Y_0j) - W_i1 Y_1j) - ..), r_f = gc - W z likewise, its |e|^2, Y and z (calib_schur_entry).
// Across frames: the 55 sums of S, r and |e|^2 (and the count of frames whose 6 x 16 system was refused) over the usable frames
// in frame order -- the usable frame of rank k is lane k mod 64's, the same tree.  An unusable frame takes no lane: a batch
// without it gives the same bytes.
// The reduced system (calib_reduced_solve): d_i = pose_sqrt(S_ii), which must be finite and > 0; S'_ij = S_ij / d_i / d_j,
// r'_i = r_i / d_i; fit_solve_n<9> (its 2^-40 rule now compares a scaled pivot against 1); dc_i = x_i / d_i.  The camera becomes
// c + dc (a held entry keeps its bits), each frame's pose goes through pose_update with dp = z - Y dc (calib_pose_step).
// Iterates: iterate 0 is the inputs.  calib_step (one lane, after the fold of iterate `it`) keeps the iterate with the lowest
// finite |e|^2 (pose_better: the lowest iterate at equal cost; iterate 0 while none is finite), and freezes the state -- every
// later launch stores nothing new -- when the iterate's cost is not finite, a frame's or the reduced system is refused, or the
// next camera fails pose_args_ok (that iterate's cost is then +inf).  A refused system at iterate 0 is AGX_CALIB_SINGULAR.
#pragma once
#include <cstdint>

#include "board_pose_math.h"

namespace agx {

constexpr int CALIB_CAM = 9, CALIB_POSE = 6, CALIB_COLS = 15;
constexpr int CALIB_SUMS = 136;                     // 45 + 54 + 21 + 9 + 6 + 1
constexpr int CALIB_PARTS = 4;
constexpr int CALIB_PART_SUMS[CALIB_PARTS] = {46, 36, 33, 21};  // U, |e|^2;  W's rows 0 .. 4, gp;  W's rows 5 .. 8, gc;  V
constexpr int CALIB_W_SPLIT = 5;
constexpr int CALIB_FOLD = 56;                      // S (45), r (9), |e|^2, refused frames
constexpr int CALIB_BLOCK = 116;                    // a frame's block: the 56, then Y [6][9] and z [6]
constexpr uint32_t CALIB_MAX_ITERATIONS = POSE_MAX_ITERATIONS;
constexpr uint32_t CALIB_MAX_FRAMES = 65535;

// an iterate that was not reached reports this cost
AGX_HD double calib_nan() { return __builtin_nan(""); }

// the camera slots a lens model defines as 0: always held
AGX_HD uint32_t calib_held(int lens, uint32_t fixed_mask)
{
    const uint32_t forced = lens == AGX_LENS_DOUBLE_SPHERE ? 0x1c0u : lens == AGX_LENS_EQUIDISTANT ? 0x100u : 0u;
    return (fixed_mask | forced) & 0x1ffu;
}

// ---- the 2 x 9 derivative of (u, v) by the nine camera doubles, from what pose_project<LENS> left in q -----------------------------
AGX_HD void calib_param_jacobian(const agx_camera &c, const PosePoint &q, double *ju, double *jv)
{
    const double x = q.x, y = q.y, r2 = q.r2, r4 = q.r4, r6 = r4 * r2;
    const double xd = x * q.rad + 2.0 * c.p1 * x * y + c.p2 * (r2 + 2.0 * x * x);  // pose_project's statements
    const double yd = y * q.rad + c.p1 * (r2 + 2.0 * y * y) + 2.0 * c.p2 * x * y;
    const double fxx = c.fx * x, fyy = c.fy * y;
    ju[0] = xd, ju[1] = 0.0, ju[2] = 1.0, ju[3] = 0.0;
    jv[0] = 0.0, jv[1] = yd, jv[2] = 0.0, jv[3] = 1.0;
    ju[4] = fxx * r2, ju[5] = fxx * r4, ju[8] = fxx * r6;
    jv[4] = fyy * r2, jv[5] = fyy * r4, jv[8] = fyy * r6;
    ju[6] = c.fx * (2.0 * x * y), ju[7] = c.fx * (r2 + 2.0 * x * x);
    jv[6] = c.fy * (r2 + 2.0 * y * y), jv[7] = c.fy * (2.0 * x * y);
}
AGX_HD void calib_param_jacobian(const agx_camera &c, const PosePointEqui &q, double *ju, double *jv)
{
    const double x = q.x, y = q.y;
    const double r2 = x * x + y * y, r = pose_sqrt(r2);
    double th, tr;  // theta, theta / r: pose_project's statements
    if (r2 < POSE_EQUI_SMALL_R2) {
        tr = 1.0 - r2 * (1.0 / 3.0 - r2 * (1.0 / 5.0 - r2 * (1.0 / 7.0 - r2 / 9.0)));
        th = r * tr;
    } else {
        th = pose_atan(r);
        tr = th / r;
    }
    const double t2 = th * th, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
    const double ax = c.fx * x * tr, ay = c.fy * y * tr;
    ju[0] = q.s * x, ju[1] = 0.0, ju[2] = 1.0, ju[3] = 0.0;
    jv[0] = 0.0, jv[1] = q.s * y, jv[2] = 0.0, jv[3] = 1.0;
    ju[4] = ax * t2, ju[5] = ax * t4, ju[6] = ax * t6, ju[7] = ax * t8, ju[8] = 0.0;
    jv[4] = ay * t2, jv[5] = ay * t4, jv[6] = ay * t6, jv[7] = ay * t8, jv[8] = 0.0;
}
AGX_HD void calib_param_jacobian(const agx_camera &c, const PosePointDs &q, double *ju, double *jv)
{
    const double al = c.k2;
    const double dxi = (al * q.k / q.d2 + (1.0 - al)) * q.d1;  // d den / d xi
    const double dal = q.d2 - q.k;                             // d den / d alpha
    const double su = -(c.fx * q.mx / q.den), sv = -(c.fy * q.my / q.den);
    ju[0] = q.mx, ju[1] = 0.0, ju[2] = 1.0, ju[3] = 0.0;
    jv[0] = 0.0, jv[1] = q.my, jv[2] = 0.0, jv[3] = 1.0;
    ju[4] = su * dxi, ju[5] = su * dal, ju[6] = 0.0, ju[7] = 0.0, ju[8] = 0.0;
    jv[4] = sv * dxi, jv[5] = sv * dal, jv[6] = 0.0, jv[7] = 0.0, jv[8] = 0.0;
}

// a correspondence's row: ja, jb [CALIB_COLS + 1], the last entry the residual; -> |e|^2 (+inf: no row)
template <int LENS>
AGX_HD double calib_row(const agx_camera &c, const Pose &p, double X, double Y, double uo, double vo, double *ja, double *jb)
{
    PosePointOf<LENS> q;
    double eu = 0.0, ev = 0.0;
    const double e = pose_error<LENS>(c, p, X, Y, uo, vo, q, eu, ev);
    if (!(e < __builtin_inf())) return e;
    calib_param_jacobian(c, q, ja, jb);
    pose_jacobian_rows<LENS>(c, p, q, X, Y, ja + CALIB_CAM, jb + CALIB_CAM);
    ja[CALIB_COLS] = eu;
    jb[CALIB_COLS] = ev;
    return e;
}

// one correspondence into a lane's sums of part PART (acc [CALIB_PART_SUMS[PART]])
template <int LENS, int PART>
AGX_HD void calib_accumulate(const agx_camera &c, const Pose &p, double *acc, double X, double Y, double uo, double vo)
{
    double ja[CALIB_COLS + 1], jb[CALIB_COLS + 1];
    const double e = calib_row<LENS>(c, p, X, Y, uo, vo, ja, jb);
    if constexpr (PART == 0) acc[45] += e;
    if (!(e < __builtin_inf())) return;
    if constexpr (PART == 0) {  // U (i <= j, row by row)
        int k = 0;
#pragma unroll
        for (int i = 0; i < CALIB_CAM; ++i)
#pragma unroll
            for (int j = i; j < CALIB_CAM; ++j, ++k) acc[k] += ja[i] * ja[j] + jb[i] * jb[j];
    } else if constexpr (PART == 1) {  // W's rows 0 .. 4 (row major, 6 a row), gp
#pragma unroll
        for (int i = 0; i < CALIB_W_SPLIT; ++i)
#pragma unroll
            for (int j = 0; j < CALIB_POSE; ++j) acc[6 * i + j] += ja[i] * ja[CALIB_CAM + j] + jb[i] * jb[CALIB_CAM + j];
#pragma unroll
        for (int j = 0; j < CALIB_POSE; ++j) acc[30 + j] += ja[CALIB_CAM + j] * ja[CALIB_COLS] + jb[CALIB_CAM + j] * jb[CALIB_COLS];
    } else if constexpr (PART == 2) {  // W's rows 5 .. 8, gc
#pragma unroll
        for (int i = CALIB_W_SPLIT; i < CALIB_CAM; ++i)
#pragma unroll
            for (int j = 0; j < CALIB_POSE; ++j) acc[6 * (i - CALIB_W_SPLIT) + j] += ja[i] * ja[CALIB_CAM + j] + jb[i] * jb[CALIB_CAM + j];
#pragma unroll
        for (int i = 0; i < CALIB_CAM; ++i) acc[24 + i] += ja[i] * ja[CALIB_COLS] + jb[i] * jb[CALIB_COLS];
    } else {  // V (i <= j, row by row)
        int k = 0;
#pragma unroll
        for (int i = 0; i < CALIB_POSE; ++i)
#pragma unroll
            for (int j = i; j < CALIB_POSE; ++j, ++k) acc[k] += ja[CALIB_CAM + i] * ja[CALIB_CAM + j] + jb[CALIB_CAM + i] * jb[CALIB_CAM + j];
    }
}

// the four correspondences of one inlier row into a lane's sums of part PART
template <int LENS, int PART>
AGX_HD void calib_accumulate_row(const FitGeom &g, double tag_size, const agx_camera &c, const Pose &p, double *acc, uint32_t id, const float xy[8])
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double X, Y;
        pose_board_point(g, tag_size, id - g.first_id, j, X, Y);
        calib_accumulate<LENS, PART>(c, p, acc, X, Y, (double)xy[2 * j], (double)xy[2 * j + 1]);
    }
}

// ---- a frame's system from its folded sums.  The arrays are indexed at run time: the kernel keeps them in LDS. -------------------
struct CalibFrameSys {
    double m[6 * 16];  // [V | W^T | gp], destroyed by the elimination
    double x[6 * 10];  // its solution: Y [6][9] in columns 0 .. 8, z in column 9
    double U[45], W[54], gc[9];
};

// part 0's folded sums: U, damped and masked
AGX_HD void calib_frame_system_u(const double *acc, double damping, uint32_t held, CalibFrameSys &s)
{
    int k = 0;
    for (int i = 0; i < CALIB_CAM; ++i)
        for (int j = i; j < CALIB_CAM; ++j, ++k) {
            const bool off = ((held >> i) | (held >> j)) & 1u;
            s.U[k] = off ? (i == j ? 1.0 : 0.0) : (i == j ? acc[k] * (1.0 + damping) : acc[k]);
        }
}
// part 1's (first = 0) and part 2's (first = CALIB_W_SPLIT): W's rows first .. last - 1 masked, and into the augmented matrix as
// columns of W^T; the part's other sums: gp into the matrix, gc masked
AGX_HD void calib_frame_system_w(const double *acc, int first, int last, uint32_t held, CalibFrameSys &s)
{
    for (int i = first; i < last; ++i)
        for (int j = 0; j < CALIB_POSE; ++j) {
            const double w = (held >> i) & 1u ? 0.0 : acc[6 * (i - first) + j];
            s.W[6 * i + j] = w;
            s.m[16 * j + 6 + i] = w;
        }
    if (first == 0)
        for (int j = 0; j < CALIB_POSE; ++j) s.m[16 * j + 15] = acc[30 + j];
    else
        for (int i = 0; i < CALIB_CAM; ++i) s.gc[i] = (held >> i) & 1u ? 0.0 : acc[24 + i];
}
// part 3's: V damped, both halves
AGX_HD void calib_frame_system_v(const double *acc, double damping, CalibFrameSys &s)
{
    int k = 0;
    for (int i = 0; i < CALIB_POSE; ++i)
        for (int j = i; j < CALIB_POSE; ++j, ++k) {
            s.m[16 * i + j] = i == j ? acc[k] * (1.0 + damping) : acc[k];
            s.m[16 * j + i] = s.m[16 * i + j];
        }
}

// fit_solve_n's elimination, tie rule and pivot rule with M right-hand sides: m [N][N + M] -> x [N][M]; m is destroyed
template <int N, int M>
AGX_HD bool fit_solve_multi(double *m, double *x)
{
    constexpr int W = N + M;
    double scale = 0.0;
    for (int i = 0; i < N; ++i) {
        const double d = __builtin_fabs(m[W * i + i]);
        if (!f64_finite(d)) return false;
        if (d > scale) scale = d;
    }
    const double tiny = scale * (1.0 / 1099511627776.0);  // 2^-40
    for (int c = 0; c < N; ++c) {
        int p = c;
        double best = __builtin_fabs(m[W * c + c]);
        for (int r = c + 1; r < N; ++r) {
            const double a = __builtin_fabs(m[W * r + c]);
            if (a > best) {  // (strictly: the lowest row stays at equal magnitude)
                best = a;
                p = r;
            }
        }
        if (!f64_finite(best) || !(best > tiny)) return false;
        if (p != c)
            for (int j = c; j < W; ++j) {
                const double t = m[W * c + j];
                m[W * c + j] = m[W * p + j];
                m[W * p + j] = t;
            }
        const double piv = m[W * c + c];
        for (int r = c + 1; r < N; ++r) {
            const double f = m[W * r + c] / piv;
            for (int j = c + 1; j < W; ++j) m[W * r + j] = m[W * r + j] - f * m[W * c + j];
        }
    }
    for (int k = 0; k < M; ++k)
        for (int c = N - 1; c >= 0; --c) {
            double s = m[W * c + N + k];
            for (int j = c + 1; j < N; ++j) s = s - m[W * c + j] * x[M * j + k];
            x[M * c + k] = s / m[W * c + c];
            if (!f64_finite(x[M * c + k])) return false;
        }
    return true;
}

// entry t of a frame's block: t < 45 S_f (i <= j, row by row), 45 .. 53 r_f
AGX_HD double calib_schur_entry(const CalibFrameSys &s, int t)
{
    if (t >= 45) {
        const int i = t - 45;
        double v = s.gc[i];
        for (int k = 0; k < CALIB_POSE; ++k) v = v - s.W[6 * i + k] * s.x[10 * k + 9];
        return v;
    }
    int i = 0, first = 0;  // row i holds the entries first .. first + 9 - i
    while (t >= first + CALIB_CAM - i) {
        first += CALIB_CAM - i;
        ++i;
    }
    const int j = i + (t - first);
    double v = s.U[t];
    for (int k = 0; k < CALIB_POSE; ++k) v = v - s.W[6 * i + k] * s.x[10 * k + j];
    return v;
}

// a frame's pose step: dp = z - Y dc (left to right), through pose_update;  yz: the block's Y [6][9] then z [6]
AGX_HD void calib_pose_step(Pose &p, const double *yz, const double *dc)
{
    double dp[6];
    for (int k = 0; k < CALIB_POSE; ++k) {
        double v = yz[54 + k];
        for (int i = 0; i < CALIB_CAM; ++i) v = v - yz[9 * k + i] * dc[i];
        dp[k] = v;
    }
    pose_update(p, dp);
}

// the reduced system from the folded S (45) and r (9) -> dc [9];  m: CALIB_SCRATCH doubles, indexed at run time;  false: refused
constexpr int CALIB_SCRATCH = 90 + 9 + 9;  // the 9 x 10 system, its solution, the scales
AGX_HD bool calib_reduced_solve(const double *fold, double *m, double *dc)
{
    double *x = m + 90, *d = m + 99;
    int k = 0;
    for (int i = 0; i < CALIB_CAM; ++i) {
        d[i] = pose_sqrt(fold[k]);
        if (!f64_finite(d[i]) || !(d[i] > 0.0)) return false;
        k += CALIB_CAM - i;
    }
    k = 0;
    for (int i = 0; i < CALIB_CAM; ++i)
        for (int j = i; j < CALIB_CAM; ++j, ++k) {
            m[10 * i + j] = fold[k] / d[i] / d[j];
            m[10 * j + i] = m[10 * i + j];
        }
    for (int i = 0; i < CALIB_CAM; ++i) m[10 * i + 9] = fold[45 + i] / d[i];
    if (!fit_solve_n<CALIB_CAM>(m, x)) return false;
    for (int i = 0; i < CALIB_CAM; ++i) {
        dc[i] = x[i] / d[i];
        if (!f64_finite(dc[i])) return false;
    }
    return true;
}

// ---- the call's state between launches (device memory in the kernels' workspace) -------------------------------------------------
struct CalibCtl {
    double cam[9];       // the current iterate's camera (the caller's nine: no w2)
    double cam_best[9];  // the best iterate's
    double dc[9];        // the step the next blocks launch applies (apply != 0)
    double cost[CALIB_MAX_ITERATIONS + 1];
    double best_cost;
    uint32_t status;     // AGX_CALIB_*
    uint32_t frozen;     // no launch stores anything new
    uint32_t have;       // an iterate with a finite cost was seen
    uint32_t mark_best;  // the iterate just folded is the best: the next blocks launch keeps its poses and frame costs
    uint32_t apply;      // dc is a step to take
    uint32_t best_it, it_run, n_usable, n_corners;
    uint32_t pad;
};

AGX_HD agx_camera calib_camera(const double *c) { return agx_camera{c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8]}; }

// the state at the start of a call
AGX_HD void calib_ctl_init(CalibCtl &t, const double *camera)
{
    for (int i = 0; i < 9; ++i) t.cam[i] = t.cam_best[i] = camera[i], t.dc[i] = 0.0;
    for (uint32_t i = 0; i <= CALIB_MAX_ITERATIONS; ++i) t.cost[i] = calib_nan();
    t.best_cost = 0.0;
    t.status = AGX_CALIB_OK;
    t.frozen = t.have = t.mark_best = t.apply = t.best_it = t.it_run = t.n_usable = t.n_corners = t.pad = 0u;
}

// is the call refused as AGX_CALIB_FEW (known once the usable frames are counted, before iterate 0 is folded)
AGX_HD bool calib_few(uint32_t n_usable, uint32_t n_corners, uint32_t min_frames, uint32_t held)
{
    uint32_t n_free = 0;
    for (int i = 0; i < CALIB_CAM; ++i) n_free += ((held >> i) & 1u) ^ 1u;
    return n_usable < min_frames || n_usable == 0u || (uint64_t)n_corners < (uint64_t)n_free + 6ull * n_usable;
}

// The best-iterate and freeze core of a call's control block, one text for calib_step here and rig_math.h's rig_step.  Ctl has
// cost[], best_cost, frozen, have, mark_best, apply, best_it, it_run and status; *cost is iterate `it`'s folded |e|^2 (read only
// while the state is not frozen); keep() copies the current iterate's unknowns to the best's.  -> true: a step is to be solved for.
template <class Ctl, class Keep>
AGX_HD bool ctl_iterate(Ctl &t, uint32_t it, uint32_t iterations, const double *cost_at, Keep keep)
{
    t.mark_best = 0u;
    t.apply = 0u;
    if (t.frozen) return false;
    const double cost = *cost_at;
    t.cost[it] = cost;
    t.it_run = it;
    if (it == 0u || pose_better(cost, t.have != 0u, t.best_cost)) {  // (iterate 0 stands while no cost is finite)
        if (f64_finite(cost)) t.have = 1u, t.best_cost = cost;
        t.best_it = it;
        t.mark_best = 1u;
        keep();
    }
    if (!f64_finite(cost)) {
        t.frozen = 1u;
        return false;
    }
    return it != iterations;  // (the last launches gave the final iterate's cost only)
}
// a refused system ends the steps; at iterate 0 it is the call's `singular` status
template <class Ctl>
AGX_HD void ctl_refused(Ctl &t, uint32_t it, uint32_t singular)
{
    if (it == 0u) t.status = singular;
    t.frozen = 1u;
}

// One lane, after iterate `it`'s blocks were folded (fold [CALIB_FOLD]): the best rule, the reduced solve, the next camera.
// fold and m (CALIB_SCRATCH doubles) are indexed at run time: LDS in the kernel.
AGX_HD void calib_step(CalibCtl &t, uint32_t it, uint32_t iterations, int lens, uint32_t held, const double *fold, double *m)
{
    if (!ctl_iterate(t, it, iterations, fold + 54, [&]() {
            for (int i = 0; i < 9; ++i) t.cam_best[i] = t.cam[i];
        }))
        return;
    double *dc = t.dc;  // (read by the next blocks launch only under apply)
    if (fold[55] != 0.0 || !calib_reduced_solve(fold, m, dc)) return ctl_refused(t, it, AGX_CALIB_SINGULAR);
    double *next = m;  // (the system is spent)
    for (int i = 0; i < 9; ++i) next[i] = (held >> i) & 1u ? t.cam[i] : t.cam[i] + dc[i];
    if (!pose_args_ok(lens, calib_camera(next), 1.0, 0u)) {  // the step leaves the model's domain: that iterate's cost is +inf
        t.cost[it + 1u] = __builtin_inf();
        t.it_run = it + 1u;
        t.frozen = 1u;
        return;
    }
    for (int i = 0; i < 9; ++i) t.cam[i] = next[i];
    t.apply = 1u;
}

// what both forms refuse in the call's own scalars (the camera is pose_args_ok's)
AGX_HD bool calib_args_ok(double damping, uint32_t iterations, uint32_t min_tags, uint32_t min_frames, uint32_t fixed_mask, int flags)
{
    return f64_finite(damping) && damping >= 0.0 && iterations <= CALIB_MAX_ITERATIONS && min_tags >= 1u && min_frames >= 1u && fixed_mask <= 0x1ffu &&
           !(flags & ~AGX_CALIB_ACCEPT_LOOSE);
}

// which frames and rows count, fixed for the whole call: a frame by agx_board_pose_enqueue_m's status word, a row by its mask
// (and an id on the board: the row has a board point)
AGX_HD bool calib_frame_ok(uint32_t fit_status, int flags) { return fit_status == AGX_FIT_OK || ((flags & AGX_CALIB_ACCEPT_LOOSE) && fit_status == AGX_FIT_LOOSE); }
AGX_HD bool calib_row_counts(const FitGeom &g, uint32_t id, uint32_t row_status) { return row_status == AGX_FIT_ROW_INLIER && fit_on_board(g, id); }

// what every call's report says of its iterates, one text for calib_report here and rig_math.h's rig_report: the RMS is
// pose_sqrt(best cost / corners), not a number under the call's `few` status
template <class Ctl, class Rep>
AGX_HD void ctl_report_iterates(const Ctl &t, Rep *r, uint32_t few)
{
    r->rms = t.status == few ? calib_nan() : pose_sqrt(t.cost[t.best_it] / (double)t.n_corners);
    for (uint32_t i = 0; i <= CALIB_MAX_ITERATIONS; ++i) r->cost[i] = t.cost[i];
}

// the call's report from its final state
AGX_HD void calib_report(const CalibCtl &t, agx_calib_report *r)
{
    r->status = t.status;
    r->best_iter = t.best_it;
    r->iterations_run = t.it_run;
    r->n_frames_used = t.n_usable;
    r->n_corners = t.n_corners;
    r->reserved = 0u;
    ctl_report_iterates(t, r, AGX_CALIB_FEW);
}

}  // namespace agx
