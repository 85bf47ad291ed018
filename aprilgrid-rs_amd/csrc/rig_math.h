// rig_math.h -- the extrinsics of a rig of cameras from synchronised tag tables (agx_rig_calibrate_enqueue): Levenberg-damped
// Gauss-Newton on the pixel residual over every free camera's E_c (camera from rig) and every usable instant's T_s (rig from
// board), the T_s eliminated instant by instant (the Schur complement, as calib_math.h eliminates the frames' poses).  One
// definition each for the kernels (rig.hip) and the host form (rig_host.cpp).  The projection, its Jacobian by the point of the
// camera frame, pose_update, the eliminations, the frame and row rules and the best-iterate comparison are board_pose_math.h's,
// board_fit_math.h's and calib_math.h's and are not restated.  Binary64, + - * / and pose_sqrt only, no contraction.
//
// Frame f = c n_instants + s is camera c at instant s; its board-to-camera pose is P = E_c o T_s (rig_compose: R = R_E R_T,
// t = R_E t_T + t_E, each entry left to right).  E_0 is the identity and camera 0's frames read P = T_s itself.
// Updates: pose_update on E_c and on T_s (R <- R C(w), t <- t + dt, the one text there is): 6 + 6 unknowns a frame.
// A correspondence's row (rig_row<LENS>) has RIG_COLS = 12 columns, [dE_c | dT_s], with m = d(u, v) / d(Xc, Yc, Zc) and the first
// three columns of pose_jacobian_rows<LENS> under P, and Q = R_T X + t_T the point in the rig's frame, r_k the columns of R_E:
//   dE: w  m (Q1 r_2 - Q2 r_1), m (Q2 r_0 - Q0 r_2), m (Q0 r_1 - Q1 r_0)   (= -R_E [Q]x);   dt  m
//   dT: w  pose_jacobian_rows' (-R [X]x under the composed R);                              dt  m R_E
// Per counted frame of a camera c >= 1, RIG_SUMS = 91: the 78 entries i <= j of J^T J row by row, the 12 of J^T e, |e|^2, in
// board_fit_math.h's order (lane l of 64 takes rows l, l + 64, .., corners 0 .. 3, one addition a correspondence; the tree
// l ^ 32 .. 1).  Taken in three parts (rig_accumulate<LENS, PART>): 0 = rows 0 .. 2 of J^T J (33); 1 = rows 3 .. 5 (24) and
// the 6 of dE's J^T e; 2 = rows 6 .. 11 (V, 21), the 6 of dT's J^T e and |e|^2.  A frame of camera 0 takes the T_s part alone:
// pose_accumulate_row<LENS>'s 28 sums under T_s, which have part 2's layout.  A frame's block (RIG_FRAME = 91): J^T J at 0,
// J^T e at 78, |e|^2 at 90.
// Per usable instant (rig_instant_*): V_s, its gradient and the cost are summed over the instant's counted frames in camera
// order; V's and every U_c's diagonal times (1 + damping); [V | W_1^T .. W_{C-1}^T | g] (6 x (6 C + 1), a camera without a
// counted frame here has zero columns) through fit_solve_multi<6, 6 (C - 1) + 1>; the instant's contribution to the reduced
// n = 6 (C - 1) square system: S_IJ = [same camera] U_ij - sum_k W_Ik Y_kJ (0 where either camera has no frame here),
// r_I = g_I - sum_k W_Ik z_k, each as ((a - b0) - b1) - ...  An instant's block: S (n (n + 1) / 2, i <= j row by row), r (n),
// the cost, refused (0 / 1), Y [6][n], z [6].
// Across instants: the first n (n + 1) / 2 + n + 2 entries are added over the usable instants in instant order, the usable
// instant of rank k is lane k mod 64's, the same tree.  An unusable instant takes no lane.  A camera c >= 1 without a counted
// frame is held: calib_math.h's rule for a held double on its six (row and column 0, U_ii = 1, g_i = 0).  The reduced system is
// scaled by d_i = pose_sqrt(S_ii) as calib_reduced_solve scales its own and solved by fit_solve_n<n> (the 2^-40 rule against 1).
// Step: E_c <- pose_update(E_c, dE_c); T_s <- pose_update(T_s, z_s - Y_s dE) (left to right).
// Iterates: calib_math.h's rule and text (ctl_iterate, ctl_refused, ctl_report_iterates: iterate 0 is the inputs and stands while
// no cost is finite; a cost that is not finite or a refused system freezes the state; a refusal at iterate 0 is AGX_RIG_SINGULAR).
#pragma once
#include <cstdint>

#include "calib_math.h"

namespace agx {

constexpr int RIG_MAX_CAMS = 8, RIG_MIN_CAMS = 2;
constexpr int RIG_COLS = 12, RIG_SUMS = 91, RIG_FRAME = 91;
constexpr int RIG_PARTS = 3;
constexpr int RIG_PART_SUMS[RIG_PARTS] = {33, 30, POSE_SUMS};
constexpr int RIG_MAX_N = 6 * (RIG_MAX_CAMS - 1);          // the reduced system's side
constexpr int RIG_MAX_W = 6 * RIG_MAX_CAMS + 1;            // the widest row of an instant's elimination
constexpr int RIG_FOLD_CHUNK = 32;                         // entries of an instant's block a lane of k_rig_solve adds at a time

AGX_HD int rig_n(int n_cams) { return 6 * (n_cams - 1); }
AGX_HD int rig_tri(int n) { return n * (n + 1) / 2; }
AGX_HD int rig_fold_len(int n_cams) { return rig_tri(rig_n(n_cams)) + rig_n(n_cams) + 2; }      // S, r, cost, refused
AGX_HD int rig_block_len(int n_cams) { return rig_fold_len(n_cams) + 6 * rig_n(n_cams) + 6; }   // .. Y [6][n], z [6]
// entry (i, j), i <= j, of a symmetric matrix of side n kept as its rows i <= j
AGX_HD int rig_sym(int n, int i, int j) { return i * n - i * (i - 1) / 2 + (j - i); }

AGX_HD Pose rig_identity() { return Pose{{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, {0.0, 0.0, 0.0}}; }
AGX_HD Pose rig_load(const double *p)
{
    Pose o;
#pragma unroll
    for (int i = 0; i < 9; ++i) o.R[i] = p[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) o.t[i] = p[9 + i];
    return o;
}
AGX_HD void rig_store(double *p, const Pose &o)
{
#pragma unroll
    for (int i = 0; i < 9; ++i) p[i] = o.R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) p[9 + i] = o.t[i];
}

// a o b: first b, then a
AGX_HD Pose rig_compose(const Pose &a, const Pose &b)
{
    Pose o;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) o.R[3 * i + j] = a.R[3 * i] * b.R[j] + a.R[3 * i + 1] * b.R[3 + j] + a.R[3 * i + 2] * b.R[6 + j];
        o.t[i] = a.R[3 * i] * b.t[0] + a.R[3 * i + 1] * b.t[1] + a.R[3 * i + 2] * b.t[2] + a.t[i];
    }
    return o;
}
// the inverse of a rigid pose: R^T, -(R^T t)
AGX_HD Pose rig_inverse(const Pose &a)
{
    Pose o;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) o.R[3 * i + j] = a.R[3 * j + i];
        o.t[i] = -(a.R[i] * a.t[0] + a.R[3 + i] * a.t[1] + a.R[6 + i] * a.t[2]);
    }
    return o;
}
// an instant's seed from the pose of its lowest usable camera: E_c^-1 o pose (camera 0: the pose itself)
AGX_HD Pose rig_seed_instant(int c, const Pose &e, const Pose &pose) { return c == 0 ? pose : rig_compose(rig_inverse(e), pose); }

// a correspondence's row under a camera c >= 1: ja, jb [RIG_COLS + 1], the last entry the residual; -> |e|^2 (+inf: no row)
template <int LENS>
AGX_HD double rig_row(const agx_camera &c, const Pose &e, const Pose &t, const Pose &p, double X, double Y, double uo, double vo, double *ja, double *jb)
{
    PosePointOf<LENS> q;
    double eu = 0.0, ev = 0.0;
    const double err = pose_error<LENS>(c, p, X, Y, uo, vo, q, eu, ev);
    if (!(err < __builtin_inf())) return err;
    pose_jacobian_rows<LENS>(c, p, q, X, Y, ja + 6, jb + 6);  // dT's w; m in [9 .. 12)
    const double a0 = ja[9], a1 = ja[10], a2 = ja[11], b0 = jb[9], b1 = jb[10], b2 = jb[11];
    const double q0 = t.R[0] * X + t.R[1] * Y + t.t[0], q1 = t.R[3] * X + t.R[4] * Y + t.t[1], q2 = t.R[6] * X + t.R[7] * Y + t.t[2];
    const double *r = e.R;
    const double g00 = q1 * r[2] - q2 * r[1], g10 = q1 * r[5] - q2 * r[4], g20 = q1 * r[8] - q2 * r[7];
    const double g01 = q2 * r[0] - q0 * r[2], g11 = q2 * r[3] - q0 * r[5], g21 = q2 * r[6] - q0 * r[8];
    const double g02 = q0 * r[1] - q1 * r[0], g12 = q0 * r[4] - q1 * r[3], g22 = q0 * r[7] - q1 * r[6];
    ja[0] = a0 * g00 + a1 * g10 + a2 * g20, ja[1] = a0 * g01 + a1 * g11 + a2 * g21, ja[2] = a0 * g02 + a1 * g12 + a2 * g22;
    jb[0] = b0 * g00 + b1 * g10 + b2 * g20, jb[1] = b0 * g01 + b1 * g11 + b2 * g21, jb[2] = b0 * g02 + b1 * g12 + b2 * g22;
    ja[3] = a0, ja[4] = a1, ja[5] = a2;
    jb[3] = b0, jb[4] = b1, jb[5] = b2;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ja[9 + k] = a0 * r[k] + a1 * r[3 + k] + a2 * r[6 + k];
        jb[9 + k] = b0 * r[k] + b1 * r[3 + k] + b2 * r[6 + k];
    }
    ja[RIG_COLS] = eu;
    jb[RIG_COLS] = ev;
    return err;
}

// one correspondence into a lane's sums of part PART (acc [RIG_PART_SUMS[PART]])
template <int LENS, int PART>
AGX_HD void rig_accumulate(const agx_camera &c, const Pose &e, const Pose &t, const Pose &p, double *acc, double X, double Y, double uo, double vo)
{
    double ja[RIG_COLS + 1], jb[RIG_COLS + 1];
    const double err = rig_row<LENS>(c, e, t, p, X, Y, uo, vo, ja, jb);
    if constexpr (PART == 2) acc[27] += err;
    if (!(err < __builtin_inf())) return;
    constexpr int FIRST = PART == 0 ? 0 : PART == 1 ? 3 : 6, LAST = PART == 0 ? 3 : PART == 1 ? 6 : 12;
    int k = 0;
#pragma unroll
    for (int i = FIRST; i < LAST; ++i)
#pragma unroll
        for (int j = i; j < RIG_COLS; ++j, ++k) acc[k] += ja[i] * ja[j] + jb[i] * jb[j];
    if constexpr (PART == 1) {
#pragma unroll
        for (int i = 0; i < 6; ++i) acc[24 + i] += ja[i] * ja[RIG_COLS] + jb[i] * jb[RIG_COLS];
    }
    if constexpr (PART == 2) {
#pragma unroll
        for (int i = 0; i < 6; ++i) acc[21 + i] += ja[6 + i] * ja[RIG_COLS] + jb[6 + i] * jb[RIG_COLS];
    }
}

// the four correspondences of one inlier row into a lane's sums of part PART
template <int LENS, int PART>
AGX_HD void rig_accumulate_row(const FitGeom &g, double tag_size, const agx_camera &c, const Pose &e, const Pose &t, const Pose &p, double *acc,
                               uint32_t id, const float xy[8])
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double X, Y;
        pose_board_point(g, tag_size, id - g.first_id, j, X, Y);
        rig_accumulate<LENS, PART>(c, e, t, p, acc, X, Y, (double)xy[2 * j], (double)xy[2 * j + 1]);
    }
}

// where part PART's folded sum k goes in the frame's block
AGX_HD int rig_part_slot(int part, int k)
{
    if (part == 0) return k;
    if (part == 1) return k < 24 ? 33 + k : 78 + (k - 24);
    return k < 21 ? 57 + k : k < 27 ? 84 + (k - 21) : 90;
}

// ---- an instant's system from its frames' blocks.  blk(c): camera c's frame block at this instant, null where it has none. ----
// entry e of the 28 summed over the cameras in camera order: V (21), its gradient (6), the cost
template <class B>
AGX_HD double rig_instant_sum(int n_cams, const B &blk, int e)
{
    const int slot = rig_part_slot(2, e);
    double v = 0.0;
    for (int c = 0; c < n_cams; ++c)
        if (const double *b = blk(c)) v += b[slot];
    return v;
}
// entry (k, col) of the instant's augmented matrix [V | W_1^T .. | g] (row stride 6 n_cams + 1) from the 28 sums and the blocks
template <class B>
AGX_HD double rig_instant_entry(int n_cams, const B &blk, const double *sum28, double damping, int k, int col)
{
    const int n = rig_n(n_cams);
    if (col < 6) {
        const double v = sum28[k <= col ? rig_sym(6, k, col) : rig_sym(6, col, k)];
        return k == col ? v * (1.0 + damping) : v;
    }
    if (col == 6 + n) return sum28[21 + k];
    const int a = (col - 6) / 6, i = (col - 6) - 6 * a;
    const double *b = blk(a + 1);
    return b ? b[rig_sym(RIG_COLS, i, 6 + k)] : 0.0;
}

// fit_solve_multi<6, 6 (C - 1) + 1> at the call's camera count: m [6][6 C + 1] -> x [6][6 (C - 1) + 1]
AGX_HD bool rig_eliminate(int n_cams, double *m, double *x)
{
    switch (n_cams) {
    case 2: return fit_solve_multi<6, 7>(m, x);
    case 3: return fit_solve_multi<6, 13>(m, x);
    case 4: return fit_solve_multi<6, 19>(m, x);
    case 5: return fit_solve_multi<6, 25>(m, x);
    case 6: return fit_solve_multi<6, 31>(m, x);
    case 7: return fit_solve_multi<6, 37>(m, x);
    default: return fit_solve_multi<6, 43>(m, x);
    }
}

// entry t of an instant's contribution: t < n (n + 1) / 2: S_IJ (I <= J row by row), then r_I;  x: rig_eliminate's solution
template <class B>
AGX_HD double rig_schur_entry(int n_cams, const B &blk, const double *x, double damping, int t)
{
    const int n = rig_n(n_cams), nt = rig_tri(n), M = n + 1;
    if (t >= nt) {
        const int I = t - nt, a = I / 6, i = I - 6 * a;
        const double *b = blk(a + 1);
        if (!b) return 0.0;
        double v = b[78 + i];
        for (int k = 0; k < 6; ++k) v = v - b[rig_sym(RIG_COLS, i, 6 + k)] * x[M * k + n];
        return v;
    }
    int I = 0, first = 0;  // row I holds the entries first .. first + n - I
    while (t >= first + n - I) {
        first += n - I;
        ++I;
    }
    const int J = I + (t - first);
    const int a = I / 6, i = I - 6 * a, c = J / 6, j = J - 6 * c;
    const double *b = blk(a + 1);
    if (!b || !blk(c + 1)) return 0.0;
    double v = 0.0;
    if (a == c) {
        v = b[rig_sym(RIG_COLS, i, j)];
        if (i == j) v = v * (1.0 + damping);
    }
    for (int k = 0; k < 6; ++k) v = v - b[rig_sym(RIG_COLS, i, 6 + k)] * x[M * k + J];
    return v;
}

// fit_solve_n<n> at the call's camera count: m [n][n + 1] -> x [n]
AGX_HD bool rig_solve_n(int n_cams, double *m, double *x)
{
    switch (n_cams) {
    case 2: return fit_solve_n<6>(m, x);
    case 3: return fit_solve_n<12>(m, x);
    case 4: return fit_solve_n<18>(m, x);
    case 5: return fit_solve_n<24>(m, x);
    case 6: return fit_solve_n<30>(m, x);
    case 7: return fit_solve_n<36>(m, x);
    default: return fit_solve_n<42>(m, x);
    }
}

// the reduced system from the folded S and r -> de [n];  m: RIG_SCRATCH doubles, indexed at run time;  held: bit c of a camera
// c >= 1 without a counted frame;  false: refused.  (calib_reduced_solve's scaling at side n.)
constexpr int RIG_SCRATCH = RIG_MAX_N * (RIG_MAX_N + 1) + 2 * RIG_MAX_N;
AGX_HD bool rig_reduced_solve(int n_cams, uint32_t held, const double *fold, double *m, double *de)
{
    const int n = rig_n(n_cams), W = n + 1, nt = rig_tri(n);
    double *x = m + RIG_MAX_N * (RIG_MAX_N + 1), *d = x + RIG_MAX_N;
    const auto off = [&](int i) { return ((held >> (i / 6 + 1)) & 1u) != 0u; };
    for (int i = 0; i < n; ++i) {
        d[i] = off(i) ? 1.0 : pose_sqrt(fold[rig_sym(n, i, i)]);
        if (!f64_finite(d[i]) || !(d[i] > 0.0)) return false;
    }
    int k = 0;
    for (int i = 0; i < n; ++i)
        for (int j = i; j < n; ++j, ++k) {
            m[W * i + j] = off(i) || off(j) ? (i == j ? 1.0 : 0.0) : fold[k] / d[i] / d[j];
            m[W * j + i] = m[W * i + j];
        }
    for (int i = 0; i < n; ++i) m[W * i + n] = off(i) ? 0.0 : fold[nt + i] / d[i];
    if (!rig_solve_n(n_cams, m, x)) return false;
    for (int i = 0; i < n; ++i) {
        de[i] = x[i] / d[i];
        if (!f64_finite(de[i])) return false;
    }
    return true;
}

// an instant's step: dT = z - Y dE (left to right), through pose_update;  yz: the block's Y [6][n] then z [6]
AGX_HD void rig_instant_step(Pose &t, int n, const double *yz, const double *de)
{
    double d0 = yz[6 * n], d1 = yz[6 * n + 1], d2 = yz[6 * n + 2], d3 = yz[6 * n + 3], d4 = yz[6 * n + 4], d5 = yz[6 * n + 5];
    for (int i = 0; i < n; ++i) {  // (six named sums: nothing here is indexed at run time but the block)
        const double e = de[i];
        d0 = d0 - yz[i] * e;
        d1 = d1 - yz[n + i] * e;
        d2 = d2 - yz[2 * n + i] * e;
        d3 = d3 - yz[3 * n + i] * e;
        d4 = d4 - yz[4 * n + i] * e;
        d5 = d5 - yz[5 * n + i] * e;
    }
    const double dp[6] = {d0, d1, d2, d3, d4, d5};
    pose_update(t, dp);
}

// ---- the call's state between launches -------------------------------------------------------------------------------------------
struct RigCtl {
    double ext[RIG_MAX_CAMS][12];       // the current iterate's E_c
    double ext_best[RIG_MAX_CAMS][12];  // the best iterate's
    double de[RIG_MAX_N];               // the step (apply != 0)
    double cost[CALIB_MAX_ITERATIONS + 1];
    double best_cost;
    uint32_t status;  // AGX_RIG_*
    uint32_t frozen, have, mark_best, apply;
    uint32_t best_it, it_run, n_instants_used, n_frames_used, n_corners, n_cams_free;
    uint32_t held;    // bit c: camera c >= 1 has no counted frame
    uint32_t cam_n[RIG_MAX_CAMS];
};

AGX_HD void rig_ctl_init(RigCtl &t, int n_cams, const double *ext_in)
{
    for (int c = 0; c < RIG_MAX_CAMS; ++c) {
        const bool id = c == 0 || c >= n_cams;  // (the identity)
        for (int i = 0; i < 12; ++i) t.ext_best[c][i] = t.ext[c][i] = id ? (i == 0 || i == 4 || i == 8 ? 1.0 : 0.0) : ext_in[12 * c + i];
        t.cam_n[c] = 0u;
    }
    for (int i = 0; i < RIG_MAX_N; ++i) t.de[i] = 0.0;
    for (uint32_t i = 0; i <= CALIB_MAX_ITERATIONS; ++i) t.cost[i] = calib_nan();
    t.best_cost = 0.0;
    t.status = AGX_RIG_OK;
    t.frozen = t.have = t.mark_best = t.apply = t.best_it = t.it_run = 0u;
    t.n_instants_used = t.n_frames_used = t.n_corners = t.n_cams_free = t.held = 0u;
}

// is the call refused as AGX_RIG_FEW (calib_few's shape: known once the instants are counted, before iterate 0 is folded)
AGX_HD bool rig_few(uint32_t n_instants_used, uint32_t n_cams_free, uint32_t n_corners, uint32_t min_instants)
{
    return n_instants_used < min_instants || n_instants_used == 0u || n_cams_free == 0u ||
           (uint64_t)n_corners < 6ull * n_cams_free + 6ull * n_instants_used;
}

// One lane, after iterate `it`'s instants were folded (fold [rig_fold_len]): calib_math.h's ctl_iterate on the extrinsics, the
// reduced solve, the E_c's update.
AGX_HD void rig_step(RigCtl &t, uint32_t it, uint32_t iterations, int n_cams, const double *fold, double *m)
{
    const int n = rig_n(n_cams), nt = rig_tri(n);
    if (!ctl_iterate(t, it, iterations, fold + nt + n, [&]() {
            for (int c = 0; c < n_cams; ++c)
                for (int i = 0; i < 12; ++i) t.ext_best[c][i] = t.ext[c][i];
        }))
        return;
    if (fold[nt + n + 1] != 0.0 || !rig_reduced_solve(n_cams, t.held, fold, m, t.de)) return ctl_refused(t, it, AGX_RIG_SINGULAR);
    for (int c = 1; c < n_cams; ++c) {
        if ((t.held >> c) & 1u) continue;  // (a held camera keeps its bits)
        Pose e = rig_load(t.ext[c]);
        pose_update(e, t.de + 6 * (c - 1));
        rig_store(t.ext[c], e);
    }
    t.apply = 1u;
}

// what both forms refuse in the call's own scalars
AGX_HD bool rig_args_ok(int n_cams, int n_instants, double damping, uint32_t iterations, uint32_t min_tags, uint32_t min_cams, uint32_t min_instants,
                        int flags)
{
    return n_cams >= RIG_MIN_CAMS && n_cams <= RIG_MAX_CAMS && n_instants >= 1 && (uint64_t)n_cams * (uint64_t)n_instants <= CALIB_MAX_FRAMES &&
           min_cams >= 1u && calib_args_ok(damping, iterations, min_tags, min_instants, 0u, flags);
}

// the call's report from its final state
AGX_HD void rig_report(const RigCtl &t, agx_rig_report *r)
{
    r->status = t.status;
    r->best_iter = t.best_it;
    r->iterations_run = t.it_run;
    r->n_instants_used = t.n_instants_used;
    r->n_frames_used = t.n_frames_used;
    r->n_corners = t.n_corners;
    r->n_cams_free = t.n_cams_free;
    r->reserved = 0u;
    ctl_report_iterates(t, r, AGX_RIG_FEW);
}

}  // namespace agx
