// board_fit_math.h -- the board-to-image homography through a frame's tag table, one definition each for the host form
// (host_tail.cpp: board_fit) and the kernel (board_fit.hip: k_board_fit).  Binary64, + - * / only (and one correctly rounded
// binary32 square root, the RMS), no contraction (every file that includes it is compiled with -ffp-contract=off), so both forms
// give the same bytes.  The reference has no such function; the
// corner convention is Kalibr's AprilGrid: tag id t sits at column c = (t - first_id) % cols, row r = (t - first_id) /
// cols, and corner j of its xy is the board point (c (1 + s) + ox[j], r (1 + s) + oy[j]), (ox, oy)[j] = (0,0), (1,0), (1,1),
// (0,1), in units of the tag side, s = spacing_ratio, y along increasing row.
//
// Normalisation (no reductions, so no order): board  X' = (X - Bw/2) sb,  sb = 2 / max(Bw, Bh),  Bw = cols (1 + s) - s,
// Bh = rows (1 + s) - s;  image  u' = (u - w/2) si,  si = 2 / max(w, h).
// System, h33 = 1 (w = 1 at the board's centre, tag_homography's convention): per correspondence the two rows
//   [X' Y' 1 0 0 0 -u'X' -u'Y' | u']   [0 0 0 X' Y' 1 -v'X' -v'Y' | v'].
// Sums: the 36 entries i <= j of A^T A, row by row, then the 8 of A^T b -- FIT_SUMS = 44 doubles.  THE ORDER OF SUMMATION:
// correspondence k = 4 row + j runs over the table's rows in table order; lane l of 64 adds the rows with row = l (mod 64) in
// increasing order, corners j = 0 .. 3, each correspondence as r1[i] r1[j] + r2[i] r2[j] (one addition into the sum); a row that
// is not an inlier adds nothing; the 64 partial sums are folded by the tree l ^ 32, 16, 8, 4, 2, 1 (p[l] + p[l ^ m], which is
// commutative: every lane holds the same bytes).  The host form runs the same 64 lanes one after the other.
// Solve: Gaussian elimination with partial pivoting on the 8 x 9 augmented matrix, the lowest row at equal magnitude; a pivot
// that is zero, not finite, or not above 2^-40 of the largest diagonal entry of A^T A, or a solution that is not finite, is
// AGX_FIT_SINGULAR (four coincident corners leave a pivot of rounding noise, not an exact zero).
// Projection of a board point: un = (h0 X' + h1 Y' + h2) / wn, vn likewise, wn = h6 X' + h7 Y' + 1, left to right;
// u = un / si + w/2.  wn that is not > 0: no point (a prediction is stored as NaN, NaN; a residual is +inf).
// Reported H (row major, board units -> pixels) = Ti^-1 (Hn Tb): first M = Hn Tb, then Ti^-1 M.
#pragma once
#include <cstdint>

#include "decode_math.h"

namespace agx {

constexpr int FIT_SUMS = 44;           // 36 of A^T A (i <= j) + 8 of A^T b
constexpr uint32_t FIT_MAX_ROWS = 640; // rows of one frame's table the kernel stages (TCODES: no family has more codes)
constexpr uint32_t FIT_MAX_BOARD = 4096;

struct FitGeom {
    double pitch;        // 1 + s
    double bx, by, sb;   // Bw/2, Bh/2, 2 / max(Bw, Bh)
    double ix, iy, si;   // w/2, h/2, 2 / max(w, h)
    uint32_t cols, n_board, first_id;
};

AGX_HD FitGeom fit_geom(uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, int img_w, int img_h)
{
    FitGeom g;
    const double s = (double)spacing_ratio;
    g.pitch = 1.0 + s;
    const double bw = (double)cols * g.pitch - s, bh = (double)rows * g.pitch - s;
    g.bx = bw / 2.0;
    g.by = bh / 2.0;
    g.sb = 2.0 / (bw > bh ? bw : bh);
    g.ix = (double)img_w / 2.0;
    g.iy = (double)img_h / 2.0;
    g.si = 2.0 / (double)(img_w > img_h ? img_w : img_h);
    g.cols = cols;
    g.n_board = cols * rows;
    g.first_id = first_id;
    return g;
}

// is `id` a tag of the layout (wrapping subtraction: first_id + rows cols may pass 2^32)
AGX_HD bool fit_on_board(const FitGeom &g, uint32_t id) { return id - g.first_id < g.n_board; }

// corner j of the layout's tag t (0 .. n_board - 1), normalised
AGX_HD void fit_board_point(const FitGeom &g, uint32_t t, int j, double &xn, double &yn)
{
    const uint32_t r = t / g.cols, c = t - r * g.cols;
    const double ox = (j == 1 || j == 2) ? 1.0 : 0.0, oy = j >= 2 ? 1.0 : 0.0;
    xn = ((double)c * g.pitch + ox - g.bx) * g.sb;
    yn = ((double)r * g.pitch + oy - g.by) * g.sb;
}

// one correspondence into a lane's sums
AGX_HD void fit_accumulate(double acc[FIT_SUMS], double xn, double yn, double un, double vn)
{
    const double r1[9] = {xn, yn, 1.0, 0.0, 0.0, 0.0, -(un * xn), -(un * yn), un};
    const double r2[9] = {0.0, 0.0, 0.0, xn, yn, 1.0, -(vn * xn), -(vn * yn), vn};
    int k = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = i; j < 8; ++j, ++k) acc[k] += r1[i] * r1[j] + r2[i] * r2[j];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[36 + i] += r1[i] * r1[8] + r2[i] * r2[8];
}

// the four correspondences of one table row (id on the board, corners finite) into a lane's sums
AGX_HD void fit_accumulate_row(const FitGeom &g, double acc[FIT_SUMS], uint32_t id, const float xy[8])
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double xn, yn;
        fit_board_point(g, id - g.first_id, j, xn, yn);
        fit_accumulate(acc, xn, yn, ((double)xy[2 * j] - g.ix) * g.si, ((double)xy[2 * j + 1] - g.iy) * g.si);
    }
}

// the folded sums as the augmented matrix m [8][9] (both halves of A^T A)
AGX_HD void fit_system(const double acc[FIT_SUMS], double *m)
{
    int k = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = i; j < 8; ++j, ++k) {
            m[9 * i + j] = acc[k];
            m[9 * j + i] = acc[k];
        }
#pragma unroll
    for (int i = 0; i < 8; ++i) m[9 * i + 8] = acc[36 + i];
}

// m [N][N + 1] -> h [N]; m is destroyed.  false: AGX_FIT_SINGULAR.  (m is indexed at run time: the kernels keep it in LDS)
// One statement of the elimination for the 8 x 9 system here and the 6 x 7 system of board_pose_math.h.
template <int N>
AGX_HD bool fit_solve_n(double *m, double *h)
{
    constexpr int W = N + 1;
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
            if (a > best) {  // (strictly: the lowest row stays at equal magnitude; a NaN never wins and fails below)
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
    for (int c = N - 1; c >= 0; --c) {
        double s = m[W * c + N];
        for (int j = c + 1; j < N; ++j) s = s - m[W * c + j] * h[j];
        h[c] = s / m[W * c + c];
        if (!f64_finite(h[c])) return false;
    }
    return true;
}

// m [8][9] -> h [8]: the homography's system
AGX_HD bool fit_solve(double *m, double *h) { return fit_solve_n<8>(m, h); }

// a normalised board point to pixels; false: w is not > 0 (u, v untouched)
AGX_HD bool fit_project(const FitGeom &g, const double h[8], double xn, double yn, double &u, double &v)
{
    const double wn = h[6] * xn + h[7] * yn + 1.0;
    if (!(wn > 0.0)) return false;
    u = (h[0] * xn + h[1] * yn + h[2]) / wn / g.si + g.ix;
    v = (h[3] * xn + h[4] * yn + h[5]) / wn / g.si + g.iy;
    return true;
}

// the residual of one table row under h: the largest of its four corners' (u - u^)^2 + (v - v^)^2 in pixels, binary64 rounded to
// binary32 (+inf where a corner has no projection or the value is not below +inf); *sum gets the four corners' sum in corner order
AGX_HD float fit_row_residual(const FitGeom &g, const double h[8], uint32_t id, const float xy[8], double *sum)
{
    double worst = 0.0, total = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double xn, yn, u, v, e = __builtin_inf();
        fit_board_point(g, id - g.first_id, j, xn, yn);
        if (fit_project(g, h, xn, yn, u, v)) {
            const double du = (double)xy[2 * j] - u, dv = (double)xy[2 * j + 1] - v;
            e = du * du + dv * dv;
            if (!(e < __builtin_inf())) e = __builtin_inf();
        }
        total += e;
        if (e > worst) worst = e;
    }
    *sum = total;
    return (float)worst;
}

// the predicted corners of the layout's tag t, rounded to binary32; NaN, NaN where w is not > 0
AGX_HD void fit_predict(const FitGeom &g, const double h[8], uint32_t t, float xy[8])
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double xn, yn, u, v;
        fit_board_point(g, t, j, xn, yn);
        if (fit_project(g, h, xn, yn, u, v)) {
            xy[2 * j] = (float)u;
            xy[2 * j + 1] = (float)v;
        } else {
            xy[2 * j] = xy[2 * j + 1] = f32_from_bits(0x7fc00000u);
        }
    }
}

// H = Ti^-1 (Hn Tb), row major, board units -> pixels
AGX_HD void fit_h_matrix(const FitGeom &g, const double h[8], double H[9])
{
    // M = Hn Tb, Tb = [sb 0 -sb bx; 0 sb -sb by; 0 0 1]
    double M[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double a = h[3 * r], b = h[3 * r + 1], c = r < 2 ? h[3 * r + 2] : 1.0;
        M[3 * r] = a * g.sb;
        M[3 * r + 1] = b * g.sb;
        M[3 * r + 2] = c - (a * g.sb * g.bx + b * g.sb * g.by);
    }
    // Ti^-1 = [1/si 0 ix; 0 1/si iy; 0 0 1]
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        H[j] = M[j] / g.si + g.ix * M[6 + j];
        H[3 + j] = M[3 + j] / g.si + g.iy * M[6 + j];
        H[6 + j] = M[6 + j];
    }
}

// the frame's RMS reprojection error from the folded sum of squared corner errors over the inliers
AGX_HD float fit_rms(double sum_sq, uint32_t n_inliers)
{
    return __builtin_sqrtf((float)(sum_sq / (4.0 * (double)n_inliers)));
}

}  // namespace agx
