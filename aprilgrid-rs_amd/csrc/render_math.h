// render_math.h -- the printed board as a camera at a given pose sees it: a sensor pixel's samples back to the board's plane, what
// is printed there, and the pixel's value.  One definition each for the kernel (render.hip: k_render_boards) and the host form
// (render.hip: render_boards_host), so both give the same bytes.  Binary64, + - * / and pose_sqrt only, no contraction (every
// file that includes it is compiled with -ffp-contract=off); nothing after the classification of a sample is floating point.
// The reference draws the board flat (scripts/generate_aprilgrid.py); it has no camera.
//
// The forward model is board_pose_math.h's pose_project<LENS> and nothing else.  A sample (u, v) is inverted, THE ORDER OF
// OPERATIONS:
//   ray d: under AGX_LENS_RADTAN and AGX_LENS_EQUIDISTANT (x, y, 1) of pose_undistort<LENS>(u, v); under AGX_LENS_DOUBLE_SPHERE the
//     closed-form unprojection's (sc x0, sc y0, sc mz - xi) itself (pose_undistort_ds's statements up to there: the ray may point
//     behind the image plane), and pose_undistort_ds's clamped (x, y, 1) where the pixel is outside the unprojection's domain or
//     a component is not finite;
//   the ray's point in the board's plane: n = column 2 of R,  nd = n . d,  nt = n . t,  lambda = nt / nd,  P = lambda d - t,
//     X = (column 0 of R) . P,  Y = (column 1 of R) . P   (every dot product left to right);
//   RENDER_NEWTON_STEPS times, no early exit: q = pose_project<LENS>(X, Y) (none: the sample is background), e = (u, v) - q,
//     m = d(u, v) / d(Xc, Yc, Zc) by pose_accumulate's statements, J = m [c0 c1] (2 x 2), det = j00 j11 - j01 j10,
//     X = X + (j11 e0 - j01 e1) / det,  Y = Y + (j00 e1 - j10 e0) / det;
//   acceptance: q = pose_project<LENS>(X, Y) exists and |(u, v) - q|^2 <= RENDER_RESIDUAL_SQ (2^-40 px^2: a millionth of a
//     pixel), and (X, Y) lies on the page.  Whatever the seed was -- clamped or not -- only this test decides.
// The page, in tag sides from the outer squares' corner: xs = X / tag_size + Bw/2 + s,  ys likewise;  Ws = cols (1 + s) + s,
//   Hs = rows (1 + s) + s.  On the page: -margin <= xs <= Ws + margin and the same in y.  Outside [0, Ws) x [0, Hs): white.
//   i = floor(xs / (1 + s)),  fx = xs - i (1 + s), the same in y (j, fy):  fx < s and fy < s: a black square (one at every lattice
//   point, the outer ring included);  fx >= s, fy >= s, i < cols, j < rows: tag j cols + i;  else white.
//   Inside a tag with n = edge + 2 border cells a side:  cx = floor((fx - s) n),  cy = floor((fy - s) n), both clamped to
//   0 .. n - 1;  the tag's rows are printed from Y's high end (Kalibr's board has y up): row = n - 1 - cy.  A border cell is
//   black; code cell (row - border, cx - border) is bit edge^2 - 1 - ((row - border) edge + cx - border) of the code, 1 = white.
// The pixel (i, j) takes S x S samples at (i + ox[a], j + ox[b]),  ox[a] = (a + 1/2) / S - 1/2, rows b outer;  value =
//   (n_w white + n_b black + n_bg bg + S S / 2) / (S S) in uint32.
// Per frame, before its first store: a pose entry that is not finite, or two columns of R whose dot product is further than
// RENDER_ORTHO_TOL (2^-20) from 1 (a column with itself) or 0: AGX_RENDER_INPUT;  none of the page-less board's four outer
// corners (+-(Ws / 2) tag_size, +-(Hs / 2) tag_size) projects: AGX_RENDER_EMPTY.
#pragma once
#include <cstdint>

#include "../../include/aprilgrid_amd.h"
#include "board_pose_math.h"

namespace agx {

constexpr int RENDER_NEWTON_STEPS = 4;
constexpr double RENDER_RESIDUAL_SQ = 0x1p-40;
constexpr double RENDER_ORTHO_TOL = 0x1p-20;
constexpr int RENDER_MAX_SUPERSAMPLE = 4;
constexpr uint32_t RENDER_MAX_CODES = 640;  // codes of one layout staged in LDS (no family has more)
constexpr int RENDER_MAX_SIDE = 16384;

enum RenderSample { RENDER_BG = 0, RENDER_WHITE = 1, RENDER_BLACK = 2 };

struct RenderGeom {
    FitGeom g;       // pose_geom's
    agx_camera cam;  // pose_camera's
    double tag_size, s, margin;
    double ws, hs;   // the board with its outer squares, in tag sides
    int edge, border;
    int S;
    uint32_t black, white, background;
    int flags;
};

inline RenderGeom render_geom(int lens, const agx_camera &cam, uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, double tag_size,
                              int edge, int border, const agx_render_params &p)
{
    RenderGeom r;
    r.g = pose_geom(cols, rows, first_id, spacing_ratio);
    r.cam = pose_camera(lens, cam);
    r.tag_size = tag_size;
    r.s = (double)spacing_ratio;
    r.margin = (double)p.page_margin;
    r.ws = (double)cols * r.g.pitch + r.s;
    r.hs = (double)rows * r.g.pitch + r.s;
    r.edge = edge;
    r.border = border;
    r.S = (int)p.supersample;
    r.black = p.black;
    r.white = p.white;
    r.background = p.background;
    r.flags = (int)p.flags;
    return r;
}

// the sample's ray in the camera frame (not normalised)
template <int LENS>
AGX_HD void render_ray(const agx_camera &c, double u, double v, double d[3])
{
    if constexpr (LENS == AGX_LENS_DOUBLE_SPHERE) {
        const double xi = c.k1, al = c.k2;
        const double x0 = (u - c.cx) / c.fx, y0 = (v - c.cy) / c.fy;
        const double r2 = x0 * x0 + y0 * y0;
        const double t = 1.0 - (2.0 * al - 1.0) * r2;
        const double mz = (1.0 - al * al * r2) / (al * pose_sqrt(t) + (1.0 - al));
        const double n = mz * mz + r2;
        const double sc = (mz * xi + pose_sqrt(mz * mz + (1.0 - xi * xi) * r2)) / n;
        d[0] = sc * x0;
        d[1] = sc * y0;
        d[2] = sc * mz - xi;
        if (t >= 0.0 && f64_finite(d[0]) && f64_finite(d[1]) && f64_finite(d[2])) return;
    }
    pose_undistort<LENS>(c, u, v, d[0], d[1]);
    d[2] = 1.0;
}

// d(u, v) / d(Xc, Yc, Zc) at a projected point: pose_accumulate's statements
template <int LENS>
AGX_HD void render_point_jacobian(const agx_camera &c, const PosePointOf<LENS> &q, double m[6])
{
    if constexpr (LENS == AGX_LENS_DOUBLE_SPHERE) {
        pose_ds_jacobian(c, q, m[0], m[1], m[2], m[3], m[4], m[5]);
    } else {
        const double x = q.x, y = q.y;
        double d00, d01, d10, d11;
        pose_lens_jacobian(c, q, d00, d01, d10, d11);
        m[0] = c.fx * d00 / q.zc, m[1] = c.fx * d01 / q.zc, m[2] = -(m[0] * x + m[1] * y);
        m[3] = c.fy * d10 / q.zc, m[4] = c.fy * d11 / q.zc, m[5] = -(m[3] * x + m[4] * y);
    }
}

// the board point whose forward projection is (u, v); false: there is none within the residual
template <int LENS>
AGX_HD bool render_invert(const agx_camera &c, const Pose &p, double u, double v, double &X, double &Y)
{
    double d[3];
    render_ray<LENS>(c, u, v, d);
    const double nd = p.R[2] * d[0] + p.R[5] * d[1] + p.R[8] * d[2];
    const double nt = p.R[2] * p.t[0] + p.R[5] * p.t[1] + p.R[8] * p.t[2];
    const double lam = nt / nd;
    const double p0 = lam * d[0] - p.t[0], p1 = lam * d[1] - p.t[1], p2 = lam * d[2] - p.t[2];
    X = p.R[0] * p0 + p.R[3] * p1 + p.R[6] * p2;
    Y = p.R[1] * p0 + p.R[4] * p1 + p.R[7] * p2;
    PosePointOf<LENS> q;
#pragma unroll 1
    for (int i = 0; i < RENDER_NEWTON_STEPS; ++i) {
        if (!pose_project<LENS>(c, p, X, Y, q)) return false;
        const double e0 = u - q.u, e1 = v - q.v;
        double m[6];
        render_point_jacobian<LENS>(c, q, m);
        const double j00 = m[0] * p.R[0] + m[1] * p.R[3] + m[2] * p.R[6], j01 = m[0] * p.R[1] + m[1] * p.R[4] + m[2] * p.R[7];
        const double j10 = m[3] * p.R[0] + m[4] * p.R[3] + m[5] * p.R[6], j11 = m[3] * p.R[1] + m[4] * p.R[4] + m[5] * p.R[7];
        const double det = j00 * j11 - j01 * j10;
        X = X + (j11 * e0 - j01 * e1) / det;
        Y = Y + (j00 * e1 - j10 * e0) / det;
    }
    if (!pose_project<LENS>(c, p, X, Y, q)) return false;
    const double e0 = u - q.u, e1 = v - q.v;
    return e0 * e0 + e1 * e1 <= RENDER_RESIDUAL_SQ;  // (a value that is not a number fails)
}

// what is printed at the board point (X, Y); codes[t]: the code of the layout's tag t
AGX_HD int render_board_at(const RenderGeom &r, const uint64_t *codes, double X, double Y)
{
    const double xs = X / r.tag_size + r.g.bx + r.s, ys = Y / r.tag_size + r.g.by + r.s;
    if (!(xs >= -r.margin && xs <= r.ws + r.margin && ys >= -r.margin && ys <= r.hs + r.margin)) return RENDER_BG;
    if (!(xs >= 0.0 && xs < r.ws && ys >= 0.0 && ys < r.hs)) return RENDER_WHITE;
    const double fi = __builtin_floor(xs / r.g.pitch), fj = __builtin_floor(ys / r.g.pitch);
    const double fx = xs - fi * r.g.pitch, fy = ys - fj * r.g.pitch;
    if (fx < r.s && fy < r.s) return RENDER_BLACK;
    const uint32_t i = (uint32_t)fi, j = (uint32_t)fj, rows = r.g.n_board / r.g.cols;
    if (!(fx >= r.s && fy >= r.s && i < r.g.cols && j < rows)) return RENDER_WHITE;
    const int n = r.edge + 2 * r.border;
    int cx = (int)__builtin_floor((fx - r.s) * (double)n), cy = (int)__builtin_floor((fy - r.s) * (double)n);
    cx = cx < 0 ? 0 : cx > n - 1 ? n - 1 : cx;
    cy = cy < 0 ? 0 : cy > n - 1 ? n - 1 : cy;
    const int col = cx - r.border, row = n - 1 - cy - r.border;
    if (col < 0 || col >= r.edge || row < 0 || row >= r.edge) return RENDER_BLACK;
    const uint64_t code = codes[j * r.g.cols + i];
    return (code >> (r.edge * r.edge - 1 - (row * r.edge + col))) & 1u ? RENDER_WHITE : RENDER_BLACK;
}

// the S x S samples of pixel (px, py): how many are white, how many black
template <int LENS>
AGX_HD void render_pixel(const RenderGeom &r, const Pose &p, const uint64_t *codes, uint32_t px, uint32_t py, uint32_t &n_w, uint32_t &n_b)
{
    n_w = n_b = 0;
#pragma unroll 1
    for (int b = 0; b < r.S; ++b) {
        const double v = (double)py + (((double)b + 0.5) / (double)r.S - 0.5);
#pragma unroll 1
        for (int a = 0; a < r.S; ++a) {
            const double u = (double)px + (((double)a + 0.5) / (double)r.S - 0.5);
            double X, Y;
            if (!render_invert<LENS>(r.cam, p, u, v, X, Y)) continue;
            const int what = render_board_at(r, codes, X, Y);
            n_w += what == RENDER_WHITE;
            n_b += what == RENDER_BLACK;
        }
    }
}

AGX_HD uint32_t render_shade(const RenderGeom &r, uint32_t n_w, uint32_t n_b, uint32_t bg)
{
    const uint32_t ss = (uint32_t)(r.S * r.S);
    return (n_w * r.white + n_b * r.black + (ss - n_w - n_b) * bg + ss / 2u) / ss;
}

// AGX_RENDER_* of one frame's pose
template <int LENS>
AGX_HD uint32_t render_frame_status(const RenderGeom &r, const Pose &p)
{
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) finite = finite && f64_finite(p.R[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) finite = finite && f64_finite(p.t[i]);
    if (!finite) return AGX_RENDER_INPUT;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) {
            const double dot = p.R[i] * p.R[j] + p.R[3 + i] * p.R[3 + j] + p.R[6 + i] * p.R[6 + j];
            const double off = dot - (i == j ? 1.0 : 0.0);
            if (!(off <= RENDER_ORTHO_TOL && off >= -RENDER_ORTHO_TOL)) return AGX_RENDER_INPUT;
        }
    const double hx = r.ws / 2.0 * r.tag_size, hy = r.hs / 2.0 * r.tag_size;
    bool any = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        PosePointOf<LENS> q;
        any = pose_project<LENS>(r.cam, p, (k == 1 || k == 2) ? hx : -hx, k >= 2 ? hy : -hy, q) || any;
    }
    return any ? AGX_RENDER_OK : AGX_RENDER_EMPTY;
}

}  // namespace agx
