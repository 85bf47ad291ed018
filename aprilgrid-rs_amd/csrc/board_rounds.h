// board_rounds.h -- the outlier rounds over one frame's tag table as the host forms run them (host_tail.cpp: board_fit, board_pose),
// one text for every fitter, and the one check of a fitter's argument record.  A fitter is a model: what it fits to the inlier
// rows, the residual of a row under the fit and the predicted corners of a tag of the layout.  Everything else is here.  The
// kernels (board_fit.hip, board_pose.hip) state the same rounds for a wave of 64 lanes and give the same bytes.
// The rounds.  Rows whose id is not on the board are AGX_FIT_ROW_OFF_BOARD and take no part; an inlier row with a corner that is
// not finite, a table longer than its capacity or FIT_MAX_ROWS, or a status word that is not AGX_TAGS_OK is AGX_FIT_INPUT.  The
// model's seed(), once.  Then a round: fewer inliers than min_tags is AGX_FIT_FEW; the model's fit() (false: AGX_FIT_SINGULAR);
// every inlier row's residual, the worst being the largest residual, the lowest row at equal bits; while the worst is above
// max_err_sq and fewer than max_drop rows were dropped it becomes AGX_FIT_ROW_OUTLIER and the round is run again, else the
// frame is AGX_FIT_LOOSE or AGX_FIT_OK.  A refused frame (FEW, SINGULAR, INPUT) gets n_inliers = n_pred = 0 and its status,
// nothing else.  Otherwise row_status of every row, err_sq of every row on the board, the model's result, n_inliers, rms, and
// the predicted corners of the layout's tags in id order -- under AGX_FIT_PREDICT_MISSING only of the tags that are no inlier row.
// THE ORDER OF SUMMATION (board_fit_math.h): lane l of 64 adds the inlier rows l, l + 64, ... in increasing order into its own
// sums; the 64 partial sums are folded by the tree l ^ 32, 16, 8, 4, 2, 1, sums k ascending inside.  The kernels do it by
// shuffles, RoundsHost runs the same 64 lanes one after the other.
// A model fits through RoundsHost, the kernel's wave on the host,
//   w.sums<N>(acc, add)      acc[0 .. N) = the folded sums of add(lane's acc, id, xy) over the inlier rows
//   w.solve<K>(out, system)  system(m, sol) builds and solves in m; out[0 .. K) = sol; -> what system returned
// and has seed(w, n_inl, min_tags) -> AGX_FIT_*, fit(w) -> bool, residual(id, xy, &sum), predict(t, xy) and store(b, f).
#pragma once
#include <cstdint>
#include <memory>
#include <vector>

#include "board_fit.h"
#include "board_fit_math.h"
#include "board_pose.h"
#include "board_pose_math.h"

namespace agx {

// What every fitter's entry points and its launch refuse in a record (BoardFitArgs, BoardPoseArgs): the rule's text, or null.
// result is the record's binary64 output, more its other output (result again where there is none), own the rule that the
// fitter's own scalars break, or null.  device: the kernel's record -- every array but tag_status, n_frames and tags_per_frame
// > 0; else the host form's, which reads frame 0: tags, err_sq and row_status may be null while n_tags[0] == 0.
template <class Args>
const char *rounds_args_bad(const Args &b, bool device, const double *result, const void *more, const char *own)
{
    if (!result || !more || !b.n_tags || !b.n_inliers || !b.rms || !b.pred || !b.n_pred || !b.status || (device && (b.n_frames <= 0 || !b.tags_per_frame)))
        return "a null array, n_frames <= 0 or tags_per_frame == 0";
    if ((device || b.n_tags[0]) && (!b.tags || !b.err_sq || !b.row_status)) return "a null array of tag rows";
    if (!b.cols || !b.rows || (uint64_t)b.cols * b.rows > FIT_MAX_BOARD || !f32_finite(b.spacing_ratio) || !(b.spacing_ratio > -1.0f) ||
        !(b.max_err_sq >= 0.0f) || !b.min_tags || (b.flags & ~AGX_FIT_PREDICT_MISSING))  // (a NaN fails the comparisons)
        return "rows * cols in 1 .. 4096, spacing_ratio finite and > -1, max_err_sq >= 0, min_tags >= 1, flags AGX_FIT_PREDICT_MISSING or 0";
    if (own) return own;
    if ((((uintptr_t)b.tags | (uintptr_t)b.n_tags | (uintptr_t)b.tag_status | (uintptr_t)b.err_sq | (uintptr_t)b.row_status | (uintptr_t)b.n_inliers |
          (uintptr_t)b.rms | (uintptr_t)more | (uintptr_t)b.pred | (uintptr_t)b.n_pred | (uintptr_t)b.status) & 3) || ((uintptr_t)result & 7))
        return "the binary64 array must be 8-byte aligned, every other array 4-byte aligned";
    if ((uint64_t)b.n_frames * b.tags_per_frame >= (1ull << 27)) return "at most 2^27 - 1 tag rows per batch";
    return nullptr;
}

// ---- the kernel's wave on the host: what a model fits through ----------------------------------------------------------------------
struct RoundsHost {
    const agx_tag *tags;
    uint32_t n_tags;
    std::vector<uint8_t> st;  // AGX_FIT_ROW_*
    std::unique_ptr<double[][FIT_SUMS]> lanes{new double[64][FIT_SUMS]};  // the kernel's 64 lanes one after the other

    // the fold is p[l] + p[l ^ m] over m = 32 .. 1, of which lane 0's value needs p[l] += p[l + m] for l < m only
    void fold(int n)
    {
        for (int m = 32; m >= 1; m >>= 1)
            for (int l = 0; l < m; ++l)
                for (int k = 0; k < n; ++k) lanes[l][k] = lanes[l][k] + lanes[l + m][k];
    }
    template <int N, class Add>
    void sums(double acc[N], Add add)
    {
        static_assert(N <= FIT_SUMS, "the lanes' sums share board_fit's rows");
        for (int l = 0; l < 64; ++l) {
            for (int k = 0; k < N; ++k) lanes[l][k] = 0.0;
            for (uint32_t r = (uint32_t)l; r < n_tags; r += 64u)
                if (st[r] == AGX_FIT_ROW_INLIER) add(lanes[l], tags[r].id, tags[r].xy);
        }
        fold(N);
        for (int k = 0; k < N; ++k) acc[k] = lanes[0][k];
    }
    template <int K, class System>
    bool solve(double out[K], System system)
    {
        double m[72], sol[8];
        if (!system(m, sol)) return false;
        for (int i = 0; i < K; ++i) out[i] = sol[i];
        return true;
    }
};

// ---- the two models -----------------------------------------------------------------------------------------------------------------
// the homography of board_fit_math.h: no seed, one linear fit a round
struct FitModel {
    const FitGeom &g;
    double h[8] = {0, 0, 0, 0, 0, 0, 0, 0};

    uint32_t seed(RoundsHost &, uint32_t, uint32_t)
    {
        return AGX_FIT_OK;
    }
    bool fit(RoundsHost &w)
    {
        double acc[FIT_SUMS];
        w.sums<FIT_SUMS>(acc, [&](double *a, uint32_t id, const float *xy) { fit_accumulate_row(g, a, id, xy); });
        return w.solve<8>(h, [&](double *m, double *sol) {
            fit_system(acc, m);
            return fit_solve(m, sol);
        });
    }
    float residual(uint32_t id, const float xy[8], double *sum) const { return fit_row_residual(g, h, id, xy, sum); }
    void predict(uint32_t t, float xy[8]) const { fit_predict(g, h, t, xy); }
    void store(const BoardFitArgs &b, uint32_t f) const
    {
        double H[9];
        fit_h_matrix(g, h, H);
        for (int i = 0; i < 9; ++i) b.h[(size_t)f * 9u + i] = H[i];
    }
};

// the pose of board_pose_math.h under the lens model LENS: a homography seed through the undistorted corners, then per round
// Gauss-Newton iterates from the last round's answer with the best iterate kept.  b.camera is pose_camera()'s.
template <int LENS>
struct PoseModel {
    const BoardPoseArgs &b;
    const FitGeom &g;
    double *iter_sums;  // null or [iterations + 1]: the last round's sums of |e|^2 (agx_debug_board_pose_sums)
    Pose pose = {{0, 0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0}};
    uint32_t best_it = 0;

    uint32_t seed(RoundsHost &w, uint32_t n_inl, uint32_t min_tags)
    {
        if (n_inl < min_tags) return AGX_FIT_FEW;
        double acc[FIT_SUMS], h[8];
        w.sums<FIT_SUMS>(acc, [&](double *a, uint32_t id, const float *xy) { pose_seed_accumulate_row<LENS>(g, b.camera, a, id, xy); });
        const bool solved = w.solve<8>(h, [&](double *m, double *sol) {
            fit_system(acc, m);
            return fit_solve(m, sol);
        });
        return solved && pose_from_homography(g, b.tag_size, h, pose) ? AGX_FIT_OK : AGX_FIT_SINGULAR;
    }
    bool fit(RoundsHost &w)
    {
        Pose cur = pose;
        double best_cost = 0.0;
        bool have = false;
        best_it = 0;
        if (iter_sums)
            for (uint32_t i = 0; i <= b.iterations; ++i) iter_sums[i] = __builtin_nan("");
        for (uint32_t it = 0;; ++it) {
            double acc[POSE_SUMS], d[6];
            w.sums<POSE_SUMS>(acc, [&](double *a, uint32_t id, const float *xy) { pose_accumulate_row<LENS>(g, b.tag_size, b.camera, cur, a, id, xy); });
            if (iter_sums) iter_sums[it] = acc[27];
            if (pose_better(acc[27], have, best_cost)) {
                pose = cur;
                best_cost = acc[27];
                best_it = it;
                have = true;
            }
            if (it == b.iterations) break;  // (the last iterate's pass gave its sum of |e|^2 only)
            const bool solved = w.solve<6>(d, [&](double *m, double *sol) {
                pose_system(acc, m);
                return fit_solve_n<6>(m, sol);
            });
            if (!solved) {
                if (it == 0) return false;
                break;
            }
            pose_update(cur, d);
        }
        return pose_gram_schmidt(pose.R);
    }
    float residual(uint32_t id, const float xy[8], double *sum) const { return pose_row_residual<LENS>(g, b.tag_size, b.camera, pose, id, xy, sum); }
    void predict(uint32_t t, float xy[8]) const { pose_predict<LENS>(g, b.tag_size, b.camera, pose, t, xy); }
    void store(const BoardPoseArgs &o, uint32_t f) const
    {
        for (int i = 0; i < 9; ++i) o.pose[(size_t)f * 12u + i] = pose.R[i];
        for (int i = 0; i < 3; ++i) o.pose[(size_t)f * 12u + 9u + i] = pose.t[i];
        o.best_iter[f] = best_it;
    }
};

// ---- the rounds: frame 0 of b, whose pointers are host pointers --------------------------------------------------------------------
// -> AGX_FIT_*, which the caller stores
template <class Args, class Model>
uint32_t board_rounds_host(const Args &b, const FitGeom &g, Model &m)
{
    const uint32_t n_tags = b.n_tags[0];
    const auto refuse = [&](uint32_t status) {
        b.n_inliers[0] = 0;
        b.n_pred[0] = 0;
        return status;
    };
    if (n_tags > b.tags_per_frame || n_tags > FIT_MAX_ROWS || (b.tag_status && b.tag_status[0] != AGX_TAGS_OK)) return refuse(AGX_FIT_INPUT);
    RoundsHost w{b.tags, n_tags, std::vector<uint8_t>(n_tags)};
    const agx_tag *tags = b.tags;
    uint32_t n_inl = 0;
    for (uint32_t r = 0; r < n_tags; ++r) {
        w.st[r] = AGX_FIT_ROW_OFF_BOARD;
        if (!fit_on_board(g, tags[r].id)) continue;
        for (int j = 0; j < 8; ++j)
            if (!f32_finite(tags[r].xy[j])) return refuse(AGX_FIT_INPUT);
        w.st[r] = AGX_FIT_ROW_INLIER;
        ++n_inl;
    }
    uint32_t status = m.seed(w, n_inl, b.min_tags), drops = 0;
    if (status != AGX_FIT_OK) return refuse(status);
    double sum_sq = 0.0;
    for (;;) {  // a round
        if (n_inl < b.min_tags) return refuse(AGX_FIT_FEW);
        if (!m.fit(w)) return refuse(AGX_FIT_SINGULAR);
        float worst = 0.0f;
        uint32_t worst_row = 0xffffffffu;
        for (int l = 0; l < 64; ++l) {
            w.lanes[l][0] = 0.0;
            for (uint32_t r = (uint32_t)l; r < n_tags; r += 64u) {
                if (w.st[r] != AGX_FIT_ROW_INLIER) continue;
                double sum;
                const float e = m.residual(tags[r].id, tags[r].xy, &sum);
                w.lanes[l][0] += sum;
                if (worst_row == 0xffffffffu || e > worst || (e == worst && r < worst_row)) {  // the lowest row at equal residual
                    worst = e;
                    worst_row = r;
                }
            }
        }
        if (worst > b.max_err_sq) {
            if (drops < b.max_drop) {
                w.st[worst_row] = AGX_FIT_ROW_OUTLIER;
                ++drops;
                --n_inl;
                continue;
            }
            status = AGX_FIT_LOOSE;
        }
        w.fold(1);
        sum_sq = w.lanes[0][0];
        break;
    }
    for (uint32_t r = 0; r < n_tags; ++r) {
        b.row_status[r] = w.st[r];
        double sum;
        if (w.st[r] != AGX_FIT_ROW_OFF_BOARD) b.err_sq[r] = m.residual(tags[r].id, tags[r].xy, &sum);
    }
    m.store(b, 0);
    b.n_inliers[0] = n_inl;
    b.rms[0] = fit_rms(sum_sq, n_inl);
    std::vector<bool> member(g.n_board, false);
    if (b.flags & AGX_FIT_PREDICT_MISSING)
        for (uint32_t r = 0; r < n_tags; ++r)
            if (w.st[r] == AGX_FIT_ROW_INLIER) member[tags[r].id - g.first_id] = true;
    uint32_t kept = 0;
    for (uint32_t t = 0; t < g.n_board; ++t) {
        if (member[t]) continue;
        b.pred[kept].id = g.first_id + t;
        m.predict(t, b.pred[kept].xy);
        ++kept;
    }
    b.n_pred[0] = kept;
    return status;
}

}  // namespace agx
