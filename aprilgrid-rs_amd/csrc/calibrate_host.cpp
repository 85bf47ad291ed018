// calibrate_host.cpp -- the host forms of calibrate.hip (agx_calibrate_tail): the launches of k_calib_blocks and k_calib_solve
// one after the other, a wave's 64 lanes one after the other, every number calib_math.h's -- the same bytes.  And the two host-only
// pieces: the closed-form seed (agx_calibrate_seed_tail) and the parameter Jacobian for tests (agx_debug_calib_param_jacobian).
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "calib_math.h"
#include "calibrate.h"

namespace agx {
namespace {

// the kernels' fold: p[l] + p[l ^ m] over m = 32 .. 1, of which lane 0's value needs p[l] += p[l + m] for l < m only
template <int N>
void calib_fold(double (*lanes)[N])
{
    for (int m = 32; m >= 1; m >>= 1)
        for (int l = 0; l < m; ++l)
            for (int k = 0; k < N; ++k) lanes[l][k] = lanes[l][k] + lanes[l + m][k];
}

template <int LENS, int PART>
void calib_pass_host(const agx_tag *tags, const uint8_t *st, uint32_t cnt, const FitGeom &g, double tag_size, const agx_camera &cam, const Pose &pose,
                     double *acc)
{
    constexpr int N = CALIB_PART_SUMS[PART];
    std::unique_ptr<double[][N]> lanes(new double[64][N]);
    for (int l = 0; l < 64; ++l) {
        for (int k = 0; k < N; ++k) lanes[l][k] = 0.0;
        for (uint32_t r = (uint32_t)l; r < cnt; r += 64u)
            if (st[r]) calib_accumulate_row<LENS, PART>(g, tag_size, cam, pose, lanes[l], tags[r].id, tags[r].xy);
    }
    calib_fold<N>(lanes.get());
    for (int k = 0; k < N; ++k) acc[k] = lanes[0][k];
}

template <int LENS>
void calibrate_lens(const CalibArgs &a)
{
    const size_t n = (size_t)a.n_frames;
    std::vector<char> mem(calib_work_bytes(a.n_frames) + 8);
    const CalibWork w = calib_work(mem.data() + ((8 - ((uintptr_t)mem.data() & 7)) & 7), a.n_frames);
    CalibCtl &t = *w.ctl;
    const FitGeom g = pose_geom(a.cols, a.rows, a.first_id, a.spacing_ratio);
    const uint32_t held = calib_held(LENS, a.fixed_mask);
    std::vector<uint8_t> st(FIT_MAX_ROWS);

    const auto blocks = [&](uint32_t it, bool finish) {  // k_calib_blocks<LENS>(it, finish)
        for (size_t f = 0; f < n; ++f) {
            double *blk = w.blocks + f * CALIB_BLOCK;
            if (it > 0u || finish) {
                const uint32_t corners = w.corners[f];
                if (t.mark_best && corners) {
                    std::memcpy(w.pose_best + f * 12, w.pose_cur + f * 12, 12 * sizeof(double));
                    w.cost_best[f] = blk[54];
                }
                if (finish) {
                    if (t.status == AGX_CALIB_OK) {
                        if (corners) std::memcpy(a.pose + f * 12, w.pose_best + f * 12, 12 * sizeof(double));
                        a.frame_cost[f] = corners ? (float)w.cost_best[f] : 0.0f;
                        a.frame_n[f] = corners;
                    }
                    continue;
                }
                if (t.frozen || !corners) continue;
            }
            const uint32_t cnt = a.n_tags[f];
            const size_t row0 = f * a.tags_per_frame;
            if (it == 0u) {
                const bool ok = calib_frame_ok(a.fit_status[f], a.flags) && cnt <= a.tags_per_frame && cnt <= FIT_MAX_ROWS && !(a.tag_status && a.tag_status[f] != AGX_TAGS_OK);
                uint32_t n_inl = 0;
                if (ok)
                    for (uint32_t r = 0; r < cnt; ++r) n_inl += calib_row_counts(g, a.tags[row0 + r].id, a.row_status[row0 + r]) ? 1u : 0u;
                const uint32_t corners = ok && n_inl >= a.min_tags ? 4u * n_inl : 0u;
                w.corners[f] = corners;
                if (!corners) continue;
                std::memcpy(w.pose_cur + f * 12, a.pose_in + f * 12, 12 * sizeof(double));
                std::memcpy(w.pose_best + f * 12, a.pose_in + f * 12, 12 * sizeof(double));
            }
            for (uint32_t r = 0; r < cnt; ++r) st[r] = calib_row_counts(g, a.tags[row0 + r].id, a.row_status[row0 + r]) ? 1 : 0;
            Pose pose;
            const double *pin = w.pose_cur + f * 12;
            for (int i = 0; i < 9; ++i) pose.R[i] = pin[i];
            for (int i = 0; i < 3; ++i) pose.t[i] = pin[9 + i];
            agx_camera cam = a.camera;
            if (it > 0u) {
                cam = calib_camera(t.cam);
                if (t.apply) {
                    calib_pose_step(pose, blk + CALIB_FOLD, t.dc);
                    for (int i = 0; i < 9; ++i) w.pose_cur[f * 12 + i] = pose.R[i];
                    for (int i = 0; i < 3; ++i) w.pose_cur[f * 12 + 9 + i] = pose.t[i];
                }
            }
            cam = pose_camera(LENS, cam);
            CalibFrameSys sys;
            double acc[CALIB_PART_SUMS[0]];  // (the largest part)
            calib_pass_host<LENS, 0>(a.tags + row0, st.data(), cnt, g, a.tag_size, cam, pose, acc);
            const double cost = acc[45];
            calib_frame_system_u(acc, a.damping, held, sys);
            calib_pass_host<LENS, 1>(a.tags + row0, st.data(), cnt, g, a.tag_size, cam, pose, acc);
            calib_frame_system_w(acc, 0, CALIB_W_SPLIT, held, sys);
            calib_pass_host<LENS, 2>(a.tags + row0, st.data(), cnt, g, a.tag_size, cam, pose, acc);
            calib_frame_system_w(acc, CALIB_W_SPLIT, CALIB_CAM, held, sys);
            calib_pass_host<LENS, 3>(a.tags + row0, st.data(), cnt, g, a.tag_size, cam, pose, acc);
            calib_frame_system_v(acc, a.damping, sys);
            const bool solved = fit_solve_multi<6, 10>(sys.m, sys.x);
            for (int e = 0; e < 54; ++e) blk[e] = solved ? calib_schur_entry(sys, e) : 0.0;
            blk[54] = cost;
            blk[55] = solved ? 0.0 : 1.0;
            for (uint32_t e = 0; e < 60u; ++e) {
                const uint32_t k = e / 10u, j = e - 10u * k;
                blk[CALIB_FOLD + (j < 9u ? 9u * k + j : 54u + k)] = solved ? sys.x[e] : 0.0;
            }
        }
        if (finish) {
            if (t.status == AGX_CALIB_OK)
                for (int i = 0; i < 9; ++i) a.camera_out[i] = t.cam_best[i];
            calib_report(t, a.report);
        }
    };

    std::unique_ptr<double[][CALIB_FOLD]> lanes(new double[64][CALIB_FOLD]);
    const auto solve = [&](uint32_t it) {  // k_calib_solve(it)
        if (it == 0u) {
            uint32_t base = 0, corners = 0;
            for (size_t f = 0; f < n; ++f)
                if (w.corners[f]) {
                    w.list[base++] = (uint32_t)f;
                    corners += w.corners[f];
                }
            const double c9[9] = {a.camera.fx, a.camera.fy, a.camera.cx, a.camera.cy, a.camera.k1, a.camera.k2, a.camera.p1, a.camera.p2, a.camera.k3};
            calib_ctl_init(t, c9);
            t.n_usable = base;
            t.n_corners = corners;
            if (calib_few(base, corners, a.min_frames, held)) t.status = AGX_CALIB_FEW, t.frozen = 1u;
        }
        double fold[CALIB_FOLD], m[CALIB_SCRATCH];
        for (int k = 0; k < CALIB_FOLD; ++k) fold[k] = 0.0;
        if (!t.frozen) {
            for (int l = 0; l < 64; ++l) {
                for (int k = 0; k < CALIB_FOLD; ++k) lanes[l][k] = 0.0;
                for (uint32_t r = (uint32_t)l; r < t.n_usable; r += 64u) {
                    const double *blk = w.blocks + (size_t)w.list[r] * CALIB_BLOCK;
                    for (int k = 0; k < CALIB_FOLD; ++k) lanes[l][k] += blk[k];
                }
            }
            calib_fold<CALIB_FOLD>(lanes.get());
            for (int k = 0; k < CALIB_FOLD; ++k) fold[k] = lanes[0][k];
        }
        calib_step(t, it, a.iterations, LENS, held, fold, m);
    };

    for (uint32_t it = 0; it <= a.iterations; ++it) {
        blocks(it, false);
        solve(it);
    }
    blocks(a.iterations + 1u, true);
}

}  // namespace

const char *calib_args_bad(const CalibArgs &a, int lens)
{
    if (a.n_frames < 1 || (uint32_t)a.n_frames > CALIB_MAX_FRAMES || !a.tags_per_frame) return "n_frames in 1 .. 65535, tags_per_frame > 0";
    if (!a.tags || !a.n_tags || !a.pose_in || !a.row_status || !a.fit_status || !a.camera_out || !a.pose || !a.frame_cost || !a.frame_n || !a.report)
        return "a null array";
    if (!a.cols || !a.rows || (uint64_t)a.cols * a.rows > FIT_MAX_BOARD || !f32_finite(a.spacing_ratio) || !(a.spacing_ratio > -1.0f))
        return "rows * cols in 1 .. 4096, spacing_ratio finite and > -1";
    if (!pose_args_ok(lens, a.camera, a.tag_size, 0u)) return AGX_LENS_CAMERA_RULE ", tag_size finite and > 0";
    if (!calib_args_ok(a.damping, a.iterations, a.min_tags, a.min_frames, a.fixed_mask, a.flags))
        return "damping finite and >= 0, iterations <= 64, min_tags and min_frames >= 1, fixed_mask below 2^9, flags AGX_CALIB_ACCEPT_LOOSE or 0";
    if ((((uintptr_t)a.tags | (uintptr_t)a.n_tags | (uintptr_t)a.tag_status | (uintptr_t)a.row_status | (uintptr_t)a.fit_status | (uintptr_t)a.frame_cost |
          (uintptr_t)a.frame_n) & 3) || (((uintptr_t)a.pose_in | (uintptr_t)a.camera_out | (uintptr_t)a.pose | (uintptr_t)a.report) & 7))
        return "the binary64 arrays and the report must be 8-byte aligned, every other array 4-byte aligned";
    if ((uint64_t)a.n_frames * a.tags_per_frame >= (1ull << 27)) return "at most 2^27 - 1 tag rows per batch";
    return nullptr;
}

void calibrate_host(const CalibArgs &a, int lens)
{
    with_lens(lens, [&](auto L) { calibrate_lens<decltype(L)::value>(a); });
}

// OpenCV's initCameraMatrix2D: the principal point at the image's centre, 1 / fx^2 and 1 / fy^2 from the two orthogonality
// constraints of every homography (Zhang 2000), h1 . w h2 = 0 and (h1 + h2) . w (h1 - h2) = 0 with w = diag(1 / fx^2, 1 / fy^2, 1)
// and the four vectors normalised, through the 2 x 2 normal equations; sums in frame order
uint32_t calibrate_seed_host(const double *h, const uint32_t *fit_status, uint32_t n, int img_w, int img_h, double *camera_out)
{
    const double cx = ((double)img_w - 1.0) / 2.0, cy = ((double)img_h - 1.0) / 2.0;
    double a00 = 0.0, a01 = 0.0, a11 = 0.0, b0 = 0.0, b1 = 0.0;
    uint32_t used = 0;
    for (uint32_t f = 0; f < n; ++f) {
        if (fit_status[f] != AGX_FIT_OK && fit_status[f] != AGX_FIT_LOOSE) continue;
        const double *H = h + 9 * (size_t)f;
        const double c1[3] = {H[0] - H[6] * cx, H[3] - H[6] * cy, H[6]}, c2[3] = {H[1] - H[7] * cx, H[4] - H[7] * cy, H[7]};
        double v[4][3];  // h1, h2, (h1 + h2) / 2, (h1 - h2) / 2, each normalised
        bool ok = true;
        for (int i = 0; i < 3; ++i) v[0][i] = c1[i], v[1][i] = c2[i], v[2][i] = (c1[i] + c2[i]) / 2.0, v[3][i] = (c1[i] - c2[i]) / 2.0;
        for (int k = 0; k < 4; ++k) {
            const double nk = pose_sqrt(v[k][0] * v[k][0] + v[k][1] * v[k][1] + v[k][2] * v[k][2]);
            ok = ok && f64_finite(nk) && nk > 0.0;
            for (int i = 0; i < 3; ++i) v[k][i] = v[k][i] / nk;
        }
        if (!ok) continue;
        const double rows[2][3] = {{v[0][0] * v[1][0], v[0][1] * v[1][1], -(v[0][2] * v[1][2])}, {v[2][0] * v[3][0], v[2][1] * v[3][1], -(v[2][2] * v[3][2])}};
        for (int r = 0; r < 2; ++r) {
            a00 += rows[r][0] * rows[r][0];
            a01 += rows[r][0] * rows[r][1];
            a11 += rows[r][1] * rows[r][1];
            b0 += rows[r][0] * rows[r][2];
            b1 += rows[r][1] * rows[r][2];
        }
        ++used;
    }
    if (!used) return AGX_CALIB_FEW;
    const double det = a00 * a11 - a01 * a01, scale = a00 * a11;
    if (!f64_finite(det) || !(det > scale * (1.0 / 1099511627776.0)) || !(scale > 0.0)) return AGX_CALIB_SINGULAR;
    const double f0 = (b0 * a11 - a01 * b1) / det, f1 = (a00 * b1 - a01 * b0) / det;  // 1 / fx^2, 1 / fy^2
    if (!f64_finite(f0) || !f64_finite(f1) || !(f0 > 0.0) || !(f1 > 0.0)) return AGX_CALIB_SINGULAR;
    const double fx = pose_sqrt(1.0 / f0), fy = pose_sqrt(1.0 / f1);
    if (!f64_finite(fx) || !f64_finite(fy)) return AGX_CALIB_SINGULAR;
    const double out[9] = {fx, fy, cx, cy, 0.0, 0.0, 0.0, 0.0, 0.0};
    std::memcpy(camera_out, out, sizeof out);
    return AGX_CALIB_OK;
}

void calib_param_jacobian_host(int lens, const agx_camera &camera, const double *xyz, uint32_t n, double *out)
{
    const agx_camera cam = pose_camera(lens, camera);
    with_lens(lens, [&](auto L) {
        constexpr int LENS = decltype(L)::value;
        for (uint32_t i = 0; i < n; ++i) {
            const Pose p = {{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, {0.0, 0.0, xyz[3 * i + 2]}};
            PosePointOf<LENS> q;
            double *o = out + 18 * (size_t)i;
            if (pose_project<LENS>(cam, p, xyz[3 * i], xyz[3 * i + 1], q)) calib_param_jacobian(cam, q, o, o + 9);
            else
                for (int k = 0; k < 18; ++k) o[k] = std::numeric_limits<double>::quiet_NaN();
        }
    });
}

}  // namespace agx
