// rig_host.cpp -- the host forms of rig.hip (agx_rig_calibrate_tail): the launches of k_rig_blocks, k_rig_instants and k_rig_solve
// one after the other, a wave's 64 lanes one after the other, every number rig_math.h's -- the same bytes.  And the two host-only
// pieces: the closed-form seed (agx_rig_seed_tail) and the row's Jacobian for tests (agx_debug_rig_jacobian).
#include <cstring>
#include <limits>
#include <vector>

#include "rig.h"
#include "rig_math.h"

namespace agx {
namespace {

// the kernels' fold: p[l] + p[l ^ m] over m = 32 .. 1, of which lane 0's value needs p[l] += p[l + m] for l < m only
void rig_fold(std::vector<double> &lanes, int n)
{
    for (int m = 32; m >= 1; m >>= 1)
        for (int l = 0; l < m; ++l)
            for (int k = 0; k < n; ++k) lanes[(size_t)l * n + k] = lanes[(size_t)l * n + k] + lanes[(size_t)(l + m) * n + k];
}

// 4 x the frame's inlier rows on the board, 0 for a frame that is not usable (agx_calibrate_enqueue's rule)
uint32_t rig_frame_corners(const RigArgs &a, const FitGeom &g, size_t f)
{
    const uint32_t cnt = a.n_tags[f];
    const size_t row0 = f * a.tags_per_frame;
    const bool ok = calib_frame_ok(a.fit_status[f], a.flags) && cnt <= a.tags_per_frame && cnt <= FIT_MAX_ROWS && !(a.tag_status && a.tag_status[f] != AGX_TAGS_OK);
    if (!ok) return 0u;
    uint32_t n_inl = 0;
    for (uint32_t r = 0; r < cnt; ++r) n_inl += calib_row_counts(g, a.tags[row0 + r].id, a.row_status[row0 + r]) ? 1u : 0u;
    return n_inl >= a.min_tags ? 4u * n_inl : 0u;
}

template <int LENS, int PART>
void rig_pass_host(const agx_tag *tags, const uint8_t *st, uint32_t cnt, const FitGeom &g, double tag_size, const agx_camera &cam, bool free_cam, const Pose &e,
                   const Pose &t, const Pose &p, double *blk)
{
    constexpr int N = RIG_PART_SUMS[PART];
    std::vector<double> lanes((size_t)64 * N, 0.0);
    for (int l = 0; l < 64; ++l)
        for (uint32_t r = (uint32_t)l; r < cnt; r += 64u) {
            if (!st[r]) continue;
            if (free_cam) rig_accumulate_row<LENS, PART>(g, tag_size, cam, e, t, p, &lanes[(size_t)l * N], tags[r].id, tags[r].xy);
            else pose_accumulate_row<LENS>(g, tag_size, cam, t, &lanes[(size_t)l * N], tags[r].id, tags[r].xy);
        }
    rig_fold(lanes, N);
    for (int k = 0; k < N; ++k) blk[rig_part_slot(PART, k)] = lanes[k];
}

template <int LENS>
void rig_frame_sums(const RigArgs &a, const FitGeom &g, size_t f, int c, const uint8_t *st, const Pose &e, const Pose &t, double *blk)
{
    const agx_camera cam = pose_camera(LENS, a.camera[c]);
    const agx_tag *tags = a.tags + f * a.tags_per_frame;
    const uint32_t cnt = a.n_tags[f];
    if (c == 0) {
        rig_pass_host<LENS, 2>(tags, st, cnt, g, a.tag_size, cam, false, e, t, t, blk);
        return;
    }
    const Pose p = rig_compose(e, t);
    rig_pass_host<LENS, 0>(tags, st, cnt, g, a.tag_size, cam, true, e, t, p, blk);
    rig_pass_host<LENS, 1>(tags, st, cnt, g, a.tag_size, cam, true, e, t, p, blk);
    rig_pass_host<LENS, 2>(tags, st, cnt, g, a.tag_size, cam, true, e, t, p, blk);
}

}  // namespace

const char *rig_args_bad(const RigArgs &a, bool host)
{
    if (!rig_args_ok(a.n_cams, a.n_instants, a.damping, a.iterations, a.min_tags, a.min_cams, a.min_instants, a.flags))
        return "n_cams in 2 .. 8, n_cams * n_instants in 1 .. 65535, damping finite and >= 0, iterations <= 64, min_tags, min_cams and min_instants >= 1, "
               "flags AGX_CALIB_ACCEPT_LOOSE or 0";
    if (!a.tags_per_frame) return "tags_per_frame > 0";
    if (!a.tags || !a.n_tags || !a.pose_in || !a.row_status || !a.fit_status || !a.ext_in || !a.ext || !a.rig_pose || !a.frame_cost || !a.frame_n || !a.cam_n ||
        !a.report)
        return "a null array";
    if (!a.cols || !a.rows || (uint64_t)a.cols * a.rows > FIT_MAX_BOARD || !f32_finite(a.spacing_ratio) || !(a.spacing_ratio > -1.0f))
        return "rows * cols in 1 .. 4096, spacing_ratio finite and > -1";
    for (int c = 0; c < a.n_cams; ++c)
        if (!pose_args_ok(a.lens[c], a.camera[c], a.tag_size, 0u)) return "every camera: " AGX_LENS_CAMERA_RULE ", tag_size finite and > 0";
    if ((((uintptr_t)a.tags | (uintptr_t)a.n_tags | (uintptr_t)a.tag_status | (uintptr_t)a.row_status | (uintptr_t)a.fit_status | (uintptr_t)a.frame_cost |
          (uintptr_t)a.frame_n | (uintptr_t)a.cam_n) & 3) ||
        (((uintptr_t)a.pose_in | (uintptr_t)a.ext_in | (uintptr_t)a.ext | (uintptr_t)a.rig_pose | (uintptr_t)a.report) & 7))
        return "the binary64 arrays and the report must be 8-byte aligned, every other array 4-byte aligned";
    if ((uint64_t)a.n_cams * a.n_instants * a.tags_per_frame >= (1ull << 27)) return "at most 2^27 - 1 tag rows per batch";
    if (host)
        for (int i = 0; i < 12 * a.n_cams; ++i)
            if (!f64_finite(a.ext_in[i])) return "a seed extrinsic that is not finite";
    return nullptr;
}

void rig_calibrate_host(const RigArgs &a)
{
    const int C = a.n_cams, S = a.n_instants, n = rig_n(C), nt = rig_tri(n), FL = rig_fold_len(C), BL = rig_block_len(C), W = 6 * C + 1, M = n + 1;
    const size_t nf = (size_t)C * S;
    std::vector<char> mem(rig_work_bytes(C, S) + 8);
    const RigWork w = rig_work(mem.data() + ((8 - ((uintptr_t)mem.data() & 7)) & 7), C, S);
    RigCtl &t = *w.ctl;
    const FitGeom g = pose_geom(a.cols, a.rows, a.first_id, a.spacing_ratio);
    std::vector<uint8_t> st(FIT_MAX_ROWS);

    const auto blocks = [&](uint32_t it) {  // k_rig_blocks(it)
        for (size_t f = 0; f < nf; ++f) {
            const int c = (int)(f / (size_t)S), s = (int)(f % (size_t)S);
            Pose e, T;
            if (it == 0u) {
                uint32_t raw[RIG_MAX_CAMS], n_ok = 0;
                int low = -1;
                for (int k = 0; k < C; ++k) {
                    raw[k] = rig_frame_corners(a, g, (size_t)k * S + s);
                    if (raw[k]) {
                        ++n_ok;
                        if (low < 0) low = k;
                    }
                }
                const bool ok = n_ok >= a.min_cams;
                w.corners[f] = ok ? raw[c] : 0u;
                if (ok) T = rig_seed_instant(low, rig_load(a.ext_in + 12 * low), rig_load(a.pose_in + ((size_t)low * S + s) * 12));
                if (c == 0) {
                    w.inst_ok[s] = ok ? 1u : 0u;
                    if (ok) {
                        rig_store(w.t_cur + (size_t)s * 12, T);
                        rig_store(w.t_best + (size_t)s * 12, T);
                    }
                }
                if (!w.corners[f]) continue;
                e = c == 0 ? rig_identity() : rig_load(a.ext_in + 12 * c);
            } else {
                if (t.frozen || !w.corners[f]) continue;
                e = rig_load(t.ext[c]);
                T = rig_load(w.t_cur + (size_t)s * 12);
            }
            const uint32_t cnt = a.n_tags[f];
            const size_t row0 = f * a.tags_per_frame;
            for (uint32_t r = 0; r < cnt; ++r) st[r] = calib_row_counts(g, a.tags[row0 + r].id, a.row_status[row0 + r]) ? 1 : 0;
            double *blk = w.frames + f * RIG_FRAME;
            with_lens(a.lens[c], [&](auto L) { rig_frame_sums<decltype(L)::value>(a, g, f, c, st.data(), e, T, blk); });
        }
    };

    std::vector<double> m((size_t)6 * RIG_MAX_W), x((size_t)6 * (RIG_MAX_N + 1));
    const auto instants = [&](uint32_t it) {  // k_rig_instants(it)
        if (it > 0u && t.frozen) return;
        for (int s = 0; s < S; ++s) {
            if (!w.inst_ok[s]) continue;
            const auto blk = [&](int c) -> const double * { return w.corners[(size_t)c * S + s] ? w.frames + ((size_t)c * S + s) * RIG_FRAME : nullptr; };
            double sum28[POSE_SUMS];
            for (int e = 0; e < POSE_SUMS; ++e) sum28[e] = rig_instant_sum(C, blk, e);
            for (int k = 0; k < 6; ++k)
                for (int col = 0; col < W; ++col) m[(size_t)W * k + col] = rig_instant_entry(C, blk, sum28, a.damping, k, col);
            const bool solved = rig_eliminate(C, m.data(), x.data());
            double *ib = w.instants + (size_t)s * BL;
            for (int e = 0; e < nt + n; ++e) ib[e] = solved ? rig_schur_entry(C, blk, x.data(), a.damping, e) : 0.0;
            ib[nt + n] = sum28[27];
            ib[nt + n + 1] = solved ? 0.0 : 1.0;
            for (int e = 0; e < 6 * M; ++e) {
                const int k = e / M, j = e - M * k;
                ib[FL + (j < n ? n * k + j : 6 * n + k)] = solved ? x[e] : 0.0;
            }
        }
    };

    std::vector<double> lanes((size_t)64 * FL), fold(FL), scratch(RIG_SCRATCH);
    const auto solve = [&](uint32_t it) {  // k_rig_solve(it)
        if (it == 0u) {
            rig_ctl_init(t, C, a.ext_in);
            uint32_t base = 0;
            for (int s = 0; s < S; ++s)
                if (w.inst_ok[s]) w.list[base++] = (uint32_t)s;
            t.n_instants_used = base;
            for (int c = 0; c < C; ++c) {
                for (int s = 0; s < S; ++s) {
                    const uint32_t k = w.corners[(size_t)c * S + s];
                    t.cam_n[c] += k ? 1u : 0u;
                    t.n_corners += k;
                }
                t.n_frames_used += t.cam_n[c];
                if (c >= 1) {
                    if (t.cam_n[c]) ++t.n_cams_free;
                    else t.held |= 1u << c;
                }
            }
            if (rig_few(t.n_instants_used, t.n_cams_free, t.n_corners, a.min_instants)) t.status = AGX_RIG_FEW, t.frozen = 1u;
        }
        for (int k = 0; k < FL; ++k) fold[k] = 0.0;
        if (!t.frozen) {
            for (int l = 0; l < 64; ++l) {
                for (int k = 0; k < FL; ++k) lanes[(size_t)l * FL + k] = 0.0;
                for (uint32_t r = (uint32_t)l; r < t.n_instants_used; r += 64u) {
                    const double *ib = w.instants + (size_t)w.list[r] * BL;
                    for (int k = 0; k < FL; ++k) lanes[(size_t)l * FL + k] += ib[k];
                }
            }
            rig_fold(lanes, FL);
            for (int k = 0; k < FL; ++k) fold[k] = lanes[k];
        }
        rig_step(t, it, a.iterations, C, fold.data(), scratch.data());
        if (t.mark_best) {
            for (uint32_t r = 0; r < t.n_instants_used; ++r) std::memcpy(w.t_best + (size_t)w.list[r] * 12, w.t_cur + (size_t)w.list[r] * 12, 12 * sizeof(double));
            for (size_t f = 0; f < nf; ++f)
                if (w.corners[f]) w.cost_best[f] = w.frames[f * RIG_FRAME + 90];
        }
        if (t.apply)
            for (uint32_t r = 0; r < t.n_instants_used; ++r) {
                const size_t s = w.list[r];
                Pose T = rig_load(w.t_cur + s * 12);
                rig_instant_step(T, n, w.instants + s * BL + FL, t.de);
                rig_store(w.t_cur + s * 12, T);
            }
        if (it != a.iterations) return;
        if (t.status == AGX_RIG_OK) {
            for (int c = 0; c < C; ++c) {
                std::memcpy(a.ext + 12 * c, t.ext_best[c], 12 * sizeof(double));
                a.cam_n[c] = t.cam_n[c];
            }
            for (uint32_t r = 0; r < t.n_instants_used; ++r) std::memcpy(a.rig_pose + (size_t)w.list[r] * 12, w.t_best + (size_t)w.list[r] * 12, 12 * sizeof(double));
            for (size_t f = 0; f < nf; ++f) {
                a.frame_cost[f] = w.corners[f] ? (float)w.cost_best[f] : 0.0f;
                a.frame_n[f] = w.corners[f];
            }
        }
        rig_report(t, a.report);
    };

    for (uint32_t it = 0; it <= a.iterations; ++it) {
        blocks(it);
        instants(it);
        solve(it);
    }
}

// Levels from camera 0: in every level each camera that is not attached yet looks, in camera order, for the lowest-numbered
// camera attached in an earlier level with which it shares an instant (both status words AGX_FIT_OK; with frame_n, both counts
// > 0); among the shared instants the one with the largest frame_n[c, s] + frame_n[r, s], the lowest s at ties.
void rig_seed_host(int n_cams, int n_instants, const double *pose, const uint32_t *fit_status, const uint32_t *frame_n, double *ext_out, uint32_t *cam_status)
{
    const size_t S = (size_t)n_instants;
    std::vector<int> level(n_cams, -1);
    const Pose id = rig_identity();
    for (int c = 0; c < n_cams; ++c) {
        rig_store(ext_out + 12 * c, id);
        cam_status[c] = AGX_RIG_CAM_DETACHED;
    }
    level[0] = 0;
    cam_status[0] = AGX_RIG_CAM_ATTACHED;
    const auto seen = [&](int c, size_t s) { return fit_status[c * S + s] == AGX_FIT_OK && (!frame_n || frame_n[c * S + s] > 0u); };
    for (int lv = 1; lv < n_cams; ++lv) {
        bool any = false;
        for (int c = 1; c < n_cams; ++c) {
            if (level[c] >= 0) continue;
            for (int r = 0; r < n_cams && level[c] < 0; ++r) {
                if (level[r] < 0 || level[r] >= lv) continue;
                long best_s = -1;
                uint64_t best_n = 0;
                for (size_t s = 0; s < S; ++s) {
                    if (!seen(c, s) || !seen(r, s)) continue;
                    const uint64_t k = frame_n ? (uint64_t)frame_n[c * S + s] + frame_n[r * S + s] : 1u;
                    if (best_s < 0 || k > best_n) best_s = (long)s, best_n = k;
                }
                if (best_s < 0) continue;
                const Pose pc = rig_load(pose + (c * S + (size_t)best_s) * 12), pr = rig_load(pose + (r * S + (size_t)best_s) * 12);
                const Pose e = rig_compose(rig_compose(pc, rig_inverse(pr)), rig_load(ext_out + 12 * r));
                rig_store(ext_out + 12 * c, e);
                level[c] = lv;
                cam_status[c] = AGX_RIG_CAM_ATTACHED;
                any = true;
            }
        }
        if (!any) break;
    }
}

void rig_jacobian_host(int lens, const agx_camera &camera, const double *extrinsic, const double *rig_pose, const double *xy, uint32_t n, double *out)
{
    const agx_camera cam = pose_camera(lens, camera);
    const Pose T = rig_load(rig_pose);
    with_lens(lens, [&](auto L) {
        constexpr int LENS = decltype(L)::value;
        for (uint32_t i = 0; i < n; ++i) {
            double ja[RIG_COLS + 1] = {0.0}, jb[RIG_COLS + 1] = {0.0};
            double *o = out + 24 * (size_t)i;
            const double X = xy[2 * i], Y = xy[2 * i + 1];
            bool ok;
            if (extrinsic) {
                const Pose E = rig_load(extrinsic);
                ok = rig_row<LENS>(cam, E, T, rig_compose(E, T), X, Y, 0.0, 0.0, ja, jb) < __builtin_inf();
            } else {  // camera 0: the T_s part alone, pose_accumulate's row
                PosePointOf<LENS> q;
                ok = pose_project<LENS>(cam, T, X, Y, q);
                if (ok) pose_jacobian_rows<LENS>(cam, T, q, X, Y, ja + 6, jb + 6);
            }
            for (int k = 0; k < RIG_COLS; ++k) {
                o[k] = ok ? ja[k] : std::numeric_limits<double>::quiet_NaN();
                o[RIG_COLS + k] = ok ? jb[k] : std::numeric_limits<double>::quiet_NaN();
            }
        }
    });
}

}  // namespace agx
