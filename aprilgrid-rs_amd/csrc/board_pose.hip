// board_pose.hip -- k_board_pose (agx_board_pose_enqueue): per frame the board's pose (R, t: board -> camera) under the pinhole +
// radial-tangential model through all 4 n correspondences of the frame's tag table -- a homography seed on undistorted corners,
// Gauss-Newton steps on the pixel residual with the best iterate kept, rounds that drop the worst row while it disagrees with
// the board -- and the predicted corners of the layout's tags through the lens model.  Every number is board_pose_math.h's,
// which the host form (host_tail.cpp: board_pose) runs too: the two give the same bytes.
// Geometry: k_board_fit's (board_fit.hip).  One wave per frame, POSE_FRAMES_PER_WG frames per workgroup; the waves of a
// workgroup never meet (no workgroup barrier: each frame runs its own number of rounds and iterates).  A frame's rows are staged
// once in LDS (36 B a row, a stride of 9 dwords) with a status byte per row.  A pass of sums: lane l adds the inlier rows l,
// l + 64, ... into its sums (registers; 44 for the seed, 28 for an iterate), the sums are folded by shuffles over l ^ 32, 16, 8, 4,
// 2, 1, lane 0 eliminates the system in LDS (its rows are indexed at run time -- registers would go to scratch) and every lane
// reads the unknowns back and applies them to its own copy of the pose, which is the same bytes in all lanes.  Residuals: one
// lane per row, a (residual, lowest row) key folded by shuffles.  The frame's verdict is known before its first store.
// Prediction: one lane per tag of the layout, 64 at a time, compacted by ballot under AGX_FIT_PREDICT_MISSING against a bitmap of
// the inlier rows' ids.  No floating-point atomics.
// The kernel is a template on the lens model (AGX_LENS_*): the projection, the lens's Jacobian and the seed's undistortion are
// board_pose_math.h's for that model, everything else is one text.  No instantiation uses scratch.  Under
// AGX_LENS_DOUBLE_SPHERE the camera in the arguments is pose_camera()'s, which the launch makes on the host.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "board_pose.h"
#include "board_pose_math.h"
#include "board_rounds.h"

namespace agx {
namespace {

using u64 = unsigned long long;

struct PoseFrameLds {
    double m[72];                         // the augmented system, lane 0's: 8 x 9 for the seed, 6 x 7 for an iterate
    double sol[8];                        // its solution
    uint32_t rows[FIT_MAX_ROWS * 9];      // the frame's tag rows as they stand in the table
    uint32_t member[FIT_MAX_BOARD / 32];  // AGX_FIT_PREDICT_MISSING: bit t = the layout's tag t is an inlier row
    uint32_t solved;
    uint8_t st[FIT_MAX_ROWS];  // AGX_FIT_ROW_*
};
static_assert(sizeof(PoseFrameLds) * POSE_FRAMES_PER_WG <= 65536, "k_board_pose: static LDS");

// LDS written by some lanes of this wave, read by others: order the accesses (no workgroup barrier: the waves run apart)
__device__ __forceinline__ void pose_wsync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ void pose_row_xy(const uint32_t *row, float xy[8])
{
#pragma unroll
    for (int j = 0; j < 8; ++j) xy[j] = f32_from_bits(row[1 + j]);
}

template <int LENS>
__global__ void __launch_bounds__(64 * POSE_FRAMES_PER_WG) k_board_pose(BoardPoseArgs b)
{
    __shared__ PoseFrameLds lds[POSE_FRAMES_PER_WG];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t f = blockIdx.x * POSE_FRAMES_PER_WG + wave;
    if (f >= (uint32_t)b.n_frames) return;  // (the whole wave)
    PoseFrameLds &s = lds[wave];
    const FitGeom g = pose_geom(b.cols, b.rows, b.first_id, b.spacing_ratio);
    const agx_camera &cam = b.camera;
    const uint32_t cnt = b.n_tags[f];
    const u64 row0 = (u64)f * b.tags_per_frame;
    bool input = cnt > b.tags_per_frame || cnt > FIT_MAX_ROWS || (b.tag_status && b.tag_status[f] != AGX_TAGS_OK);
    uint32_t n_inl = 0;
    if (!input) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(b.tags + row0);
        for (uint32_t i = lane; i < cnt * 9u; i += 64u) s.rows[i] = src[i];
        pose_wsync();
        bool bad = false;
        for (uint32_t r = lane; r < cnt; r += 64u) {
            const uint32_t *row = s.rows + 9u * r;
            uint32_t st = AGX_FIT_ROW_OFF_BOARD;
            if (fit_on_board(g, row[0])) {
                st = AGX_FIT_ROW_INLIER;
                ++n_inl;
#pragma unroll
                for (int j = 0; j < 8; ++j) bad = bad || !f32_finite(f32_from_bits(row[1 + j]));
            }
            s.st[r] = (uint8_t)st;
        }
        input = __ballot(bad) != 0;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) n_inl += __shfl_xor(n_inl, m);
    }
    uint32_t status = input ? AGX_FIT_INPUT : AGX_FIT_OK, drops = 0, best_it = 0;
    Pose pose;
#pragma unroll
    for (int i = 0; i < 9; ++i) pose.R[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) pose.t[i] = 0.0;
    double sum_sq = 0.0;
    // every branch below is taken by the whole wave: cnt, n_inl, drops, the folded sums, the pose and the folded key are the same in all lanes
    if (status == AGX_FIT_OK && n_inl < b.min_tags) status = AGX_FIT_FEW;
    if (status == AGX_FIT_OK) {  // the seed: a homography through the undistorted corners, decomposed
        double acc[FIT_SUMS];
#pragma unroll
        for (int k = 0; k < FIT_SUMS; ++k) acc[k] = 0.0;
        for (uint32_t r = lane; r < cnt; r += 64u) {
            if (s.st[r] != AGX_FIT_ROW_INLIER) continue;
            float xy[8];
            pose_row_xy(s.rows + 9u * r, xy);
            pose_seed_accumulate_row<LENS>(g, cam, acc, s.rows[9u * r], xy);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
            for (int k = 0; k < FIT_SUMS; ++k) acc[k] += __shfl_xor(acc[k], m);
        if (lane == 0) {
            fit_system(acc, s.m);
            s.solved = fit_solve(s.m, s.sol) ? 1u : 0u;
        }
        pose_wsync();
        const bool solved = s.solved != 0u;
        double h[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) h[i] = s.sol[i];
        pose_wsync();  // (read before lane 0 writes the first iterate's system)
        if (!solved || !pose_from_homography(g, b.tag_size, h, pose)) status = AGX_FIT_SINGULAR;
    }
    while (status == AGX_FIT_OK) {  // a round
        if (n_inl < b.min_tags) {
            status = AGX_FIT_FEW;
            break;
        }
        Pose cur = pose;
        double best_cost = 0.0;
        bool have = false, singular = false;
        best_it = 0;
        for (uint32_t it = 0;; ++it) {
            double acc[POSE_SUMS];
#pragma unroll
            for (int k = 0; k < POSE_SUMS; ++k) acc[k] = 0.0;
            for (uint32_t r = lane; r < cnt; r += 64u) {
                if (s.st[r] != AGX_FIT_ROW_INLIER) continue;
                float xy[8];
                pose_row_xy(s.rows + 9u * r, xy);
                pose_accumulate_row<LENS>(g, b.tag_size, cam, cur, acc, s.rows[9u * r], xy);
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
                for (int k = 0; k < POSE_SUMS; ++k) acc[k] += __shfl_xor(acc[k], m);
            if (pose_better(acc[27], have, best_cost)) {
                pose = cur;
                best_cost = acc[27];
                best_it = it;
                have = true;
            }
            if (it == b.iterations) break;  // (the last iterate's pass gave its sum of |e|^2 only)
            if (lane == 0) {
                pose_system(acc, s.m);
                s.solved = fit_solve_n<6>(s.m, s.sol) ? 1u : 0u;
            }
            pose_wsync();
            const bool solved = s.solved != 0u;
            double d[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) d[i] = s.sol[i];
            pose_wsync();  // (read before lane 0 of the next iterate writes)
            if (!solved) {
                singular = it == 0;
                break;
            }
            pose_update(cur, d);
        }
        if (singular || !pose_gram_schmidt(pose.R)) {
            status = AGX_FIT_SINGULAR;
            break;
        }
        u64 key = 0;  // (residual bits, ~row): the largest residual, the lowest row at equal bits; 0 = no inlier row
        double part = 0.0;
        for (uint32_t r = lane; r < cnt; r += 64u) {
            if (s.st[r] != AGX_FIT_ROW_INLIER) continue;
            float xy[8];
            double sum;
            pose_row_xy(s.rows + 9u * r, xy);
            const float e = pose_row_residual<LENS>(g, b.tag_size, cam, pose, s.rows[9u * r], xy, &sum);
            part += sum;
            const u64 k = ((u64)f32_bits(e) << 32) | (u64)(0xffffffffu - r);
            key = k > key ? k : key;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const u64 o = __shfl_xor(key, m);
            key = o > key ? o : key;
        }
        const float worst = f32_from_bits((uint32_t)(key >> 32));
        if (worst > b.max_err_sq) {
            if (drops < b.max_drop) {
                const uint32_t r = 0xffffffffu - (uint32_t)key;  // (an inlier row: n_inl >= min_tags >= 1)
                if (lane == 0) s.st[r] = (uint8_t)AGX_FIT_ROW_OUTLIER;
                pose_wsync();
                ++drops;
                --n_inl;
                continue;
            }
            status = AGX_FIT_LOOSE;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) part += __shfl_xor(part, m);
        sum_sq = part;
        break;
    }
    if (status != AGX_FIT_OK && status != AGX_FIT_LOOSE) {  // refused: the two counts and the verdict, nothing else
        if (lane == 0) {
            b.n_inliers[f] = 0u;
            b.n_pred[f] = 0u;
            b.status[f] = status;
        }
        return;
    }
    for (uint32_t r = lane; r < cnt; r += 64u) {
        const uint32_t st = s.st[r];
        b.row_status[row0 + r] = st;
        if (st == AGX_FIT_ROW_OFF_BOARD) continue;
        float xy[8];
        double sum;
        pose_row_xy(s.rows + 9u * r, xy);
        b.err_sq[row0 + r] = pose_row_residual<LENS>(g, b.tag_size, cam, pose, s.rows[9u * r], xy, &sum);
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) b.pose[(u64)f * 12u + i] = pose.R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) b.pose[(u64)f * 12u + 9u + i] = pose.t[i];
        b.n_inliers[f] = n_inl;
        b.rms[f] = fit_rms(sum_sq, n_inl);
        b.best_iter[f] = best_it;
        b.status[f] = status;
    }
    const bool missing = (b.flags & AGX_FIT_PREDICT_MISSING) != 0;
    if (missing) {
        for (uint32_t i = lane; i < (g.n_board + 31u) / 32u; i += 64u) s.member[i] = 0u;
        pose_wsync();
        for (uint32_t r = lane; r < cnt; r += 64u)
            if (s.st[r] == AGX_FIT_ROW_INLIER) {
                const uint32_t t = s.rows[9u * r] - g.first_id;  // (< n_board <= 4096: the row is on the board)
                atomicOr(&s.member[t >> 5], 1u << (t & 31u));
            }
        pose_wsync();
    }
    uint32_t *pred = reinterpret_cast<uint32_t *>(b.pred + (u64)f * g.n_board);
    uint32_t base = 0;
    for (uint32_t t0 = 0; t0 < g.n_board; t0 += 64u) {
        const uint32_t t = t0 + lane;
        const bool want = t < g.n_board && !(missing && ((s.member[t >> 5] >> (t & 31u)) & 1u));
        const u64 mask = __ballot(want);
        if (want) {
            uint32_t *row = pred + 9u * (u64)(base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)));
            float xy[8];
            pose_predict<LENS>(g, b.tag_size, cam, pose, t, xy);
            row[0] = g.first_id + t;
#pragma unroll
            for (int j = 0; j < 8; ++j) row[1 + j] = f32_bits(xy[j]);
        }
        base += (uint32_t)__popcll(mask);
    }
    if (lane == 0) b.n_pred[f] = base;
}

}  // namespace

const char *board_pose_args_bad(const BoardPoseArgs &b, int lens, bool device)
{
    return rounds_args_bad(b, device, b.pose, b.best_iter,
                           pose_args_ok(lens, b.camera, b.tag_size, b.iterations) ? nullptr : AGX_LENS_CAMERA_RULE ", tag_size finite and > 0, iterations <= 64");
}

int launch_board_pose(const BoardPoseArgs &b, int lens, void *stream)
{
    if (board_pose_args_bad(b, lens, true)) return (int)hipErrorInvalidValue;
    const unsigned grid = ((unsigned)b.n_frames + POSE_FRAMES_PER_WG - 1) / POSE_FRAMES_PER_WG;
    BoardPoseArgs d = b;
    d.camera = pose_camera(lens, b.camera);  // (w2 once per call, by the host form's statements; the caller's camera under the other two)
    with_lens(lens, [&](auto L) {
        hipLaunchKernelGGL(k_board_pose<decltype(L)::value>, dim3(grid), dim3(64 * POSE_FRAMES_PER_WG), 0, (hipStream_t)stream, d);
    });
    return (int)hipGetLastError();
}

}  // namespace agx
