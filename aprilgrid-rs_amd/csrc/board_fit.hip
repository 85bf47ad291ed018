// board_fit.hip -- k_board_fit (agx_board_fit_enqueue): per frame the homography from the printed board to the image through
// all 4 n correspondences of the frame's tag table, rounds that drop the worst row while it disagrees with the board, and the
// predicted corners of the layout's tags.  Every number is board_fit_math.h's, which the host form (host_tail.cpp: board_fit)
// runs too: the two give the same bytes.
// Geometry: one wave per frame, FIT_FRAMES_PER_WG frames per workgroup; the waves of a workgroup never meet (no workgroup
// barrier: each frame runs its own number of rounds).  A frame's rows are staged once in LDS (36 B a row, a stride of 9 dwords:
// lane r reads row r without a bank conflict) with a status byte per row.  A round: lane l adds the inlier rows l, l + 64, ... into
// its 44 binary64 sums (registers), the sums are folded by shuffles over l ^ 32, 16, 8, 4, 2, 1, lane 0 eliminates the 8 x 9
// system in LDS (its rows are indexed at run time -- registers would go to scratch) and every lane reads the eight unknowns back;
// one lane per row evaluates the residuals and a (residual, lowest row) key is folded by shuffles.  The frame's verdict is known
// before its first store.  Prediction: one lane per tag of the layout, 64 at a time, compacted by ballot under
// AGX_FIT_PREDICT_MISSING against a bitmap of the inlier rows' ids.  No floating-point atomics.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "board_fit.h"
#include "board_fit_math.h"
#include "board_rounds.h"

namespace agx {
namespace {

using u64 = unsigned long long;

struct FitFrameLds {
    double m[72];                         // the augmented system, lane 0's
    double sol[8];                        // its solution
    uint32_t rows[FIT_MAX_ROWS * 9];      // the frame's tag rows as they stand in the table
    uint32_t member[FIT_MAX_BOARD / 32];  // AGX_FIT_PREDICT_MISSING: bit t = the layout's tag t is an inlier row
    uint32_t solved;
    uint8_t st[FIT_MAX_ROWS];  // AGX_FIT_ROW_*
};
static_assert(sizeof(FitFrameLds) * FIT_FRAMES_PER_WG <= 65536, "k_board_fit: static LDS");

// LDS written by some lanes of this wave, read by others: order the accesses (no workgroup barrier: the waves run apart)
__device__ __forceinline__ void fit_wsync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ void fit_row_xy(const uint32_t *row, float xy[8])
{
#pragma unroll
    for (int j = 0; j < 8; ++j) xy[j] = f32_from_bits(row[1 + j]);
}

__global__ void __launch_bounds__(64 * FIT_FRAMES_PER_WG) k_board_fit(BoardFitArgs b)
{
    __shared__ FitFrameLds lds[FIT_FRAMES_PER_WG];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t f = blockIdx.x * FIT_FRAMES_PER_WG + wave;
    if (f >= (uint32_t)b.n_frames) return;  // (the whole wave)
    FitFrameLds &s = lds[wave];
    const FitGeom g = fit_geom(b.cols, b.rows, b.first_id, b.spacing_ratio, b.img_w, b.img_h);
    const uint32_t cnt = b.n_tags[f];
    const u64 row0 = (u64)f * b.tags_per_frame;
    bool input = cnt > b.tags_per_frame || cnt > FIT_MAX_ROWS || (b.tag_status && b.tag_status[f] != AGX_TAGS_OK);
    uint32_t n_inl = 0;
    if (!input) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(b.tags + row0);
        for (uint32_t i = lane; i < cnt * 9u; i += 64u) s.rows[i] = src[i];
        fit_wsync();
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
    uint32_t status = input ? AGX_FIT_INPUT : AGX_FIT_OK, drops = 0;
    double h[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sum_sq = 0.0;
    // every branch below is taken by the whole wave: cnt, n_inl, drops, the folded sums and the folded key are the same in all lanes
    while (status == AGX_FIT_OK) {
        if (n_inl < b.min_tags) {
            status = AGX_FIT_FEW;
            break;
        }
        double acc[FIT_SUMS];
#pragma unroll
        for (int k = 0; k < FIT_SUMS; ++k) acc[k] = 0.0;
        for (uint32_t r = lane; r < cnt; r += 64u) {
            if (s.st[r] != AGX_FIT_ROW_INLIER) continue;
            float xy[8];
            fit_row_xy(s.rows + 9u * r, xy);
            fit_accumulate_row(g, acc, s.rows[9u * r], xy);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
            for (int k = 0; k < FIT_SUMS; ++k) acc[k] += __shfl_xor(acc[k], m);
        if (lane == 0) {
            fit_system(acc, s.m);
            s.solved = fit_solve(s.m, s.sol) ? 1u : 0u;
        }
        fit_wsync();
        const bool solved = s.solved != 0u;
#pragma unroll
        for (int i = 0; i < 8; ++i) h[i] = s.sol[i];
        fit_wsync();  // (read before lane 0 of the next round writes)
        if (!solved) {
            status = AGX_FIT_SINGULAR;
            break;
        }
        u64 key = 0;  // (residual bits, ~row): the largest residual, the lowest row at equal bits; 0 = no inlier row
        double part = 0.0;
        for (uint32_t r = lane; r < cnt; r += 64u) {
            if (s.st[r] != AGX_FIT_ROW_INLIER) continue;
            float xy[8];
            double sum;
            fit_row_xy(s.rows + 9u * r, xy);
            const float e = fit_row_residual(g, h, s.rows[9u * r], xy, &sum);
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
                fit_wsync();
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
        fit_row_xy(s.rows + 9u * r, xy);
        b.err_sq[row0 + r] = fit_row_residual(g, h, s.rows[9u * r], xy, &sum);
    }
    if (lane == 0) {
        double H[9];
        fit_h_matrix(g, h, H);
#pragma unroll
        for (int i = 0; i < 9; ++i) b.h[(u64)f * 9u + i] = H[i];
        b.n_inliers[f] = n_inl;
        b.rms[f] = fit_rms(sum_sq, n_inl);
        b.status[f] = status;
    }
    const bool missing = (b.flags & AGX_FIT_PREDICT_MISSING) != 0;
    if (missing) {
        for (uint32_t i = lane; i < (g.n_board + 31u) / 32u; i += 64u) s.member[i] = 0u;
        fit_wsync();
        for (uint32_t r = lane; r < cnt; r += 64u)
            if (s.st[r] == AGX_FIT_ROW_INLIER) {
                const uint32_t t = s.rows[9u * r] - g.first_id;  // (< n_board <= 4096: the row is on the board)
                atomicOr(&s.member[t >> 5], 1u << (t & 31u));
            }
        fit_wsync();
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
            fit_predict(g, h, t, xy);
            row[0] = g.first_id + t;
#pragma unroll
            for (int j = 0; j < 8; ++j) row[1 + j] = f32_bits(xy[j]);
        }
        base += (uint32_t)__popcll(mask);
    }
    if (lane == 0) b.n_pred[f] = base;
}

}  // namespace

const char *board_fit_args_bad(const BoardFitArgs &b, bool device)
{
    return rounds_args_bad(b, device, b.h, b.h, b.img_w > 0 && b.img_h > 0 ? nullptr : "img_w and img_h > 0");
}

int launch_board_fit(const BoardFitArgs &b, void *stream)
{
    if (board_fit_args_bad(b, true)) return (int)hipErrorInvalidValue;
    const unsigned grid = ((unsigned)b.n_frames + FIT_FRAMES_PER_WG - 1) / FIT_FRAMES_PER_WG;
    hipLaunchKernelGGL(k_board_fit, dim3(grid), dim3(64 * FIT_FRAMES_PER_WG), 0, (hipStream_t)stream, b);
    return (int)hipGetLastError();
}

}  // namespace agx
