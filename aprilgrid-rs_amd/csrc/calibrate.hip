// calibrate.hip -- k_calib_blocks and k_calib_solve (agx_calibrate_enqueue): the camera's nine doubles and every usable frame's
// pose from a batch of tag tables by damped Gauss-Newton with the poses eliminated frame by frame.  Every number is
// calib_math.h's, which the host form (calibrate_host.cpp) runs too: the two give the same bytes.
// k_calib_blocks<LENS>(it): one wave per frame, CALIB_FRAMES_PER_WG frames per workgroup, the waves never meet.  A frame's rows
// are staged in LDS as k_board_pose stages them (36 B a row) with a status byte per row.  The wave first keeps the last iterate's
// pose and cost where k_calib_solve marked that iterate the best, then applies the last step's dp_f = z_f - Y_f dc to its pose,
// then takes the frame's 136 sums in four passes over the staged rows (46, 36, 33 and 21 sums in registers, the cheap row
// recomputed each pass; folded by shuffles), eliminates the 6 x 16 system in LDS (lane 0: its rows are indexed at run time) and
// stores the frame's block, one entry per lane.  The launch `finish` keeps the best once more and writes the call's outputs.
// k_calib_solve(it): one wave in all.  At iterate 0 it lists the usable frames in frame order (ballot) and decides AGX_CALIB_FEW;
// then lane l adds the blocks of the usable frames of rank l, l + 64, ..., the 56 sums are folded by shuffles and lane 0 runs
// calib_step on them in LDS: the best-iterate rule, the scaled 9 x 10 elimination, the next camera.
// The camera, the step and all blocks stay in the workspace; nothing returns to the host.  No floating-point atomics, no scratch.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "calib_math.h"
#include "calibrate.h"

namespace agx {
namespace {

using u64 = unsigned long long;

struct CalibFrameLds {
    CalibFrameSys sys;
    uint32_t rows[FIT_MAX_ROWS * 9];  // the frame's tag rows as they stand in the table
    uint32_t solved;
    uint8_t st[FIT_MAX_ROWS];  // 1: an inlier row on the board
};
static_assert(sizeof(CalibFrameLds) * CALIB_FRAMES_PER_WG <= 65536, "k_calib_blocks: static LDS");

// LDS written by some lanes of this wave, read by others: order the accesses (no workgroup barrier: the waves run apart)
__device__ __forceinline__ void calib_wsync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one pass over the staged rows: part PART's sums of the frame, folded, the same bytes in every lane
template <int LENS, int PART>
__device__ __forceinline__ void calib_pass(const CalibFrameLds &s, uint32_t cnt, uint32_t lane, const FitGeom &g, double tag_size, const agx_camera &cam,
                                           const Pose &pose, double (&acc)[CALIB_PART_SUMS[PART]])
{
    constexpr int N = CALIB_PART_SUMS[PART];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0;
    for (uint32_t r = lane; r < cnt; r += 64u) {
        if (!s.st[r]) continue;
        float xy[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) xy[j] = f32_from_bits(s.rows[9u * r + 1 + j]);
        calib_accumulate_row<LENS, PART>(g, tag_size, cam, pose, acc, s.rows[9u * r], xy);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k] += __shfl_xor(acc[k], m);
}

template <int LENS>
__global__ void __launch_bounds__(64 * CALIB_FRAMES_PER_WG) k_calib_blocks(CalibArgs a, CalibWork w, uint32_t it, int finish)
{
    __shared__ CalibFrameLds lds[CALIB_FRAMES_PER_WG];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t f = blockIdx.x * CALIB_FRAMES_PER_WG + wave;
    if (f >= (uint32_t)a.n_frames) return;  // (the whole wave)
    CalibFrameLds &s = lds[wave];
    const CalibCtl &t = *w.ctl;  // (written by k_calib_solve only: it == 0 reads nothing of it)
    double *blk = w.blocks + (u64)f * CALIB_BLOCK;
    // every branch below is taken by the whole wave
    if (it > 0u || finish) {
        const uint32_t corners = w.corners[f];
        if (t.mark_best && corners && lane < 13u) {  // the iterate folded last is the best so far: keep its pose and cost
            if (lane < 12u) w.pose_best[(u64)f * 12u + lane] = w.pose_cur[(u64)f * 12u + lane];
            else w.cost_best[f] = blk[54];
        }
        if (finish) {  // the outputs, from what this wave holds (lanes 0 .. 12 wrote what they read back)
            if (t.status == AGX_CALIB_OK) {
                if (corners && lane < 12u) a.pose[(u64)f * 12u + lane] = w.pose_best[(u64)f * 12u + lane];
                if (lane == 12u) {
                    a.frame_cost[f] = corners ? (float)w.cost_best[f] : 0.0f;
                    a.frame_n[f] = corners;
                }
            }
            if (f == 0u && lane == 13u) {
                if (t.status == AGX_CALIB_OK)
                    for (int i = 0; i < 9; ++i) a.camera_out[i] = t.cam_best[i];
                calib_report(t, a.report);
            }
            return;
        }
        if (t.frozen || !corners) return;
    }
    const FitGeom g = pose_geom(a.cols, a.rows, a.first_id, a.spacing_ratio);
    const uint32_t cnt = a.n_tags[f];
    const u64 row0 = (u64)f * a.tags_per_frame;
    if (it == 0u) {  // which frames and rows count, for the whole call
        const bool ok = calib_frame_ok(a.fit_status[f], a.flags) && cnt <= a.tags_per_frame && cnt <= FIT_MAX_ROWS && !(a.tag_status && a.tag_status[f] != AGX_TAGS_OK);
        uint32_t n_inl = 0;
        if (ok) {
            for (uint32_t r = lane; r < cnt; r += 64u) n_inl += calib_row_counts(g, a.tags[row0 + r].id, a.row_status[row0 + r]) ? 1u : 0u;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) n_inl += __shfl_xor(n_inl, m);
        }
        const uint32_t corners = ok && n_inl >= a.min_tags ? 4u * n_inl : 0u;
        if (lane == 0u) w.corners[f] = corners;
        if (!corners) return;
        if (lane < 12u) {
            const double v = a.pose_in[(u64)f * 12u + lane];
            w.pose_cur[(u64)f * 12u + lane] = v;
            w.pose_best[(u64)f * 12u + lane] = v;
        }
    }
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(a.tags + row0);
        for (uint32_t i = lane; i < cnt * 9u; i += 64u) s.rows[i] = src[i];
        for (uint32_t r = lane; r < cnt; r += 64u) s.st[r] = calib_row_counts(g, a.tags[row0 + r].id, a.row_status[row0 + r]) ? 1 : 0;
        calib_wsync();
    }
    Pose pose;
    const double *pin = it == 0u ? a.pose_in + (u64)f * 12u : w.pose_cur + (u64)f * 12u;
#pragma unroll
    for (int i = 0; i < 9; ++i) pose.R[i] = pin[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) pose.t[i] = pin[9 + i];
    agx_camera cam = a.camera;
    if (it > 0u) {
        cam = calib_camera(t.cam);
        if (t.apply) {  // the last launch pair's step: dp_f = z_f - Y_f dc
            calib_pose_step(pose, blk + CALIB_FOLD, t.dc);
            calib_wsync();  // (every lane has read the block's Y and z before any lane stores the new block)
            if (lane == 0u) {
#pragma unroll
                for (int i = 0; i < 9; ++i) w.pose_cur[(u64)f * 12u + i] = pose.R[i];
#pragma unroll
                for (int i = 0; i < 3; ++i) w.pose_cur[(u64)f * 12u + 9u + i] = pose.t[i];
            }
        }
    }
    cam = pose_camera(LENS, cam);  // (w2 of this iterate's xi and alpha)
    const uint32_t held = calib_held(LENS, a.fixed_mask);
    double cost;
    {
        double acc[CALIB_PART_SUMS[0]];
        calib_pass<LENS, 0>(s, cnt, lane, g, a.tag_size, cam, pose, acc);
        cost = acc[45];
        if (lane == 0u) calib_frame_system_u(acc, a.damping, held, s.sys);
    }
    {
        double acc[CALIB_PART_SUMS[1]];
        calib_pass<LENS, 1>(s, cnt, lane, g, a.tag_size, cam, pose, acc);
        if (lane == 0u) calib_frame_system_w(acc, 0, CALIB_W_SPLIT, held, s.sys);
    }
    {
        double acc[CALIB_PART_SUMS[2]];
        calib_pass<LENS, 2>(s, cnt, lane, g, a.tag_size, cam, pose, acc);
        if (lane == 0u) calib_frame_system_w(acc, CALIB_W_SPLIT, CALIB_CAM, held, s.sys);
    }
    {
        double acc[CALIB_PART_SUMS[3]];
        calib_pass<LENS, 3>(s, cnt, lane, g, a.tag_size, cam, pose, acc);
        if (lane == 0u) {
            calib_frame_system_v(acc, a.damping, s.sys);
            s.solved = fit_solve_multi<6, 10>(s.sys.m, s.sys.x) ? 1u : 0u;
        }
    }
    calib_wsync();
    const bool solved = s.solved != 0u;
    if (lane < 54u) blk[lane] = solved ? calib_schur_entry(s.sys, (int)lane) : 0.0;
    else if (lane == 54u) blk[54] = cost;
    else if (lane == 55u) blk[55] = solved ? 0.0 : 1.0;
    if (lane < 60u) {  // Y [6][9], then z [6]
        const uint32_t k = lane / 10u, j = lane - 10u * k;
        blk[CALIB_FOLD + (j < 9u ? 9u * k + j : 54u + k)] = solved ? s.sys.x[lane] : 0.0;
    }
}

struct CalibSolveLds {
    double fold[CALIB_FOLD];
    double m[CALIB_SCRATCH];
};

__global__ void __launch_bounds__(64) k_calib_solve(CalibArgs a, CalibWork w, uint32_t it, int lens)
{
    __shared__ CalibSolveLds s;
    const uint32_t lane = threadIdx.x;
    CalibCtl &t = *w.ctl;
    const uint32_t held = calib_held(lens, a.fixed_mask);
    uint32_t n_usable, frozen;
    if (it == 0u) {  // the usable frames in frame order; AGX_CALIB_FEW
        uint32_t base = 0, corners = 0;
        for (uint32_t f0 = 0; f0 < (uint32_t)a.n_frames; f0 += 64u) {
            const uint32_t f = f0 + lane;
            const uint32_t c = f < (uint32_t)a.n_frames ? w.corners[f] : 0u;
            const u64 mask = __ballot(c != 0u);
            if (c) w.list[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = f;
            base += (uint32_t)__popcll(mask);
            corners += c;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) corners += __shfl_xor(corners, m);
        n_usable = base;
        const bool few = calib_few(n_usable, corners, a.min_frames, held);
        frozen = few ? 1u : 0u;
        if (lane == 0u) {
            const double c9[9] = {a.camera.fx, a.camera.fy, a.camera.cx, a.camera.cy, a.camera.k1, a.camera.k2, a.camera.p1, a.camera.p2, a.camera.k3};
            calib_ctl_init(t, c9);
            t.n_usable = n_usable;
            t.n_corners = corners;
            if (few) t.status = AGX_CALIB_FEW, t.frozen = 1u;
        }
        __threadfence_block();
        __syncthreads();  // (the list is read below by other lanes than wrote it)
    } else {
        n_usable = t.n_usable;
        frozen = t.frozen;
    }
    if (!frozen) {
        double acc[CALIB_FOLD];
#pragma unroll
        for (int k = 0; k < CALIB_FOLD; ++k) acc[k] = 0.0;
        for (uint32_t r = lane; r < n_usable; r += 64u) {
            const double *blk = w.blocks + (u64)w.list[r] * CALIB_BLOCK;
#pragma unroll
            for (int k = 0; k < CALIB_FOLD; ++k) acc[k] += blk[k];
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
            for (int k = 0; k < CALIB_FOLD; ++k) acc[k] += __shfl_xor(acc[k], m);
        if (lane == 0u) {
#pragma unroll
            for (int k = 0; k < CALIB_FOLD; ++k) s.fold[k] = acc[k];
        }
    }
    if (lane == 0u) calib_step(t, it, a.iterations, lens, held, s.fold, s.m);  // (frozen: it only clears the two marks)
}

}  // namespace

size_t calib_work_bytes(int n_frames)
{
    const size_t n = (size_t)n_frames;
    return sizeof(CalibCtl) + n * (CALIB_BLOCK + 12 + 12 + 1) * sizeof(double) + n * 2 * sizeof(uint32_t);
}

CalibWork calib_work(void *base, int n_frames)
{
    const size_t n = (size_t)n_frames;
    CalibWork w;
    char *p = static_cast<char *>(base);
    w.ctl = reinterpret_cast<CalibCtl *>(p);
    p += sizeof(CalibCtl);
    w.blocks = reinterpret_cast<double *>(p);
    w.pose_cur = w.blocks + n * CALIB_BLOCK;
    w.pose_best = w.pose_cur + n * 12;
    w.cost_best = w.pose_best + n * 12;
    w.corners = reinterpret_cast<uint32_t *>(w.cost_best + n);
    w.list = w.corners + n;
    return w;
}
static_assert(sizeof(CalibCtl) % 8 == 0, "the workspace's doubles follow CalibCtl");

int launch_calibrate(const CalibArgs &a, int lens, void *work, void *stream)
{
    if (calib_args_bad(a, lens) || !work) return (int)hipErrorInvalidValue;
    const CalibWork w = calib_work(work, a.n_frames);
    const unsigned grid = ((unsigned)a.n_frames + CALIB_FRAMES_PER_WG - 1) / CALIB_FRAMES_PER_WG;
    const auto blocks = [&](uint32_t it, int finish) {
        with_lens(lens, [&](auto L) {
            hipLaunchKernelGGL(k_calib_blocks<decltype(L)::value>, dim3(grid), dim3(64 * CALIB_FRAMES_PER_WG), 0, (hipStream_t)stream, a, w, it, finish);
        });
    };
    for (uint32_t it = 0; it <= a.iterations; ++it) {
        blocks(it, 0);
        hipLaunchKernelGGL(k_calib_solve, dim3(1), dim3(64), 0, (hipStream_t)stream, a, w, it, lens);
    }
    blocks(a.iterations + 1u, 1);
    return (int)hipGetLastError();
}

}  // namespace agx
