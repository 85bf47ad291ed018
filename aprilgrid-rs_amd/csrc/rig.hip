// rig.hip -- k_rig_blocks, k_rig_instants and k_rig_solve (agx_rig_calibrate_enqueue): the extrinsics E_c of a rig's cameras and
// the board's pose T_s at every usable instant from synchronised tag tables, by damped Gauss-Newton with the T_s eliminated instant
// by instant.  Every number is rig_math.h's, which the host form (rig_host.cpp) runs too: the two give the same bytes.
// k_rig_blocks(it): one wave per frame f = c n_instants + s, RIG_FRAMES_PER_WG frames per workgroup, the waves never meet.  At
// iterate 0 the wave decides which frames of its instant are usable (calib_frame_ok, calib_row_counts, min_tags), whether the
// instant is (min_cams) and the instant's seed E_c^-1 o pose_in[c, s] of its lowest usable camera; camera 0's wave stores them.
// The rows are staged in LDS as k_calib_blocks stages them; the 91 sums of a camera c >= 1 are taken in three passes (33, 30 and
// 28 sums in registers, folded by shuffles), camera 0's 28 in one.  The lens is uniform across the wave: one kernel, a switch over
// the three instantiations.
// k_rig_instants(it): one wave per usable instant.  It sums V_s, its gradient and the cost over the instant's frames, builds the
// 6 x (6 n_cams + 1) system in LDS, lane 0 eliminates it, and the lanes store the instant's contribution to the reduced system and
// the back-substitution rows Y_s, z_s.
// k_rig_solve(it): one wave in all.  At iterate 0 it lists the usable instants (ballot), counts frames and corners per camera and
// decides AGX_RIG_FEW.  Then lane l adds the contributions of the usable instants of rank l, l + 64, .. (RIG_FOLD_CHUNK entries
// at a time in registers, the folded entries into LDS), lane 0 runs rig_step on them in LDS (the best-iterate rule, the scaled
// reduced solve, the E_c's update), and the lanes keep the best iterate's T_s and frame costs and apply dT_s = z_s - Y_s dE.  The
// last launch writes the outputs.  No floating-point atomics, no scratch; nothing returns to the host.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rig.h"
#include "rig_math.h"

namespace agx {
namespace {

using u64 = unsigned long long;

struct RigFrameLds {
    uint32_t rows[FIT_MAX_ROWS * 9];  // the frame's tag rows as they stand in the table
    uint8_t st[FIT_MAX_ROWS];         // 1: an inlier row on the board
};
static_assert(sizeof(RigFrameLds) * RIG_FRAMES_PER_WG <= 65536, "k_rig_blocks: static LDS");

// LDS written by some lanes of this wave, read by others: order the accesses (no workgroup barrier: the waves run apart)
__device__ __forceinline__ void rig_wsync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// 4 x the inlier rows on the board of frame f, 0 for a frame that is not usable; the same value in every lane
__device__ __forceinline__ uint32_t rig_frame_corners(const RigArgs &a, const FitGeom &g, uint32_t f, uint32_t lane)
{
    const uint32_t cnt = a.n_tags[f];
    const u64 row0 = (u64)f * a.tags_per_frame;
    const bool ok = calib_frame_ok(a.fit_status[f], a.flags) && cnt <= a.tags_per_frame && cnt <= FIT_MAX_ROWS && !(a.tag_status && a.tag_status[f] != AGX_TAGS_OK);
    if (!ok) return 0u;  // (the whole wave)
    uint32_t n_inl = 0;
    for (uint32_t r = lane; r < cnt; r += 64u) n_inl += calib_row_counts(g, a.tags[row0 + r].id, a.row_status[row0 + r]) ? 1u : 0u;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) n_inl += __shfl_xor(n_inl, m);
    return n_inl >= a.min_tags ? 4u * n_inl : 0u;
}

// one pass over the staged rows: part PART's sums of the frame (FREE: a camera c >= 1; else camera 0's 28), folded, stored by lane 0
template <int LENS, int PART, bool FREE>
__device__ __forceinline__ void rig_pass(const RigFrameLds &s, uint32_t cnt, uint32_t lane, const FitGeom &g, double tag_size, const agx_camera &cam,
                                         const Pose &e, const Pose &t, const Pose &p, double *blk)
{
    constexpr int N = RIG_PART_SUMS[PART];
    double acc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0;
    for (uint32_t r = lane; r < cnt; r += 64u) {
        if (!s.st[r]) continue;
        float xy[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) xy[j] = f32_from_bits(s.rows[9u * r + 1 + j]);
        if constexpr (FREE) rig_accumulate_row<LENS, PART>(g, tag_size, cam, e, t, p, acc, s.rows[9u * r], xy);
        else pose_accumulate_row<LENS>(g, tag_size, cam, t, acc, s.rows[9u * r], xy);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k] += __shfl_xor(acc[k], m);
    if (lane == 0u) {
#pragma unroll
        for (int k = 0; k < N; ++k) blk[rig_part_slot(PART, k)] = acc[k];
    }
}

template <int LENS>
__device__ __forceinline__ void rig_frame(const RigFrameLds &s, uint32_t cnt, uint32_t lane, const FitGeom &g, double tag_size, const agx_camera &camera, int c,
                                          const Pose &e, const Pose &t, double *blk)
{
    const agx_camera cam = pose_camera(LENS, camera);
    if (c == 0) {  // (the whole wave)
        rig_pass<LENS, 2, false>(s, cnt, lane, g, tag_size, cam, e, t, t, blk);
        return;
    }
    const Pose p = rig_compose(e, t);
    rig_pass<LENS, 0, true>(s, cnt, lane, g, tag_size, cam, e, t, p, blk);
    rig_pass<LENS, 1, true>(s, cnt, lane, g, tag_size, cam, e, t, p, blk);
    rig_pass<LENS, 2, true>(s, cnt, lane, g, tag_size, cam, e, t, p, blk);
}

__global__ void __launch_bounds__(64 * RIG_FRAMES_PER_WG) k_rig_blocks(RigArgs a, RigWork w, uint32_t it)
{
    __shared__ RigFrameLds lds[RIG_FRAMES_PER_WG];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t f = blockIdx.x * RIG_FRAMES_PER_WG + wave;
    const uint32_t S = (uint32_t)a.n_instants, nf = (uint32_t)a.n_cams * S;
    if (f >= nf) return;  // (the whole wave)
    RigFrameLds &s = lds[wave];
    const RigCtl &t = *w.ctl;  // (written by k_rig_solve only: it == 0 reads nothing of it)
    const uint32_t c = f / S, si = f - c * S;
    const FitGeom g = pose_geom(a.cols, a.rows, a.first_id, a.spacing_ratio);
    // every branch below is taken by the whole wave
    Pose e, T;
    if (it == 0u) {  // which frames and instants count, for the whole call; the instant's seed
        uint32_t mine = 0, n_ok = 0;
        int low = -1;
        for (uint32_t k = 0; k < (uint32_t)a.n_cams; ++k) {
            const uint32_t raw = rig_frame_corners(a, g, k * S + si, lane);
            if (k == c) mine = raw;
            if (raw) {
                ++n_ok;
                if (low < 0) low = (int)k;
            }
        }
        const bool ok = n_ok >= a.min_cams;
        const uint32_t corners = ok ? mine : 0u;
        if (lane == 0u) w.corners[f] = corners;
        if (ok) T = rig_seed_instant(low, rig_load(a.ext_in + 12 * low), rig_load(a.pose_in + ((u64)(uint32_t)low * S + si) * 12u));
        if (c == 0u && lane == 0u) {
            w.inst_ok[si] = ok ? 1u : 0u;
            if (ok) {
                rig_store(w.t_cur + (u64)si * 12u, T);
                rig_store(w.t_best + (u64)si * 12u, T);
            }
        }
        if (!corners) return;
        e = c == 0u ? rig_identity() : rig_load(a.ext_in + 12u * c);
    } else {
        if (t.frozen || !w.corners[f]) return;
        e = rig_load(t.ext[c]);
        T = rig_load(w.t_cur + (u64)si * 12u);
    }
    const uint32_t cnt = a.n_tags[f];
    const u64 row0 = (u64)f * a.tags_per_frame;
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(a.tags + row0);
        for (uint32_t i = lane; i < cnt * 9u; i += 64u) s.rows[i] = src[i];
        for (uint32_t r = lane; r < cnt; r += 64u) s.st[r] = calib_row_counts(g, a.tags[row0 + r].id, a.row_status[row0 + r]) ? 1 : 0;
        rig_wsync();
    }
    double *blk = w.frames + (u64)f * RIG_FRAME;
    const int lens = a.lens[c];
    if (lens == AGX_LENS_DOUBLE_SPHERE) rig_frame<AGX_LENS_DOUBLE_SPHERE>(s, cnt, lane, g, a.tag_size, a.camera[c], (int)c, e, T, blk);
    else if (lens == AGX_LENS_EQUIDISTANT) rig_frame<AGX_LENS_EQUIDISTANT>(s, cnt, lane, g, a.tag_size, a.camera[c], (int)c, e, T, blk);
    else rig_frame<AGX_LENS_RADTAN>(s, cnt, lane, g, a.tag_size, a.camera[c], (int)c, e, T, blk);
}

struct RigInstantLds {
    double m[6 * RIG_MAX_W];
    double x[6 * (RIG_MAX_N + 1)];
    double sum28[POSE_SUMS];
    uint32_t solved, pad;
};

__global__ void __launch_bounds__(64 * RIG_INSTANTS_PER_WG) k_rig_instants(RigArgs a, RigWork w, uint32_t it)
{
    __shared__ RigInstantLds lds[RIG_INSTANTS_PER_WG];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t si = blockIdx.x * RIG_INSTANTS_PER_WG + wave;
    const uint32_t S = (uint32_t)a.n_instants;
    if (si >= S) return;  // (the whole wave)
    if (it > 0u && w.ctl->frozen) return;
    if (!w.inst_ok[si]) return;
    RigInstantLds &s = lds[wave];
    const int C = a.n_cams, n = rig_n(C), nt = rig_tri(n), FL = rig_fold_len(C), W = 6 * C + 1, M = n + 1;
    const auto blk = [&](int c) -> const double * {
        const u64 f = (u64)(uint32_t)c * S + si;
        return w.corners[f] ? w.frames + f * RIG_FRAME : nullptr;
    };
    if (lane < (uint32_t)POSE_SUMS) s.sum28[lane] = rig_instant_sum(C, blk, (int)lane);
    rig_wsync();
    for (int e = (int)lane; e < 6 * W; e += 64) {
        const int k = e / W, col = e - W * k;
        s.m[e] = rig_instant_entry(C, blk, s.sum28, a.damping, k, col);
    }
    rig_wsync();
    if (lane == 0u) s.solved = rig_eliminate(C, s.m, s.x) ? 1u : 0u;
    rig_wsync();
    const bool solved = s.solved != 0u;
    double *ib = w.instants + (u64)si * (u64)rig_block_len(C);
    for (int e = (int)lane; e < nt + n; e += 64) ib[e] = solved ? rig_schur_entry(C, blk, s.x, a.damping, e) : 0.0;
    if (lane == 0u) {
        ib[nt + n] = s.sum28[27];
        ib[nt + n + 1] = solved ? 0.0 : 1.0;
    }
    for (int e = (int)lane; e < 6 * M; e += 64) {
        const int k = e / M, j = e - M * k;
        ib[FL + (j < n ? n * k + j : 6 * n + k)] = solved ? s.x[e] : 0.0;
    }
}

struct RigSolveLds {
    double fold[RIG_MAX_N * (RIG_MAX_N + 1) / 2 + RIG_MAX_N + 2 + RIG_FOLD_CHUNK];
    double m[RIG_SCRATCH];
};

__global__ void __launch_bounds__(64) k_rig_solve(RigArgs a, RigWork w, uint32_t it)
{
    __shared__ RigSolveLds s;
    const uint32_t lane = threadIdx.x;
    RigCtl &t = *w.ctl;
    const int C = a.n_cams, n = rig_n(C), FL = rig_fold_len(C), BL = rig_block_len(C);
    const uint32_t S = (uint32_t)a.n_instants, nf = (uint32_t)C * S;
    if (it == 0u) {  // the usable instants in instant order; the counts; AGX_RIG_FEW
        uint32_t base = 0;
        for (uint32_t s0 = 0; s0 < S; s0 += 64u) {
            const uint32_t si = s0 + lane;
            const bool ok = si < S && w.inst_ok[si] != 0u;
            const u64 mask = __ballot(ok);
            if (ok) w.list[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = si;
            base += (uint32_t)__popcll(mask);
        }
        if (lane == 0u) {
            rig_ctl_init(t, C, a.ext_in);
            t.n_instants_used = base;
        }
        for (int c = 0; c < C; ++c) {
            uint32_t frames = 0, corners = 0;
            for (uint32_t si = lane; si < S; si += 64u) {
                const uint32_t k = w.corners[(u64)(uint32_t)c * S + si];
                frames += k ? 1u : 0u;
                corners += k;
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                frames += __shfl_xor(frames, m);
                corners += __shfl_xor(corners, m);
            }
            if (lane == 0u) {
                t.cam_n[c] = frames;
                t.n_frames_used += frames;
                t.n_corners += corners;
                if (c >= 1) {
                    if (frames) ++t.n_cams_free;
                    else t.held |= 1u << c;
                }
            }
        }
        if (lane == 0u && rig_few(t.n_instants_used, t.n_cams_free, t.n_corners, a.min_instants)) t.status = AGX_RIG_FEW, t.frozen = 1u;
        __threadfence_block();
        __syncthreads();  // (the list and the state are read below by other lanes than wrote them)
    }
    const uint32_t n_used = t.n_instants_used;
    if (!t.frozen) {
        for (int e0 = 0; e0 < FL; e0 += RIG_FOLD_CHUNK) {
            double acc[RIG_FOLD_CHUNK];
#pragma unroll
            for (int k = 0; k < RIG_FOLD_CHUNK; ++k) acc[k] = 0.0;
            for (uint32_t r = lane; r < n_used; r += 64u) {
                const double *ib = w.instants + (u64)w.list[r] * (u64)BL + e0;
#pragma unroll
                for (int k = 0; k < RIG_FOLD_CHUNK; ++k) acc[k] += ib[k];  // (past FL: the block's Y and z, 6 n + 6 >= RIG_FOLD_CHUNK doubles, summed and not used)
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
                for (int k = 0; k < RIG_FOLD_CHUNK; ++k) acc[k] += __shfl_xor(acc[k], m);
            if (lane == 0u) {
#pragma unroll
                for (int k = 0; k < RIG_FOLD_CHUNK; ++k) s.fold[e0 + k] = acc[k];  // (fold has RIG_FOLD_CHUNK entries to spare)
            }
        }
    }
    if (lane == 0u) rig_step(t, it, a.iterations, C, s.fold, s.m);  // (frozen: it only clears the two marks)
    __threadfence_block();
    __syncthreads();
    if (t.mark_best) {  // this iterate is the best so far: keep its T_s and frame costs
        for (uint32_t r = lane; r < n_used; r += 64u) {
            const u64 si = w.list[r];
            for (int i = 0; i < 12; ++i) w.t_best[si * 12u + i] = w.t_cur[si * 12u + i];
        }
        for (uint32_t f = lane; f < nf; f += 64u)
            if (w.corners[f]) w.cost_best[f] = w.frames[(u64)f * RIG_FRAME + 90u];
    }
    if (t.apply) {  // dT_s = z_s - Y_s dE
        for (uint32_t r = lane; r < n_used; r += 64u) {
            const u64 si = w.list[r];
            Pose T = rig_load(w.t_cur + si * 12u);
            rig_instant_step(T, n, w.instants + si * (u64)BL + FL, t.de);
            rig_store(w.t_cur + si * 12u, T);
        }
    }
    if (it != a.iterations) return;
    if (t.status == AGX_RIG_OK) {  // the outputs (each lane reads back only what it wrote above)
        for (uint32_t r = lane; r < n_used; r += 64u) {
            const u64 si = w.list[r];
            for (int i = 0; i < 12; ++i) a.rig_pose[si * 12u + i] = w.t_best[si * 12u + i];
        }
        for (uint32_t f = lane; f < nf; f += 64u) {
            const uint32_t k = w.corners[f];
            a.frame_cost[f] = k ? (float)w.cost_best[f] : 0.0f;
            a.frame_n[f] = k;
        }
        for (uint32_t i = lane; i < 12u * (uint32_t)C; i += 64u) a.ext[i] = t.ext_best[i / 12u][i % 12u];
        if (lane < (uint32_t)C) a.cam_n[lane] = t.cam_n[lane];
    }
    if (lane == 0u) rig_report(t, a.report);
}

}  // namespace

static_assert(6 * 6 * (RIG_MIN_CAMS - 1) + 6 >= RIG_FOLD_CHUNK, "k_rig_solve's last chunk stays inside the instant's block");
static_assert(sizeof(RigCtl) % 8 == 0, "the workspace's doubles follow RigCtl");

size_t rig_work_bytes(int n_cams, int n_instants)
{
    const size_t s = (size_t)n_instants, f = (size_t)n_cams * s;
    return sizeof(RigCtl) + (f * (RIG_FRAME + 1) + s * ((size_t)rig_block_len(n_cams) + 24)) * sizeof(double) + (f + 2 * s) * sizeof(uint32_t);
}

RigWork rig_work(void *base, int n_cams, int n_instants)
{
    const size_t s = (size_t)n_instants, f = (size_t)n_cams * s;
    RigWork w;
    char *p = static_cast<char *>(base);
    w.ctl = reinterpret_cast<RigCtl *>(p);
    p += sizeof(RigCtl);
    w.frames = reinterpret_cast<double *>(p);
    w.instants = w.frames + f * RIG_FRAME;
    w.t_cur = w.instants + s * (size_t)rig_block_len(n_cams);
    w.t_best = w.t_cur + s * 12;
    w.cost_best = w.t_best + s * 12;
    w.corners = reinterpret_cast<uint32_t *>(w.cost_best + f);
    w.inst_ok = w.corners + f;
    w.list = w.inst_ok + s;
    return w;
}

int launch_rig_calibrate(const RigArgs &a, void *work, void *stream)
{
    if (rig_args_bad(a, false) || !work) return (int)hipErrorInvalidValue;
    const RigWork w = rig_work(work, a.n_cams, a.n_instants);
    const unsigned nf = (unsigned)a.n_cams * (unsigned)a.n_instants;
    const unsigned grid_f = (nf + RIG_FRAMES_PER_WG - 1) / RIG_FRAMES_PER_WG, grid_s = ((unsigned)a.n_instants + RIG_INSTANTS_PER_WG - 1) / RIG_INSTANTS_PER_WG;
    for (uint32_t it = 0; it <= a.iterations; ++it) {
        hipLaunchKernelGGL(k_rig_blocks, dim3(grid_f), dim3(64 * RIG_FRAMES_PER_WG), 0, (hipStream_t)stream, a, w, it);
        hipLaunchKernelGGL(k_rig_instants, dim3(grid_s), dim3(64 * RIG_INSTANTS_PER_WG), 0, (hipStream_t)stream, a, w, it);
        hipLaunchKernelGGL(k_rig_solve, dim3(1), dim3(64), 0, (hipStream_t)stream, a, w, it);
    }
    return (int)hipGetLastError();
}

}  // namespace agx
