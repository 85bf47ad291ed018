// detector.cpp -- implementation of the C ABI in include/aprilgrid_amd.h: the detector handle
// (mirror of aprilgrid::detector::TagDetector), device workspace, chain enqueue / fetch,
// profiling events and the parity-test hooks.  Compiled by hipcc; links only libamdhip64.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <system_error>
#include <vector>

#include "../../include/aprilgrid_amd.h"
#include "board_fit.h"
#include "board_fit_math.h"
#include "board_pose.h"
#include "board_pose_math.h"
#include "calibrate.h"
#include "rig.h"
#include "rig_math.h"
#include "chain_kernels.h"
#include "decimate.h"
#include "decode_math.h"
#include "decode_stages.h"
#include "detector_internal.h"
#include "host_tail.hpp"
#include "rectify.h"
#include "render.h"
#include "tail_kernels.h"

using namespace agx;

int agx::fail(agx_detector *d, int status, const std::string &msg)
{
    if (d) d->last_error = msg;
    return status;
}

// The enqueue / fetch pair of every kind of batch (BatchKind), for the refusals of the other pairs' fetches
static const struct { const char *enqueue, *fetch; } kBatchPair[BATCH_KINDS] = {
    {nullptr, nullptr},
    {"agx_saddles_batch_enqueue", "agx_saddles_batch_fetch"},
    {"agx_detect_batch_enqueue", "agx_detect_batch_fetch"},
    {"agx_refine_points_enqueue", "agx_refine_points_fetch"},
    {"agx_decode_quads_enqueue", "agx_decode_quads_fetch"},
    {"agx_find_boards_enqueue", "agx_find_boards_fetch"},
    {"agx_clusters_enqueue", "agx_clusters_fetch"},
    {"agx_grow_boards_enqueue", "agx_grow_boards_fetch"},
    {"agx_init_quads_enqueue", "agx_init_quads_fetch"}};

int agx::refuse_other_batch(agx_detector *det, int wanted)
{
    const int have = det->batch;
    if (have == wanted) return AGX_OK;
    if (have == BATCH_NONE) return fail(det, AGX_ERR_STATE, std::string("no ") + kBatchPair[wanted].enqueue + " batch in flight");
    return fail(det, AGX_ERR_STATE, std::string("the batch in flight is ") + kBatchPair[have].enqueue + "'s: fetch it with " + kBatchPair[have].fetch);
}

// AGX_OK for an agx_format (lf32: AGX_LF32 among them), else AGX_ERR_FORMAT
static int check_format(agx_detector *det, int format, bool lf32)
{
    if (format_px_bytes(format) && (lf32 || format != AGX_LF32)) return AGX_OK;
    return fail(det, AGX_ERR_FORMAT, lf32 ? "format must be one of AGX_L8 .. AGX_RGBA16 (agx_format)"
                                          : "format must be one of AGX_L8 .. AGX_RGBA16 but AGX_LF32 (the decode reads to_luma8)");
}

int agx::check_frame_batch(agx_detector *det, const FrameBatch &b, const BatchRules &rules)
{
    if (!b.frames || b.n_frames <= 0) return fail(det, AGX_ERR_ARG, "null frames or n_frames <= 0");
    if (const int rc = check_format(det, b.format, rules.lf32)) return rc;
    const size_t px_bytes = (size_t)format_px_bytes(b.format);
    if (b.width < rules.min_side || b.height < rules.min_side)
        return fail(det, AGX_ERR_ARG, "width and height must be >= " + std::to_string(rules.min_side));
    if ((long long)b.width * b.height >= (1ll << 30) || b.width > 65000) return fail(det, AGX_ERR_ARG, "frame too large (>= 2^30 px or wider than 65000)");
    if (b.n_frames > 65535) return fail(det, AGX_ERR_ARG, "at most 65535 frames per batch");
    // (the kernels take the row stride as an int)
    if (b.row_stride < (size_t)b.width * px_bytes || b.row_stride > 0x7fffffffu ||
        (b.n_frames > 1 && b.frame_stride < b.row_stride * format_rows(b.format, b.height)))
        return fail(det, AGX_ERR_ARG, "strides must cover a row / a frame");
    const size_t low_bits = b.row_stride | (uintptr_t)b.frames | (b.n_frames > 1 || rules.lone_frame_stride ? b.frame_stride : 0);
    if (rules.align16 && format_16bit(b.format) && (low_bits & 1)) return fail(det, AGX_ERR_ARG, "16-bit pixels must be 2-byte aligned");
    if (b.format == AGX_LF32 && (low_bits & 3)) return fail(det, AGX_ERR_ARG, "f32 pixels must be 4-byte aligned");
    if (rules.front_rows && format_front(b.format) && b.height > 16 * 65535)  // (k_front_luma's grid: 16 rows per workgroup, 65535 workgroups)
        return fail(det, AGX_ERR_ARG, "frames of this format may have at most 1048560 rows");
    return AGX_OK;
}

namespace {

const char *kKernelNames[K_COUNT] = {"k_blur_hessian", "k_verify_seeds", "k_flood_refine", "k_rare_emit", "k_sparse_frame"};

thread_local std::string g_create_error;  // reason of this thread's last failed agx_detector_create (det == NULL)

// Nothing unwinds across the C boundary (include/aprilgrid_amd.h, "Conventions"): every entry point runs its body through
// agx_guard.  A failed host allocation or thread creation becomes AGX_ERR_NOMEM, anything else AGX_ERR_STATE; the message
// goes to agx_last_error (best effort: storing it must not throw either).  Visible, like the reference's panic
// (src/detector.rs:500) -- and recoverable, unlike an exception that reaches a Rust frame.
void set_error_noexcept(agx_detector *d, const char *msg) noexcept
{
    try {
        if (d) d->last_error = msg;
        else g_create_error = msg;
    } catch (...) {
    }
}

template <typename F>
int agx_guard(const agx_detector *det_c, F &&body) noexcept
{
    agx_detector *det = const_cast<agx_detector *>(det_c);
    try {
        return body();
    } catch (const std::bad_alloc &) {
        set_error_noexcept(det, "out of host memory");
        return AGX_ERR_NOMEM;
    } catch (const std::system_error &e) {  // std::thread: no more threads / resources
        set_error_noexcept(det, e.what());
        return AGX_ERR_NOMEM;
    } catch (const std::exception &e) {
        set_error_noexcept(det, e.what());
        return AGX_ERR_STATE;
    } catch (...) {
        set_error_noexcept(det, "unknown exception");
        return AGX_ERR_STATE;
    }
}

// Blur taps, reference src/image_util.rs:111-124 (sigma = 1.5 at the call site detector.rs:410: radius 3, seven taps): the
// 2 * radius + 1 taps into w, which has room for them.  Returns the radius.
int blur_radius(float sigma) { return (int)std::ceil(sigma * 2.0f); }
int make_blur_weights(float sigma, float *w)
{
    const int radius = blur_radius(sigma);
    const float two_sigma_sq = 2.0f * sigma * sigma;
    float sum = 0.0f;
    for (int i = 0; i < 2 * radius + 1; ++i) {
        const float x = (float)(i - radius);
        const float v = std::exp(-(x * x) / two_sigma_sq);
        w[i] = v;
        sum += v;
    }
    for (int i = 0; i < 2 * radius + 1; ++i) w[i] /= sum;
    return radius;
}

// a sigma agx_planes_enqueue / agx_debug_blur_weights can blur with: finite, positive, at most GB_MAX_RADIUS
bool blur_sigma_ok(float sigma) { return std::isfinite(sigma) && sigma > 0.0f && std::ceil(sigma * 2.0f) <= (float)GB_MAX_RADIUS; }

// Constants of rochade_refine at half_size_patch = half in 1 .. REFINE_PATCH_MAX_HALF, ks = 2*half+1: cone kernel (:240-254)
// and the ks*ks x 6 pseudo-inverse of the quadratic design matrix (:208-237).  The design's normal matrix is block diagonal
// on the symmetric ks x ks grid (odd moments vanish): {xy}, {x}, {y} decouple and {x^2, y^2, 1} is a 3x3 block, inverted
// here by its adjugate in binary64 (every intermediate is an integer far below 2^53 for these sizes, so the quotient is that
// of the exact numerator and determinant); one rounding to binary32.
static void refine_consts_at(int half, float *cone, float *pmat)
{
    const int ks = 2 * half + 1;
    double sx2 = 0, sx4 = 0;
    for (int c = 0; c < ks; ++c) {
        const double x = c - half;
        sx2 += x * x;
        sx4 += x * x * x * x;
    }
    const double n1 = ks;
    // moments over the grid
    const double m_x4 = n1 * sx4, m_x2y2 = sx2 * sx2, m_x2 = n1 * sx2, m_1 = n1 * n1;
    // block {x^2, y^2, 1}
    const double B[3][3] = {{m_x4, m_x2y2, m_x2}, {m_x2y2, m_x4, m_x2}, {m_x2, m_x2, m_1}};
    double adj[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int r0 = (j + 1) % 3, r1 = (j + 2) % 3, c0 = (i + 1) % 3, c1 = (i + 2) % 3;
            adj[i][j] = B[r0][c0] * B[r1][c1] - B[r0][c1] * B[r1][c0];
        }
    const double det = B[0][0] * adj[0][0] + B[0][1] * adj[1][0] + B[0][2] * adj[2][0];
    int i = 0;
    for (int r = 0; r < ks; ++r)
        for (int c = 0; c < ks; ++c, ++i) {
            const double x = c - half, y = r - half;
            const double q[3] = {x * x, y * y, 1.0};
            double blk[3];
            for (int a = 0; a < 3; ++a) blk[a] = (adj[a][0] * q[0] + adj[a][1] * q[1] + adj[a][2] * q[2]) / det;
            pmat[i * 6 + 0] = (float)blk[0];          // x^2
            pmat[i * 6 + 1] = (float)(x * y / m_x2y2 + 0.0); // xy (+0.0: no negative zeros)
            pmat[i * 6 + 2] = (float)blk[1];          // y^2
            pmat[i * 6 + 3] = (float)(x / m_x2 + 0.0);      // x
            pmat[i * 6 + 4] = (float)(y / m_x2 + 0.0);      // y
            pmat[i * 6 + 5] = (float)blk[2];          // 1
        }
    const float gamma = (float)half;
    float s = 0.0f;
    for (int a = 0; a < ks; ++a)
        for (int b = 0; b < ks; ++b) {
            const float da = gamma - (float)a, db = gamma - (float)b;
            cone[a * ks + b] = std::max(0.0f, gamma + 1.0f - std::sqrt(da * da + db * db));
        }
    for (int a = 0; a < ks * ks; ++a) s += cone[a];
    for (int a = 0; a < ks * ks; ++a) cone[a] = cone[a] / s;
}

// half_size_patch = 2, the value the chain's own refinement passes (detector.rs:430)
void make_refine_consts(RefineConsts &rc) { refine_consts_at(2, rc.cone, rc.pmat); }

void make_refine_patch_consts(int half, RefinePatchConsts &rc)
{
    rc = RefinePatchConsts{};
    refine_consts_at(half, rc.cone, rc.pmat);
}

template <typename T>
int dev_alloc(agx_detector *d, T *&ptr, size_t count)
{
    void *p = nullptr;
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T), rz = d->redzone;
    HIP_TRY(d, hipMalloc(&p, bytes + 2 * rz));
    d->device_allocs.push_back(p);
    d->alloc_bytes.push_back(bytes);
    if (rz) {
        HIP_TRY(d, hipMemset(p, 0xA5, rz));
        HIP_TRY(d, hipMemset((char *)p + rz + bytes, 0xA5, rz));
    }
    ptr = (T *)((char *)p + rz);
    return AGX_OK;
}

}  // namespace

// The side buffers (detector_internal.h): guard bytes around each, like the workspace's
void agx::side_free(agx_detector *d, int which)
{
    SideBuf &b = d->side[which];
    if (b.base) (void)(b.host ? hipHostFree(b.base) : hipFree(b.base));
    b = SideBuf();
}
void *agx::side_ensure(agx_detector *d, int which, size_t bytes, int kind)
{
    SideBuf &b = d->side[which];
    if (b.base && b.bytes >= bytes) return b.payload;
    const bool idle = hipSetDevice(d->device) == hipSuccess && hipStreamSynchronize(d->stream) == hipSuccess;
    side_free(d, which);
    if (!idle) return nullptr;
    const size_t rz = d->redzone, payload = std::max<size_t>(bytes, 1);
    void *p = nullptr, *dp = nullptr;
    if (kind == 0) {
        if (hipMalloc(&p, payload + 2 * rz) != hipSuccess) return nullptr;
        if (rz && (hipMemset(p, 0xA5, rz) != hipSuccess || hipMemset((char *)p + rz + payload, 0xA5, rz) != hipSuccess)) {
            (void)hipFree(p);
            return nullptr;
        }
    } else {
        if (hipHostMalloc(&p, payload + 2 * rz, kind == 2 ? hipHostMallocMapped : hipHostMallocDefault) != hipSuccess) return nullptr;
        if (rz) {
            std::memset(p, 0xA5, rz);
            std::memset((char *)p + rz + payload, 0xA5, rz);
        }
        if (kind == 2 && hipHostGetDevicePointer(&dp, p, 0) != hipSuccess) {
            (void)hipHostFree(p);
            return nullptr;
        }
    }
    b.base = p;
    b.payload = (char *)p + rz;
    b.mapped = dp ? (char *)dp + rz : nullptr;
    b.bytes = payload;
    b.host = kind != 0;
    return b.payload;
}
bool agx::side_ensure_pair(agx_detector *d, int a, size_t bytes_a, int kind_a, int b, size_t bytes_b, int kind_b)
{
    if (side_ensure(d, a, bytes_a, kind_a) && side_ensure(d, b, bytes_b, kind_b)) return true;
    side_free(d, a);
    side_free(d, b);
    return false;
}

namespace {

void free_workspace(agx_detector *d)
{
    for (void *p : d->device_allocs) (void)hipFree(p);
    d->device_allocs.clear();
    d->alloc_bytes.clear();
    d->cap_frames = 0;
    d->cap_plane = 0;
    d->d_ctr[0] = d->d_ctr[1] = nullptr;
    d->ctr_cleared[0] = d->ctr_cleared[1] = 0;
    if (d->h_ctr) (void)hipHostFree(d->h_ctr);
    if (d->h_out) (void)hipHostFree(d->h_out);
    d->h_ctr = nullptr;
    d->h_out = nullptr;
    d->h_ctr_frames = 0;
    d->h_out_records = 0;
}

uint32_t clamp_u32(unsigned long long v, uint32_t lo, uint32_t hi)
{
    return (uint32_t)std::min<unsigned long long>(std::max<unsigned long long>(v, lo), hi);
}

size_t mask_words_per_frame(int W, int H) { return (size_t)((W + 2 * MASK_PAD_X + 3) & ~3) * (size_t)(H / 32 + 4); }

// The mask's pad words / pad rows are never written by the kernels and must read as zero: the
// plane is cleared whenever the frame geometry (hence the mask layout) changes.
int set_mask_geometry(agx_detector *d, int W, int H)
{
    ChainArgs &a = d->args;
    a.mask_wpr = (W + 2 * MASK_PAD_X + 3) & ~3;
    a.mask_yb = H / 32 + 4;
    a.mask_plane = (long long)a.mask_wpr * a.mask_yb;
    if (d->ws_W != W || d->ws_H != H) {
        HIP_TRY(d, hipMemsetAsync(a.mask, 0, d->mask_words * sizeof(uint32_t), d->stream));
        d->ws_W = W;
        d->ws_H = H;
    }
    return AGX_OK;
}

// (Re)allocate the workspace for n_frames frames of W x H.  Never called inside a timed
// region once a configuration has been seen.
int ensure_workspace(agx_detector *d, int n_frames, int W, int H)
{
    const long long plane = (long long)W * H;
    const uint32_t cap_cand = d->lim_cand ? d->lim_cand : clamp_u32((unsigned long long)plane / 2, 4096, 1u << 28);
    const uint32_t cap_roots = d->lim_roots ? d->lim_roots : clamp_u32((unsigned long long)plane / 8, 1024, 1u << 26);
    const uint32_t cap_out = d->lim_out ? d->lim_out : clamp_u32((unsigned long long)plane / 64, 256, 1u << 24);
    ChainArgs &a = d->args;
    const bool fits = (size_t)n_frames <= d->cap_frames && plane <= d->cap_plane && cap_cand <= d->alloc_cand &&
                      cap_roots <= d->alloc_roots && cap_out <= d->alloc_out &&
                      (size_t)n_frames * mask_words_per_frame(W, H) <= d->mask_words;
    if (fits) {
        a.cap_cand = cap_cand;
        a.cap_roots = cap_roots;
        a.cap_out = cap_out;
        return set_mask_geometry(d, W, H);
    }
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    free_workspace(d);
    const size_t F = (size_t)n_frames;
    int rc;
    const size_t mask_plane = mask_words_per_frame(W, H);
    if ((rc = dev_alloc(d, a.blur, F * plane + 16))) return rc;  // +16: aligned window loads may touch 3 floats past the end
    if ((rc = dev_alloc(d, a.dummy, (size_t)1 << 16))) return rc;  // any W < 65520
    if ((rc = dev_alloc(d, a.cand_max, F * mask_plane / 4 + 16))) return rc;
    if ((rc = dev_alloc(d, a.slot_plane, F * plane))) return rc;
    if ((rc = dev_alloc(d, a.mask, F * mask_plane))) return rc;
    d->mask_words = F * mask_plane;
    for (int p = 0; p < 2; ++p) {
        if ((rc = dev_alloc(d, d->d_ctr[p], F + 1))) return rc;  // + one extra record: its first word is total_out
        d->ctr_cleared[p] = 0;
    }
    a.ctr = d->d_ctr[0];
    a.total_out = &a.ctr[F].min_key_inv;
    if ((rc = dev_alloc(d, a.seeds, F * cap_roots))) return rc;
    if ((rc = dev_alloc(d, a.clu_key, F * cap_roots))) return rc;
    if ((rc = dev_alloc(d, a.clu_cnt, F * cap_roots))) return rc;
    if ((rc = dev_alloc(d, a.clu_sx, F * cap_roots))) return rc;
    if ((rc = dev_alloc(d, a.clu_sy, F * cap_roots))) return rc;
    if ((rc = dev_alloc(d, a.cand, F * cap_cand))) return rc;
    if ((rc = dev_alloc(d, a.parent, F * cap_cand))) return rc;
    if ((rc = dev_alloc(d, a.sumx, F * cap_cand))) return rc;
    if ((rc = dev_alloc(d, a.sumy, F * cap_cand))) return rc;
    if ((rc = dev_alloc(d, a.cnt, F * cap_cand))) return rc;
    if ((rc = dev_alloc(d, a.minidx, F * cap_cand))) return rc;
    if ((rc = dev_alloc(d, a.roots, F * cap_roots))) return rc;
    if ((rc = dev_alloc(d, a.refined, F * cap_roots))) return rc;
    if ((rc = dev_alloc(d, d->d_out_internal, F * cap_out * 5 + 4))) return rc;  // (+4: k_publish copies 16 bytes at a time)
    d->ws_W = d->ws_H = 0;  // forces the mask to be zeroed below
    HIP_TRY(d, hipHostMalloc((void **)&d->h_ctr, (F + 1) * sizeof(FrameCounters), hipHostMallocDefault));
    d->h_total = (uint32_t *)(d->h_ctr + F);
    d->h_ctr_frames = F;
    HIP_TRY(d, hipHostMalloc((void **)&d->h_out, (F * cap_out * 5 + 4) * sizeof(float), hipHostMallocMapped));
    d->h_out_dev = nullptr;
    if (hipHostGetDevicePointer((void **)&d->h_out_dev, d->h_out, 0) != hipSuccess) d->h_out_dev = nullptr;
    if (d->h_table_rows < F + 1) {
        if (d->h_table) (void)hipHostFree(d->h_table);
        d->h_table = d->h_table_dev = nullptr;
        d->h_table_rows = 0;
        HIP_TRY(d, hipHostMalloc((void **)&d->h_table, (F + 1) * 4 * sizeof(uint32_t), hipHostMallocMapped));
        if (hipHostGetDevicePointer((void **)&d->h_table_dev, d->h_table, 0) != hipSuccess) d->h_table_dev = nullptr;
        d->h_table_rows = F + 1;
    }
    d->h_out_records = F * cap_out;
    d->cap_frames = F;
    d->cap_plane = plane;
    d->alloc_cand = a.cap_cand = cap_cand;
    d->alloc_roots = a.cap_roots = cap_roots;
    d->alloc_out = a.cap_out = cap_out;
    return set_mask_geometry(d, W, H);
}

hipEvent_t get_event(agx_detector *d)
{
    if (!d->free_events.empty()) {
        hipEvent_t e = d->free_events.back();
        d->free_events.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

// Fold finished event pairs into the per-kernel totals (caller has synchronised the stream).
void harvest_events(agx_detector *d)
{
    for (EventPair &p : d->pending_events) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            if (p.kernel >= K_COUNT) {
                d->last_extra_us[p.kernel - K_COUNT] = (int)std::lround(1000.0 * ms);
            } else {
                d->prof_ms[p.kernel] += ms;
                d->prof_launches[p.kernel] += 1;
            }
        }
        d->free_events.push_back(p.a);
        d->free_events.push_back(p.b);
    }
    d->pending_events.clear();
}

// Profiling level 2 around a launch that is not among agx_profile_read's entries (XT_*): an event in front of it and one behind
// it on `st`, harvested like the others.  Nothing is recorded into a stream that is being captured.
EventPair extra_timer_begin(agx_detector *d, hipStream_t st, int which)
{
    EventPair ev{nullptr, nullptr, K_COUNT + which};
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (d->profiling < 2 || hipStreamIsCapturing(st, &cap) != hipSuccess || cap == hipStreamCaptureStatusActive) return ev;
    ev.a = get_event(d);
    ev.b = get_event(d);
    if (!ev.a || !ev.b || hipEventRecord(ev.a, st) != hipSuccess) {
        if (ev.a) d->free_events.push_back(ev.a);
        if (ev.b) d->free_events.push_back(ev.b);
        ev.a = ev.b = nullptr;
    }
    return ev;
}
void extra_timer_end(agx_detector *d, hipStream_t st, const EventPair &ev)
{
    if (!ev.a) return;
    if (hipEventRecord(ev.b, st) == hipSuccess) {
        d->pending_events.push_back(ev);
    } else {
        d->free_events.push_back(ev.a);
        d->free_events.push_back(ev.b);
    }
}

// The handle's device table of RefinePatchConsts (all four half sizes), uploaded on the handle's stream by the first batch that
// needs it.  While the stream is being captured nothing can be allocated or uploaded: a captured batch needs one eager batch
// that used the table first.
int ensure_patch_consts(agx_detector *det, const RefinePatchConsts **table)
{
    *table = nullptr;
    if (!det->patch_consts_uploaded) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(det->stream, &cap);
        if (cap == hipStreamCaptureStatusActive)
            return fail(det, AGX_ERR_STATE, "the refine constants are not on the device yet: run one eager batch at this half_size_patch before capturing");
    }
    const RefinePatchConsts *d_consts =
        static_cast<const RefinePatchConsts *>(side_ensure(det, SB_REFINE_CONSTS, REFINE_PATCH_MAX_HALF * sizeof(RefinePatchConsts), 0));
    if (!d_consts) return fail(det, AGX_ERR_HIP, "hipMalloc: refine constants");
    if (!det->patch_consts_uploaded) {
        det->patch_consts.resize(REFINE_PATCH_MAX_HALF);
        for (int h = 1; h <= REFINE_PATCH_MAX_HALF; ++h) make_refine_patch_consts(h, det->patch_consts[h - 1]);
        HIP_TRY(det, hipMemcpyAsync(const_cast<RefinePatchConsts *>(d_consts), det->patch_consts.data(),
                                    REFINE_PATCH_MAX_HALF * sizeof(RefinePatchConsts), hipMemcpyHostToDevice, det->stream));
        det->patch_consts_uploaded = true;
    }
    *table = d_consts;
    return AGX_OK;
}

// The chain's front at a blur sigma other than 1.5, for the frames of `a` on `st`: k_gauss_blur into the workspace blur plane and,
// with_response, k_response_front -- the frame minima, the candidate mask and cand_max, which K1 otherwise hands to the sparse
// stages.  Neither launch is among the AGX_N_KERNELS that agx_profile_* times.
bool chain_any_sigma(const agx_detector *d)
{
    const float k1_sigma = 1.5f;
    return std::memcmp(&d->blur_sigma, &k1_sigma, sizeof k1_sigma) != 0;
}
int enqueue_any_sigma_front(agx_detector *d, const ChainArgs &a, hipStream_t st, bool with_response)
{
    GaussBlurArgs g{};
    g.src = a.frames;
    g.src_frame_stride = a.frame_stride;
    g.src_row_stride = a.row_stride;
    g.W = a.W;
    g.H = a.H;
    g.dst = a.blur;
    g.dst_row_stride = a.W;
    g.dst_frame_stride = a.plane;
    g.radius = d->front_radius;
    std::memcpy(g.w, d->front_w, sizeof(g.w));
    hipError_t e = (hipError_t)launch_gauss_blur(g, a.fmt, a.n_frames, st);
    if (e != hipSuccess) return fail(d, AGX_ERR_HIP, std::string("launch k_gauss_blur: ") + hipGetErrorString(e));
    if (!with_response) return AGX_OK;
    const EventPair ev = extra_timer_begin(d, st, XT_RESPONSE_FRONT);  // (level 2 only: option "last_response_front_us")
    e = (hipError_t)launch_response_front(a, st);
    extra_timer_end(d, st, ev);
    if (e != hipSuccess) return fail(d, AGX_ERR_HIP, std::string("launch k_response_front: ") + hipGetErrorString(e));
    return AGX_OK;
}

// The chain of one chunk (frames [f0, f0+nf) of the batch) on stream `st`.
int enqueue_chunk(agx_detector *d, int f0, int nf, hipStream_t st)
{
    ChainArgs a = d->args;  // shifted copy
    const size_t F0 = (size_t)f0;
    a.n_frames = nf;
    a.frames += F0 * (size_t)a.frame_stride;
    a.blur += F0 * (size_t)a.plane;
    a.slot_plane += F0 * (size_t)a.plane;
    if (a.resp_dbg) a.resp_dbg += F0 * (size_t)a.plane;
    a.cand_max += F0 * (size_t)(a.mask_plane / 4);
    a.mask += F0 * (size_t)a.mask_plane;
    a.ctr += F0;
    if (a.ctr_next) a.ctr_next += F0;
    a.seeds += F0 * a.cap_roots;
    a.clu_key += F0 * a.cap_roots;
    a.clu_cnt += F0 * a.cap_roots;
    a.clu_sx += F0 * a.cap_roots;
    a.clu_sy += F0 * a.cap_roots;
    a.cand += F0 * a.cap_cand;
    a.parent += F0 * a.cap_cand;
    a.sumx += F0 * a.cap_cand;
    a.sumy += F0 * a.cap_cand;
    a.cnt += F0 * a.cap_cand;
    a.minidx += F0 * a.cap_cand;
    a.roots += F0 * a.cap_roots;
    a.refined += F0 * a.cap_roots;
    if (a.frame_table) a.frame_table += F0 * 4;
    // The sparse phase: one workgroup per frame doing all of it (k_sparse_frame) when the batch fills the chip that way,
    // else the three batch-wide launches.  (Timing ablations and the wave timeline instrument the three launches.)
    int path = d->sparse_path;
    {   // measurement override (read from the environment once per process, chain_kernels.h): 0 .. 3 or ignored
        const int forced = tuning_env("AGX_SPARSE_PATH", -1);
        if (forced >= 0 && forced <= 3) path = forced;
    }
    const int sparse_dbg = 32 | 64 | 128 | 256 | 2048 | 4096 | 8192 | 16384;  // debug_ablation bits that instrument K2 / K3 / K4
    // by batch size: one workgroup per frame pays when the frames fill the chip's 256 CUs in whole rounds (the last round at least
    // three quarters full); then k_verify_seeds keeps its launch (8 waves per SIMD, balanced over the whole batch: 40 us against the
    // 33 .. 75 us per frame of the verify stage inside k_sparse_frame) and flood + refine + emission share one (path 3)
    const int cus = d->n_cus > 0 ? d->n_cus : 256, nearly = cus - cus / 4;  // (MI355X: 256 CUs, 192)
    if (path == 0) path = (nf >= nearly && (nf % cus == 0 || nf % cus >= nearly)) ? 3 : 1;
    // agx_detector_set_half_size_patch: at 2 the flood stages refine as they always did; every other size (and 2 under
    // "chain_refine_general") runs as launches of its own -- the flood stage only clusters, then k_generic_cluster,
    // k_refine_clusters and the emission-only k_rare (chain_kernels.h: launch_refine_clusters)
    const bool deferred = d->half_size_patch != 2 || d->chain_refine_general;
    const int chain_half = d->half_size_patch;
    const RefinePatchConsts *patch_consts = nullptr;
    if (deferred) {
        if (const int rc = ensure_patch_consts(d, &patch_consts)) return rc;
    }
    d->last_chain_refine = deferred ? 1 : 0;
    const bool fused = (path == 2 || path == 3) && !(a.dbg & sparse_dbg) && !deferred;
    d->last_sparse_frame = fused;
    d->last_sparse_path = fused ? path : 1;
    a.sparse_after_verify = fused && path == 3;
    const int plan_fused[] = {K_BLUR_HESSIAN, K_SPARSE}, plan_multi[] = {K_BLUR_HESSIAN, K_THRESHOLD, K_FLOOD_REFINE, K_RARE},
              plan_v_fe[] = {K_BLUR_HESSIAN, K_THRESHOLD, K_SPARSE};
    const int *plan = fused ? (path == 3 ? plan_v_fe : plan_fused) : plan_multi;
    const int n_plan = fused ? (path == 3 ? 3 : 2) : 4;
    const bool any_sigma = chain_any_sigma(d);  // the plan's first entry, K1, is replaced by the any-sigma front
    d->last_chain_front = any_sigma ? 1 : 0;
    if (any_sigma) {
        const int rc = enqueue_any_sigma_front(d, a, st, true);
        if (rc) return rc;
    }
    for (int pi = any_sigma ? 1 : 0; pi < n_plan; ++pi) {
        const int k = plan[pi];
        EventPair ev{nullptr, nullptr, k};
        // (an event pair costs the stream two ~5 us gaps around the kernel: level 1 can sample)
        const bool timed = d->profiling >= 2 || (d->profiling == 1 && k == d->prof_kernel && d->prof_batches % (uint64_t)d->prof_stride == (uint64_t)d->prof_stride - 1);  // the last of each group: never the first batch after an idle stream
        if (deferred && k == K_RARE) {  // between the flood stage and the emission; like the any-sigma front, not among the timed entries
            hipError_t e = (hipError_t)launch_generic_cluster(a, st);
            if (e != hipSuccess) return fail(d, AGX_ERR_HIP, std::string("launch k_generic_cluster: ") + hipGetErrorString(e));
            e = (hipError_t)launch_refine_clusters(a, patch_consts, chain_half, st);
            if (e != hipSuccess) return fail(d, AGX_ERR_HIP, std::string("launch k_refine_clusters: ") + hipGetErrorString(e));
        }
        if (timed) {
            ev.a = get_event(d);
            ev.b = get_event(d);
            HIP_TRY(d, hipEventRecord(ev.a, st));
        }
        hipError_t e = (hipError_t)launch_kernel(k, a, d->rc, st, deferred);
        if (e != hipSuccess)
            return fail(d, AGX_ERR_HIP, std::string("launch ") + kKernelNames[k] + ": " + hipGetErrorString(e));
        if (timed) {
            HIP_TRY(d, hipEventRecord(ev.b, st));
            d->pending_events.push_back(ev);
        }
    }
    if (d->profiling) ++d->prof_batches;
    return AGX_OK;
}

int enqueue_chain(agx_detector *d)
{
    ChainArgs &a = d->args;
    // counters of the batch's frames and the compact-output cursor: the set the previous batch's last
    // kernel cleared, or -- first batch, larger batch, after an error -- one memset
    const int p = d->ctr_cur ^ 1;
    const size_t need = (size_t)a.n_frames + 1;
    // While the stream is being captured into a HIP graph the memset is always recorded: a replayed
    // graph must clear its own set every time (the clearing by the previous batch's last kernel is a fact
    // about the capture, not about the replays -- an odd number of captured batches would otherwise
    // accumulate counters from the second replay on), and nothing "known clear" survives the capture.
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(d->stream, &cap);
    const bool capturing = cap == hipStreamCaptureStatusActive;
    if (capturing) {  // (a kernel node: see launch_clear_counters)
        HIP_TRY(d, (hipError_t)launch_clear_counters(d->d_ctr[p], need, d->stream));
    } else if (d->ctr_cleared[p] < need) {
        HIP_TRY(d, hipMemsetAsync(d->d_ctr[p], 0, need * sizeof(FrameCounters), d->stream));
    }
    d->ctr_cleared[p] = 0;
    a.ctr = d->d_ctr[p];
    a.ctr_next = d->d_ctr[p ^ 1];
    a.total_out = &a.ctr[a.n_frames].min_key_inv;
    d->ctr_cleared[p ^ 1] = 0;
    // (splitting a batch over several streams -- whole chain or sparse kernels only -- was measured
    // and lost every time: see DESIGN.md; batches in flight are separate detectors)
    const int rc = enqueue_chunk(d, 0, a.n_frames, d->stream);
    if (rc) return rc;
    d->ctr_cleared[p ^ 1] = capturing ? 0 : need;  // k_rare of this batch clears it, stream-ordered before the next batch
    d->ctr_cur = p;
    d->batch = BATCH_SADDLES;
    return AGX_OK;
}

// The front of the chain alone -- K1 and whatever ran before it -- for agx_refine_points_enqueue on the frames' blur planes.
// K1 publishes the frames' minima into a counter set that nothing clears afterwards (k_rare / k_sparse_frame do not run):
// neither set is known to be clear then, and the next batch of any kind clears its own.
int enqueue_blur_only(agx_detector *d)
{
    ChainArgs &a = d->args;
    const int p = d->ctr_cur ^ 1;
    const size_t need = (size_t)a.n_frames + 1;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(d->stream, &cap);
    if (cap == hipStreamCaptureStatusActive) {  // (as enqueue_chain: a replayed graph clears its own set every time)
        HIP_TRY(d, (hipError_t)launch_clear_counters(d->d_ctr[p], need, d->stream));
    } else if (d->ctr_cleared[p] < need) {
        HIP_TRY(d, hipMemsetAsync(d->d_ctr[p], 0, need * sizeof(FrameCounters), d->stream));
    }
    d->ctr_cleared[0] = d->ctr_cleared[1] = 0;
    a.ctr = d->d_ctr[p];
    a.ctr_next = d->d_ctr[p ^ 1];
    a.total_out = &a.ctr[a.n_frames].min_key_inv;
    if (chain_any_sigma(d)) {  // the blur alone: nothing behind it looks at a minimum or a mask
        const int rc = enqueue_any_sigma_front(d, a, d->stream, false);
        if (rc) return rc;
        d->ctr_cur = p;
        return AGX_OK;
    }
    hipError_t e = (hipError_t)launch_kernel(K_BLUR_HESSIAN, a, d->rc, d->stream);
    if (e != hipSuccess) return fail(d, AGX_ERR_HIP, std::string("launch ") + kKernelNames[K_BLUR_HESSIAN] + ": " + hipGetErrorString(e));
    d->ctr_cur = p;
    return AGX_OK;
}

int frame_status_of(const FrameCounters &c, uint32_t cap_per_frame)
{
    if (c.flags & (FLAG_CAND_OVERFLOW | FLAG_ROOT_OVERFLOW | FLAG_OUT_OVERFLOW)) return AGX_ERR_CAPACITY;
    if (c.n_out > cap_per_frame) return AGX_ERR_CAPACITY;
    return AGX_OK;
}

// A row of the frame table (count, offset, flags, clusters) as the counter record the fetch works with; false where one of
// the frame's lists overflowed (the full record is then fetched, for the sizes in the error message)
bool counters_of_row(const uint32_t *row, FrameCounters &c)
{
    std::memset(&c, 0, sizeof c);
    c.n_out = row[0];
    c.out_offset = row[1];
    c.flags = row[2];
    c.n_clusters = row[3];
    return !(row[2] & (FLAG_CAND_OVERFLOW | FLAG_ROOT_OVERFLOW | FLAG_OUT_OVERFLOW));
}

// AGX_LA8 .. AGX_RGBA16: the front-end kernel writes the batch's integer luma plane (tight u8 / u16, SB_FRONT) and b becomes that
// plane, which the L8 / L16 paths read: to_luma32f of an integer image is its integer luma / 255 (/ 65535)
int front_luma_plane(agx_detector *det, FrameBatch &b)
{
    const size_t out_px = format_16bit(b.format) ? 2 : 1, need = (size_t)b.n_frames * (size_t)b.width * (size_t)b.height * out_px;
    void *d_front = side_ensure(det, SB_FRONT, need, 0);
    if (!d_front) return fail(det, AGX_ERR_HIP, "hipMalloc: front-end luma plane");
    hipError_t e = (hipError_t)launch_front_luma(b.frames, b.row_stride, b.frame_stride, b.n_frames, b.format, d_front, 0, b.width, b.height,
                                                 det->stream);
    if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_front_luma: ") + hipGetErrorString(e));
    b = {d_front, b.n_frames, b.width, b.height, b.width * out_px, b.width * out_px * b.height, out_px == 2 ? AGX_L16 : AGX_L8};
    return AGX_OK;
}

// One image in host memory: the checks every host entry point makes of it (min_side, lf32: as BatchRules) and, with upload, its
// copy into SB_STAGE, rows a multiple of 4 bytes apart, on the detector's stream: out = the batch of one it is there
int stage_host_frame(agx_detector *det, const void *pixels, int width, int height, size_t row_stride_bytes, int format, int min_side, bool lf32,
                     bool upload, FrameBatch &out)
{
    if (!pixels) return fail(det, AGX_ERR_ARG, "null argument");
    if (const int rc = check_format(det, format, lf32)) return rc;
    if (width < min_side || height < min_side) return fail(det, AGX_ERR_ARG, "width and height must be >= " + std::to_string(min_side));
    const size_t row_bytes = (size_t)width * format_px_bytes(format), pitch = (row_bytes + 3) & ~(size_t)3;
    if (row_stride_bytes < row_bytes) return fail(det, AGX_ERR_ARG, "row stride smaller than a row");
    if (!upload) return AGX_OK;
    HIP_TRY(det, hipSetDevice(det->device));
    const size_t rows = format_rows(format, height);  // (the planar layout: three planes, one under the other)
    void *d_stage = side_ensure(det, SB_STAGE, pitch * rows, 0);
    if (!d_stage) return fail(det, AGX_ERR_HIP, "hipMalloc: staging buffer");
    HIP_TRY(det, hipMemcpy2DAsync(d_stage, pitch, pixels, row_stride_bytes, row_bytes, rows, hipMemcpyHostToDevice, det->stream));
    out = {d_stage, 1, width, height, pitch, pitch * rows, format};
    return AGX_OK;
}

}  // namespace

extern "C" {

int agx_abi_version(void) { return AGX_ABI_VERSION; }

const char *agx_status_string(int status)
{
    switch (status) {
    case AGX_OK: return "ok";
    case AGX_ERR_ARG: return "invalid argument";
    case AGX_ERR_FORMAT: return "unsupported pixel format";
    case AGX_ERR_CAPACITY: return "capacity exceeded";
    case AGX_ERR_HIP: return "HIP runtime error";
    case AGX_ERR_NO_DEVICE: return "no usable gfx950 device";
    case AGX_ERR_FAMILY: return "unknown tag family";
    case AGX_ERR_STATE: return "invalid call sequence";
    case AGX_ERR_NOMEM: return "out of host memory or threads";
    default: return "unknown status";
    }
}

const char *agx_last_error(const agx_detector *det) { return det ? det->last_error.c_str() : g_create_error.c_str(); }

int agx_family_from_str(const char *name, int *family_out)
{
    return agx_guard(nullptr, [&]() -> int {
    if (!name || !family_out) return AGX_ERR_ARG;
    static const struct { const char *lo, *up; int fam; } kNames[] = {
        {"t16h5", "T16H5", AGX_T16H5},     {"t25h7", "T25H7", AGX_T25H7},
        {"t25h9", "T25H9", AGX_T25H9},     {"t36h11", "T36H11", AGX_T36H11},
        {"t36h11b1", "T36H11B1", AGX_T36H11B1}};
    for (const auto &n : kNames)
        if (!std::strcmp(name, n.lo) || !std::strcmp(name, n.up)) {
            *family_out = n.fam;
            return AGX_OK;
        }
    return AGX_ERR_FAMILY;
    });
}

void agx_default_params(agx_params *out)
{
    if (!out) return;
    out->tag_spacing_ratio = 0.3f;
    out->min_saddle_angle = 30.0f;
    out->max_saddle_angle = 60.0f;
    out->max_num_of_boards = 2;
}

int agx_detector_create(int family, const agx_params *params, int device, agx_detector **out)
{
    return agx_guard(nullptr, [&]() -> int {
    if (!out) return AGX_ERR_ARG;
    *out = nullptr;
    g_create_error.clear();
    FamilyInfo fam;
    if (!family_info(family, fam)) return AGX_ERR_FAMILY;
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0 || device < 0 || device >= n_dev) {
        g_create_error = std::string("hipGetDeviceCount: ") + hipGetErrorString(e) + ", devices=" +
                         std::to_string(n_dev) + ", requested " + std::to_string(device);
        return AGX_ERR_NO_DEVICE;
    }
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) {
        g_create_error = std::string("hipGetDeviceProperties: ") + hipGetErrorString(e);
        return AGX_ERR_NO_DEVICE;
    }
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {  // the code object is gfx950 only
        g_create_error = std::string("device arch is '") + prop.gcnArchName + "', need gfx950";
        return AGX_ERR_NO_DEVICE;
    }
    e = hipSetDevice(device);
    if (e != hipSuccess) {
        g_create_error = std::string("hipSetDevice: ") + hipGetErrorString(e);
        return AGX_ERR_NO_DEVICE;
    }
    struct Unwind {  // (an exception or an early return behind the stream's creation)
        void operator()(agx_detector *p) const
        {
            if (p->own_stream) (void)hipStreamDestroy(p->own_stream);
            delete p;
        }
    };
    tuning_env_reload();  // the AGX_* measurement overrides are read when a detector is created (and kept: no getenv per launch)
    std::unique_ptr<agx_detector, Unwind> d(new agx_detector());
    d->family = family;
    d->fam = fam;
    if (params) d->params = *params;
    else agx_default_params(&d->params);
    d->device = device;
    d->n_cus = prop.multiProcessorCount;
    if (const char *rz = std::getenv("AGX_REDZONE_BYTES")) {  // tests: guard bytes around every workspace buffer
        const long v = std::atol(rz);
        if (v > 0 && v <= (1 << 24)) d->redzone = ((size_t)v + 255) & ~(size_t)255;  // keeps the buffers' alignment
    }
    e = hipStreamCreateWithFlags(&d->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        g_create_error = std::string("hipStreamCreateWithFlags: ") + hipGetErrorString(e);
        return AGX_ERR_HIP;
    }
    d->stream = d->own_stream;
    e = (hipError_t)init_device_kernels();  // function attributes are per device
    if (e != hipSuccess) {
        g_create_error = std::string("hipFuncSetAttribute: ") + hipGetErrorString(e);
        return AGX_ERR_HIP;
    }
    make_blur_weights(1.5f, d->blur_w);
    d->front_radius = make_blur_weights(d->blur_sigma, d->front_w);
    make_refine_consts(d->rc);
    *out = d.release();
    return AGX_OK;
    });
}

void agx_detector_destroy(agx_detector *det)
{
    if (!det) return;
    try {
    (void)hipSetDevice(det->device);
    (void)hipStreamSynchronize(det->stream);
    harvest_events(det);
    for (hipEvent_t e : det->free_events) (void)hipEventDestroy(e);
    free_workspace(det);
    if (det->pool) destroy_worker_pool(det->pool);
    if (det->tail_workers) destroy_tail_workers(det->tail_workers);
    for (int i = 0; i < SB_COUNT; ++i) side_free(det, i);
    if (det->h_table) (void)hipHostFree(det->h_table);
    for (int i = 0; i < AGX_UPLOAD_STREAMS; ++i)
        if (det->upload_streams[i]) (void)hipStreamDestroy(det->upload_streams[i]);
    if (det->own_stream) (void)hipStreamDestroy(det->own_stream);
    } catch (...) {  // (joining worker threads can throw std::system_error)
    }
    delete det;
}

int agx_detector_family_info(const agx_detector *det, int *edge_bits, int *border_bits, int *hamming_distance,
                             const uint64_t **codes, int *n_codes)
{
    return agx_guard(det, [&]() -> int {
    if (!det) return AGX_ERR_ARG;
    if (edge_bits) *edge_bits = det->fam.edge;
    if (border_bits) *border_bits = det->fam.border;
    if (hamming_distance) *hamming_distance = det->fam.hamming;
    if (codes) *codes = det->fam.codes;
    if (n_codes) *n_codes = det->fam.n_codes;
    return AGX_OK;
    });
}

int agx_detector_set_limits(agx_detector *det, uint32_t max_candidates, uint32_t max_clusters, uint32_t max_saddles)
{
    return agx_guard(det, [&]() -> int {
    if (!det) return AGX_ERR_ARG;
    if (max_candidates >= (1u << 30) || max_saddles > (1u << 24)) return AGX_ERR_ARG;
    det->lim_cand = max_candidates;
    det->lim_roots = max_clusters;
    det->lim_out = max_saddles;
    return AGX_OK;
    });
}

int agx_detector_set_blur_sigma(agx_detector *det, float sigma)
{
    return agx_guard(det, [&]() -> int {
    if (!det) return AGX_ERR_ARG;
    if (!blur_sigma_ok(sigma)) return fail(det, AGX_ERR_ARG, "sigma must be positive and finite with ceil(2 sigma) <= 16");
    det->blur_sigma = sigma;
    det->front_radius = make_blur_weights(sigma, det->front_w);
    return AGX_OK;
    });
}

int agx_detector_get_blur_sigma(const agx_detector *det, float *sigma)
{
    return agx_guard(det, [&]() -> int {
    if (!det || !sigma) return AGX_ERR_ARG;
    *sigma = det->blur_sigma;
    return AGX_OK;
    });
}

int agx_detector_set_half_size_patch(agx_detector *det, int half_size_patch)
{
    return agx_guard(det, [&]() -> int {
    if (!det) return AGX_ERR_ARG;
    if (half_size_patch < 1 || half_size_patch > REFINE_PATCH_MAX_HALF) return fail(det, AGX_ERR_ARG, "half_size_patch must be in 1 .. 4");
    det->half_size_patch = half_size_patch;  // (read by the next enqueue: a batch in flight keeps what it was enqueued with)
    return AGX_OK;
    });
}

int agx_detector_get_half_size_patch(const agx_detector *det, int *half_size_patch)
{
    return agx_guard(det, [&]() -> int {
    if (!det || !half_size_patch) return AGX_ERR_ARG;
    *half_size_patch = det->half_size_patch;
    return AGX_OK;
    });
}

int agx_detector_set_stream(agx_detector *det, void *hip_stream, int external)
{
    return agx_guard(det, [&]() -> int {
    if (!det) return AGX_ERR_ARG;
    HIP_TRY(det, hipSetDevice(det->device));
    HIP_TRY(det, hipStreamSynchronize(det->stream));
    harvest_events(det);
    det->stream = external ? (hipStream_t)hip_stream : det->own_stream;
    return AGX_OK;
    });
}

int agx_detector_set_option(agx_detector *det, const char *name, int value)
{
    return agx_guard(det, [&]() -> int {
    if (!det || !name) return AGX_ERR_ARG;
    if (!std::strcmp(name, "force_generic")) det->force_generic = value != 0;
    else if (!std::strcmp(name, "k1_rows_per_segment")) det->k1_rows = value > 0 ? value : 0;
    else if (!std::strcmp(name, "sparse_path")) det->sparse_path = value >= 0 && value <= 3 ? value : 0;
    else if (!std::strcmp(name, "debug_ablation")) det->dbg = value;  // timing only, results invalid
    else if (!std::strcmp(name, "store_response")) det->store_resp = value != 0;
    else if (!std::strcmp(name, "refine_general_kernel")) det->refine_general_kernel = value != 0;  // tests, measurement: same results
    else if (!std::strcmp(name, "chain_refine_general")) det->chain_refine_general = value != 0;    // tests, measurement: same results
    else if (!std::strcmp(name, "profile_stride")) det->prof_stride = value > 1 ? value : 1;
    else if (!std::strcmp(name, "profile_kernel")) det->prof_kernel = value >= 0 && value < K_COUNT ? value : K_BLUR_HESSIAN;
    else if (!std::strcmp(name, "device_tail")) {  // 1 on (refused where libm differs), 0 off, -1 back to the default (on where possible)
        if (value > 0) {
            const uint64_t mismatches = libm_check_once();
            if (mismatches) {
                det->device_tail = 0;
                return fail(det, AGX_ERR_STATE, "device_tail: this C library's atan2f is not the routine the device tail restates (" +
                                                    std::to_string(mismatches) + " of 2^20 inputs differ); the host tail stays in use");
            }
        }
        det->device_tail = value > 0 ? 1 : (value < 0 ? -1 : 0);
    }
    else if (!std::strcmp(name, "tail_debug_band")) det->tail_debug_band_mdeg = value > 0 ? std::min(value, 30000) : 0;  // tests: thousandths of a degree
    else if (!std::strcmp(name, "reload_tuning_env")) tuning_env_reload();  // (process-wide: the AGX_* overrides are read again)
    else if (!std::strcmp(name, "tail_threads")) {
        const int n = value < 1 ? 1 : (value > 64 ? 64 : value);
        if (n != det->tail_threads) {
            if (det->tail_workers) destroy_tail_workers(det->tail_workers);
            det->tail_workers = nullptr;  // (creating the new ones can fail: AGX_ERR_NOMEM, the option back at one thread)
            det->tail_threads = 1;
            det->tail_workers = create_tail_workers(n);
            det->tail_threads = n;
        }
    } else return fail(det, AGX_ERR_ARG, std::string("unknown option ") + name);
    return AGX_OK;
    });
}

int agx_detector_get_option(const agx_detector *det, const char *name, int *value)
{
    return agx_guard(det, [&]() -> int {
    if (!det || !name || !value) return AGX_ERR_ARG;
    const ChainArgs &a = det->args;
    if (!std::strcmp(name, "force_generic")) *value = det->force_generic;
    else if (!std::strcmp(name, "store_response")) *value = det->store_resp;
    else if (!std::strcmp(name, "debug_ablation")) *value = det->dbg;
    else if (!std::strcmp(name, "tail_threads")) *value = det->tail_threads;
    else if (!std::strcmp(name, "device_tail")) *value = det->device_tail;  // (-1: by the batch's size, where available)
    else if (!std::strcmp(name, "tail_debug_band")) *value = det->tail_debug_band_mdeg;
    else if (!std::strcmp(name, "last_find_boards_frames")) *value = det->last_list_frames[LIST_FIND];  // (of the last agx_find_boards_fetch)
    else if (!std::strcmp(name, "last_find_boards_handed_back")) *value = det->last_list_handed_back[LIST_FIND];
    else if (!std::strcmp(name, "last_grow_boards_frames")) *value = det->last_list_frames[LIST_GROW];  // (of the last agx_grow_boards_fetch)
    else if (!std::strcmp(name, "last_grow_boards_handed_back")) *value = det->last_list_handed_back[LIST_GROW];
    else if (!std::strcmp(name, "last_init_quads_frames")) *value = det->last_list_frames[LIST_INIT];  // (of the last agx_init_quads_fetch)
    else if (!std::strcmp(name, "last_init_quads_handed_back")) *value = det->last_list_handed_back[LIST_INIT];
    else if (!std::strcmp(name, "last_device_tail_frames")) *value = det->last_tail_frames;
    else if (!std::strcmp(name, "last_device_tail_fallbacks")) *value = det->last_tail_fallbacks;
    else if (!std::strcmp(name, "last_device_tail_uncertain")) *value = det->last_tail_uncertain;  // (of them: an angle inside its guard band)
    // the blur kernel's tiling of the last enqueued batch (0 before the first one)
    else if (!std::strcmp(name, "k1_rows_per_segment")) *value = a.rows_per_seg;
    else if (!std::strcmp(name, "sparse_path")) *value = det->sparse_path;
    else if (!std::strcmp(name, "last_sparse_path")) *value = det->last_sparse_path;
    else if (!std::strcmp(name, "last_chain_front")) *value = det->last_chain_front;
    else if (!std::strcmp(name, "refine_general_kernel")) *value = det->refine_general_kernel;
    else if (!std::strcmp(name, "chain_refine_general")) *value = det->chain_refine_general;
    else if (!std::strcmp(name, "last_chain_refine")) *value = det->last_chain_refine;  // (of the last chain batch: 0 inside the flood stages, 1 k_refine_clusters)
    else if (!std::strcmp(name, "last_response_front_us")) *value = det->last_extra_us[XT_RESPONSE_FRONT];  // (profiling level 2: of the last batch a fetch, sync or agx_profile_read harvested)
    else if (!std::strcmp(name, "last_clusters_front_us")) *value = det->last_extra_us[XT_PLANE_FRONT];
    else if (!std::strcmp(name, "last_clusters_emit_us")) *value = det->last_extra_us[XT_EMIT_CLUSTERS];
    else if (!std::strcmp(name, "last_refine_kernel")) *value = det->last_refine_kernel;  // (of the last refine batch: 0 k_refine_points, 1 k_refine_patch)
    else if (!std::strcmp(name, "k1_segments")) *value = a.n_segs;
    else if (!std::strcmp(name, "k1_strips")) *value = a.n_strips;
    else if (!std::strcmp(name, "k1_strip_columns")) *value = a.strip_cols;
    else return AGX_ERR_ARG;
    return AGX_OK;
    });
}

int agx_detector_sync(agx_detector *det)
{
    return agx_guard(det, [&]() -> int {
    if (!det) return AGX_ERR_ARG;
    HIP_TRY(det, hipSetDevice(det->device));
    HIP_TRY(det, hipStreamSynchronize(det->stream));
    return AGX_OK;
    });
}

static int batch_enqueue_impl(agx_detector *det, const void *d_frames, int n_frames, int width, int height,
                              size_t row_stride_bytes, size_t frame_stride_bytes, int format, void *d_saddles,
                              uint32_t saddle_capacity, void *d_frame_table, bool blur_only = false)
{
    if (!det) return AGX_ERR_ARG;
    FrameBatch b{d_frames, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format};
    int rc = check_frame_batch(det, b, {/*min_side*/ 2, /*lf32*/ true, /*lone_frame_stride*/ true, /*align16*/ true, /*front_rows*/ true});
    if (rc) return rc;
    begin_batch(det);
    HIP_TRY(det, hipSetDevice(det->device));
    rc = ensure_workspace(det, n_frames, width, height);
    if (rc) return rc;
    if (format_front(format)) {  // the chain reads the front-end kernel's plane, and to_luma8 of this batch may be derived from it
        if ((rc = front_luma_plane(det, b))) return rc;
        det->front_src = d_frames;
        det->front_format = format;
        det->front_frames = n_frames;
    }
    d_frames = b.frames;
    row_stride_bytes = b.row_stride;
    frame_stride_bytes = b.frame_stride;
    format = b.format;
    // rows that are not 4-byte aligned (tightly packed L8 / RGB8 of a width that is not a multiple
    // of 4, odd-width L16): the blur kernel gathers bytes instead of loading dwords
    const bool byte_rows = ((row_stride_bytes | (uintptr_t)d_frames | (n_frames > 1 ? frame_stride_bytes : 0)) & 3) != 0;
    ChainArgs &a = det->args;
    a.frames = (const uint8_t *)d_frames;
    a.frame_stride = (long long)frame_stride_bytes;
    a.row_stride = (int)row_stride_bytes;
    a.byte_rows = byte_rows ? 1 : 0;
    a.fmt = format;
    a.W = width;
    a.H = height;
    a.n_frames = n_frames;
    a.plane = (long long)width * height;
    std::memcpy(a.w, det->blur_w, sizeof(a.w));
    a.min_angle = det->params.min_saddle_angle;
    a.max_angle = det->params.max_saddle_angle;
    if (d_saddles) {
        a.out = (float *)d_saddles;
        a.out_total_cap = saddle_capacity;
        a.frame_table = (uint32_t *)d_frame_table;
        det->external_out = true;
    } else {
        // One frame (the reference's own use): the list goes straight to the pinned host mirror over PCIe -- a few KB of
        // posted writes -- and the fetch needs no second copy behind the counters' (one wait less per call).
        det->out_in_host = n_frames == 1 && det->h_out_dev != nullptr && det->h_table_dev != nullptr;
        a.out = det->out_in_host ? det->h_out_dev : det->d_out_internal;
        a.out_total_cap = (uint32_t)std::min<size_t>((size_t)n_frames * a.cap_out, 0xffffffffu);
        a.frame_table = det->out_in_host ? det->h_table_dev : nullptr;  // ... and so do its count, offset, status
        det->external_out = false;
    }
    a.force_generic = det->force_generic;
    a.dbg = det->dbg;
    // debug_ablation & 4096: wave start / end times of the sparse kernels into the slot plane (generic path's, sparsely used)
    a.wave_times = ((det->dbg & 4096) && (size_t)n_frames * (size_t)a.plane * 4 >= 3 * WAVE_TIMES_STRIDE * 16)
                       ? reinterpret_cast<unsigned long long *>(a.slot_plane) : nullptr;
    a.resp_dbg = nullptr;
    det->resp_stored = false;
    if (det->store_resp) {  // parity tests: K1 also stores the response it evaluates in registers
        const size_t need = (size_t)n_frames * (size_t)a.plane * sizeof(float);
        a.resp_dbg = static_cast<float *>(side_ensure(det, SB_RESP_STORE, need, 0));
        if (!a.resp_dbg) return fail(det, AGX_ERR_HIP, "hipMalloc: response planes");
        HIP_TRY(det, hipMemsetAsync(a.resp_dbg, 0, need, det->stream));  // the border ring is 0
        det->resp_stored = true;
    }
    if (!plan_k1(a, det->k1_rows)) return fail(det, AGX_ERR_ARG, "unsupported frame geometry");
    if (blur_only) return enqueue_blur_only(det);  // agx_refine_points_enqueue: nothing of the chain will be there to be fetched
    return enqueue_chain(det);
}

int agx_saddles_batch_enqueue(agx_detector *det, const void *d_frames, int n_frames, int width, int height,
                              size_t row_stride_bytes, size_t frame_stride_bytes, int format)
{
    return agx_guard(det, [&]() -> int {
    return batch_enqueue_impl(det, d_frames, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format,
                              nullptr, 0, nullptr);
    });
}

int agx_saddles_batch_enqueue_to(agx_detector *det, const void *d_frames, int n_frames, int width, int height,
                                 size_t row_stride_bytes, size_t frame_stride_bytes, int format, void *d_saddles,
                                 uint32_t saddle_capacity, void *d_frame_table)
{
    return agx_guard(det, [&]() -> int {
    if (!d_saddles || !d_frame_table || ((uintptr_t)d_saddles & 3) || ((uintptr_t)d_frame_table & 3))
        return fail(det, AGX_ERR_ARG, "null or misaligned output buffers");
    return batch_enqueue_impl(det, d_frames, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format,
                              d_saddles, saddle_capacity, d_frame_table);
    });
}

// agx_saddles_batch_fetch without the pairing rule (agx::fetch_compact reads the chain's results of a detect batch too)
static int saddles_fetch_impl(agx_detector *det, agx_saddle *out, uint32_t cap_per_frame, uint32_t *counts, int *frame_status)
{
    return agx_guard(det, [&]() -> int {
    if (!det || !counts || (!out && cap_per_frame)) return fail(det, AGX_ERR_ARG, "null output");
    if (!chain_in_flight(det)) return fail(det, AGX_ERR_STATE, "no batch enqueued");
    if (det->external_out) return fail(det, AGX_ERR_STATE, "last batch wrote to caller-owned device buffers");
    HIP_TRY(det, hipSetDevice(det->device));
    const ChainArgs &a = det->args;
    const size_t F = (size_t)a.n_frames;
    bool have_counters = false;
    if (det->out_in_host) {  // one frame: list and table row are in host memory when the stream is through -- no copy at all
        HIP_TRY(det, hipStreamSynchronize(det->stream));
        have_counters = counters_of_row(det->h_table, det->h_ctr[0]);  // (false: the full record below)
        *det->h_total = det->h_table[0] + det->h_table[1];
    }
    bool out_fetched = det->out_in_host;
    if (!have_counters && !det->out_in_host && det->h_table_dev && det->h_out_dev && F + 1 <= det->h_table_rows) {
        // a batch: frame rows and the compact array come over by a kernel (k_publish), one wait
        hipError_t e = (hipError_t)launch_publish(a, (uint32_t)std::min<size_t>(det->h_out_records, 0xffffffffu), det->h_table_dev, det->h_out_dev, det->stream);
        if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_publish: ") + hipGetErrorString(e));
        HIP_TRY(det, hipStreamSynchronize(det->stream));
        bool bad = false;
        for (size_t f = 0; f < F; ++f)
            if (!counters_of_row(det->h_table + 4 * f, det->h_ctr[f])) bad = true;
        *det->h_total = det->h_table[4 * F];
        have_counters = !bad;  // (an overflowing frame: the full records below, for the sizes in the error message)
        out_fetched = true;
    }
    if (!have_counters) {
        HIP_TRY(det, hipMemcpyAsync(det->h_ctr, a.ctr, F * sizeof(FrameCounters), hipMemcpyDeviceToHost, det->stream));
        HIP_TRY(det, hipMemcpyAsync(det->h_total, a.total_out, sizeof(uint32_t), hipMemcpyDeviceToHost, det->stream));
        HIP_TRY(det, hipStreamSynchronize(det->stream));
    }
    harvest_events(det);
    const uint32_t total = *det->h_total;
    if (total > det->h_out_records) return fail(det, AGX_ERR_HIP, "compact output counter out of range");
    if (total && !out_fetched) {
        HIP_TRY(det, hipMemcpyAsync(det->h_out, a.out, (size_t)total * 5 * sizeof(float), hipMemcpyDeviceToHost,
                                    det->stream));
        HIP_TRY(det, hipStreamSynchronize(det->stream));
    }
    int first_bad = AGX_OK;
    for (size_t f = 0; f < F; ++f) {
        const FrameCounters &c = det->h_ctr[f];
        const int st = frame_status_of(c, cap_per_frame);
        counts[f] = c.n_out;
        if (frame_status) frame_status[f] = st;
        if (st != AGX_OK) {
            if (first_bad == AGX_OK) {
                first_bad = st;
                char buf[160];
                std::snprintf(buf, sizeof buf,
                              "frame %zu: capacity exceeded (flags=0x%x seeds=%u clusters=%u candidates=%u saddles=%u)", f,
                              c.flags, c.n_seeds, c.n_clusters + c.n_clusters2, c.n_cand, c.n_out);
                det->last_error = buf;
            }
            continue;
        }
        if (c.n_out)
            std::memcpy(out + f * (size_t)cap_per_frame, det->h_out + (size_t)c.out_offset * 5,
                        (size_t)c.n_out * sizeof(agx_saddle));
    }
    return first_bad;
    });
}

int agx_saddles_batch_fetch(agx_detector *det, agx_saddle *out, uint32_t cap_per_frame, uint32_t *counts,
                            int *frame_status)
{
    return agx_guard(det, [&]() -> int {
    if (det && det->batch != BATCH_NONE)  // (none: the null-output check comes first, below)
        if (const int rc = refuse_other_batch(det, BATCH_SADDLES)) return rc;
    return saddles_fetch_impl(det, out, cap_per_frame, counts, frame_status);
    });
}

// detect over a batch in device memory, stream-ordered (csrc/detect_batch.cpp: the chain, k_luma8, the device tail, the fetch)
static int detect_enqueue_checked(agx_detector *det, const void *d_frames, int n_frames, int width, int height, size_t row_stride_bytes,
                                  size_t frame_stride_bytes, int format, uint32_t cap_per_frame, int results, agx_tag *d_tags,
                                  uint32_t *d_counts, int *d_status, uint32_t slab_records = 0)
{
    const bool to_device = results == RESULTS_CALLER;
    if (!det) return AGX_ERR_ARG;
    // the format alone, ahead of everything else (the decode needs to_luma8: agx_detect_planes for an f32 plane); the chain's
    // enqueue checks the whole batch
    if (!format_px_bytes(format) || format == AGX_LF32)
        return fail(det, AGX_ERR_FORMAT, "format must be an integer agx_format (AGX_LF32: agx_detect_planes)");
    if (to_device && (!d_counts || !d_status || (!d_tags && cap_per_frame) || (((uintptr_t)d_tags | (uintptr_t)d_counts | (uintptr_t)d_status) & 3)))
        return fail(det, AGX_ERR_ARG, "null or misaligned output buffers");
    return detect_enqueue_impl(det, d_frames, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format, cap_per_frame, results,
                               d_tags, d_counts, d_status, slab_records);
}

int agx_detect_batch_enqueue(agx_detector *det, const void *d_frames, int n_frames, int width, int height, size_t row_stride_bytes,
                             size_t frame_stride_bytes, int format, uint32_t cap_per_frame)
{
    return agx_guard(det, [&]() -> int {
    return detect_enqueue_checked(det, d_frames, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format, cap_per_frame,
                                  RESULTS_HOST, nullptr, nullptr, nullptr);
    });
}

int agx_detect_batch_enqueue_to(agx_detector *det, const void *d_frames, int n_frames, int width, int height, size_t row_stride_bytes,
                                size_t frame_stride_bytes, int format, agx_tag *d_tags, uint32_t cap_per_frame, uint32_t *d_counts,
                                int *d_status)
{
    return agx_guard(det, [&]() -> int {
    return detect_enqueue_checked(det, d_frames, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format, cap_per_frame,
                                  RESULTS_CALLER, d_tags, d_counts, d_status);
    });
}

int agx_detect_batch_fetch(agx_detector *det, agx_tag *out, uint32_t *counts, int *frame_status, int n_threads)
{
    return agx_guard(det, [&]() -> int {
    if (!det) return AGX_ERR_ARG;
    if (const int other = refuse_other_batch(det, BATCH_DETECT)) return other;
    if (det->detect.results == RESULTS_GROUP) return fail(det, AGX_ERR_STATE, "the batch in flight is a group's: fetch it with agx_group_detect_fetch");
    det->last_error.clear();
    const int rc = detect_fetch_impl(det, out, counts, frame_status, n_threads);
    if (rc == AGX_ERR_NOMEM) det->last_error = "out of host memory or threads";
    else if (rc != AGX_OK && rc != AGX_ERR_CAPACITY && det->last_error.empty()) det->last_error = agx_status_string(rc);
    return rc;
    });
}

}  // extern "C"

// ---- rochade_refine of caller-given points (src/detector.rs:194-361) ---------------------------------------------------------
static int refine_points_enqueue_impl(agx_detector *det, const void *d_frames, int n_frames, int width, int height,
                                      size_t row_stride_bytes, size_t frame_stride_bytes, int format, int image,
                                      const void *d_points, uint32_t points_per_frame, const uint32_t *d_counts,
                                      agx_saddle *d_out, uint32_t *d_status, int half)
{
    if (!det) return AGX_ERR_ARG;
    if (half < 1 || half > REFINE_PATCH_MAX_HALF) return fail(det, AGX_ERR_ARG, "half_size_patch must be in 1 .. 4");
    if (!d_frames || !d_points || n_frames <= 0) return fail(det, AGX_ERR_ARG, "null frames, null points or n_frames <= 0");
    if (!points_per_frame) return fail(det, AGX_ERR_ARG, "points_per_frame must be > 0");
    if ((d_out == nullptr) != (d_status == nullptr)) return fail(det, AGX_ERR_ARG, "d_out and d_status: both or neither");
    if (image != AGX_REFINE_BLURRED && image != AGX_REFINE_PLANE) return fail(det, AGX_ERR_ARG, "image must be AGX_REFINE_BLURRED or AGX_REFINE_PLANE");
    if ((((uintptr_t)d_points | (uintptr_t)d_counts | (uintptr_t)d_out | (uintptr_t)d_status) & 3))
        return fail(det, AGX_ERR_ARG, "points, counts and result buffers must be 4-byte aligned");
    if (image == AGX_REFINE_PLANE && format != AGX_LF32) return fail(det, AGX_ERR_FORMAT, "AGX_REFINE_PLANE takes an AGX_LF32 plane");
    // (the 16-bit alignment and the front-end row limit are the chain's to check, where it runs: batch_enqueue_impl below)
    if (const int rc = check_frame_batch(det, {d_frames, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format},
                                         {/*min_side*/ 1, /*lf32*/ true, /*lone_frame_stride*/ false, /*align16*/ false, /*front_rows*/ false}))
        return rc;
    const size_t slots = (size_t)n_frames * points_per_frame;
    if (slots >= ((size_t)1 << 31)) return fail(det, AGX_ERR_ARG, "at most 2^31 - 1 points per batch");
    HIP_TRY(det, hipSetDevice(det->device));
    begin_batch(det);
    // half_size_patch = 2 is k_refine_points, one point per lane; every other size, and 2 under "refine_general_kernel", is
    // k_refine_patch with its constants from the handle's device table (all four sizes, uploaded once)
    const bool general = half != 2 || det->refine_general_kernel;
    const RefinePatchConsts *d_consts = nullptr;
    if (general) {
        if (const int rc = ensure_patch_consts(det, &d_consts)) return rc;
        d_consts += half - 1;
    }
    RefinePointsArgs p{};
    p.W = width;
    p.H = height;
    const int win = 4 * half + 1;
    const bool any_window = width >= win && height >= win;  // (a smaller frame is valid input: all its points are AGX_POINT_OUTSIDE)
    if (image == AGX_REFINE_PLANE || !any_window) {
        p.img = (const float *)d_frames;  // (!any_window: never read)
        p.pitch = (long long)(row_stride_bytes / 4);
        p.frame_stride = (long long)(frame_stride_bytes / 4);
        p.padded = 0;
    } else {
        // the front end and K1 as they are: the blur planes of the workspace, tight [n_frames][H][W]
        const int rc = batch_enqueue_impl(det, d_frames, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format, nullptr, 0,
                                          nullptr, true);
        if (rc) return rc;
        p.img = det->args.blur;
        p.pitch = width;
        p.frame_stride = det->args.plane;
        p.padded = 1;  // (ensure_workspace: 16 floats behind the last plane)
    }
    if (!d_out) {
        if (!side_ensure_pair(det, SB_REFINE_OUT, slots * sizeof(agx_saddle), 0, SB_REFINE_STATUS, slots * sizeof(uint32_t), 0))
            return fail(det, AGX_ERR_HIP, "hipMalloc: refined points");
        d_out = det->side[SB_REFINE_OUT].ptr<agx_saddle>();
        d_status = det->side[SB_REFINE_STATUS].ptr<uint32_t>();
        det->refine.results = RESULTS_HOST;
    } else {
        det->refine.results = RESULTS_CALLER;
    }
    p.points = static_cast<const float *>(d_points);
    p.points_per_frame = points_per_frame;
    p.counts = d_counts;
    p.out = reinterpret_cast<float *>(d_out);
    p.status = d_status;
    hipError_t e = (hipError_t)(general ? launch_refine_patch(p, d_consts, half, n_frames, det->stream)
                                        : launch_refine_points(p, det->rc, n_frames, det->stream));
    if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string(general ? "k_refine_patch: " : "k_refine_points: ") + hipGetErrorString(e));
    det->last_refine_kernel = general ? 1 : 0;
    det->batch = BATCH_REFINE;
    det->refine.n_frames = n_frames;
    det->refine.points_per_frame = points_per_frame;
    det->refine.d_counts = d_counts;
    return AGX_OK;
}

static int refine_points_fetch_impl(agx_detector *det, agx_saddle *out, uint32_t *status)
{
    if (!det) return AGX_ERR_ARG;
    if (const int other = refuse_other_batch(det, BATCH_REFINE)) return other;
    const RefinePending b = det->refine;
    const bool to_host = b.results == RESULTS_HOST;
    if (to_host && (!out || !status)) return fail(det, AGX_ERR_ARG, "null output");  // (the batch stays in flight)
    HIP_TRY(det, hipSetDevice(det->device));
    det->batch = BATCH_NONE;  // resolved by this call, whatever it returns
    const size_t slots = (size_t)b.n_frames * b.points_per_frame;
    if (to_host) {
        const agx_saddle *d_out = det->side[SB_REFINE_OUT].ptr<agx_saddle>();
        const uint32_t *d_status = det->side[SB_REFINE_STATUS].ptr<uint32_t>();
        if (!b.d_counts) {
            HIP_TRY(det, hipMemcpyAsync(out, d_out, slots * sizeof(agx_saddle), hipMemcpyDeviceToHost, det->stream));
            HIP_TRY(det, hipMemcpyAsync(status, d_status, slots * sizeof(uint32_t), hipMemcpyDeviceToHost, det->stream));
        } else {  // only the slots the kernel wrote reach the caller's arrays: by way of a host copy of everything + the counts
            std::vector<uint32_t> &h = det->refine_host;
            h.resize(slots * 6 + (size_t)b.n_frames);
            HIP_TRY(det, hipMemcpyAsync(h.data(), d_out, slots * sizeof(agx_saddle), hipMemcpyDeviceToHost, det->stream));
            HIP_TRY(det, hipMemcpyAsync(h.data() + slots * 5, d_status, slots * sizeof(uint32_t), hipMemcpyDeviceToHost, det->stream));
            HIP_TRY(det, hipMemcpyAsync(h.data() + slots * 6, b.d_counts, (size_t)b.n_frames * sizeof(uint32_t), hipMemcpyDeviceToHost, det->stream));
        }
    }
    HIP_TRY(det, hipStreamSynchronize(det->stream));
    harvest_events(det);
    if (to_host && b.d_counts) {
        const std::vector<uint32_t> &h = det->refine_host;
        for (int f = 0; f < b.n_frames; ++f) {
            const size_t n = std::min(h[slots * 6 + (size_t)f], b.points_per_frame), s0 = (size_t)f * b.points_per_frame;
            if (!n) continue;
            std::memcpy(out + s0, h.data() + s0 * 5, n * sizeof(agx_saddle));
            std::memcpy(status + s0, h.data() + slots * 5 + s0, n * sizeof(uint32_t));
        }
    }
    return AGX_OK;
}

extern "C" {

int agx_refine_points_enqueue_h(agx_detector *det, const void *d_frames, int n_frames, int width, int height, size_t row_stride_bytes,
                                size_t frame_stride_bytes, int format, int image, const void *d_points, uint32_t points_per_frame,
                                const uint32_t *d_counts, agx_saddle *d_out, uint32_t *d_status, int half_size_patch)
{
    return agx_guard(det, [&]() -> int {
    return refine_points_enqueue_impl(det, d_frames, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format, image,
                                      d_points, points_per_frame, d_counts, d_out, d_status, half_size_patch);
    });
}

int agx_refine_points_enqueue(agx_detector *det, const void *d_frames, int n_frames, int width, int height, size_t row_stride_bytes,
                              size_t frame_stride_bytes, int format, int image, const void *d_points, uint32_t points_per_frame,
                              const uint32_t *d_counts, agx_saddle *d_out, uint32_t *d_status)
{
    return agx_refine_points_enqueue_h(det, d_frames, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format, image, d_points,
                                       points_per_frame, d_counts, d_out, d_status, 2);
}

int agx_refine_points_fetch(agx_detector *det, agx_saddle *out, uint32_t *status)
{
    return agx_guard(det, [&]() -> int { return refine_points_fetch_impl(det, out, status); });
}

// rochade_refine on the frames' blur with no blur plane: k_refine_windows computes every point's blur window from the input
int agx_refine_windows_enqueue(agx_detector *det, const void *d_frames, int n_frames, int width, int height, size_t row_stride_bytes,
                               size_t frame_stride_bytes, int format, const void *d_points, size_t point_stride_bytes,
                               uint32_t points_per_frame, const uint32_t *d_counts, const uint32_t *d_status_in, agx_saddle *d_out,
                               uint32_t *d_status, int factor, int half_size_patch)
{
    return agx_guard(det, [&]() -> int {
    if (!det) return AGX_ERR_ARG;
    if (format != AGX_L8 && format != AGX_L16 && format != AGX_LF32) return fail(det, AGX_ERR_FORMAT, "format must be AGX_L8, AGX_L16 or AGX_LF32");
    if (half_size_patch < 1 || half_size_patch > REFINE_PATCH_MAX_HALF) return fail(det, AGX_ERR_ARG, "half_size_patch must be in 1 .. 4");
    if (factor < 1 || factor > 4) return fail(det, AGX_ERR_ARG, "factor must be in 1 .. 4");
    if (!d_frames || !d_points || n_frames <= 0) return fail(det, AGX_ERR_ARG, "null frames, null points or n_frames <= 0");
    if (!points_per_frame) return fail(det, AGX_ERR_ARG, "points_per_frame must be > 0");
    if (!d_out || !d_status) return fail(det, AGX_ERR_ARG, "d_out and d_status are the caller's: both are required");
    if (point_stride_bytes < 8 || (point_stride_bytes & 3)) return fail(det, AGX_ERR_ARG, "point_stride_bytes must be a multiple of 4 and at least 8");
    if ((((uintptr_t)d_points | (uintptr_t)d_counts | (uintptr_t)d_status_in | (uintptr_t)d_out | (uintptr_t)d_status) & 3))
        return fail(det, AGX_ERR_ARG, "points, counts, status and result buffers must be 4-byte aligned");
    if (const int rc = check_frame_batch(det, {d_frames, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format},
                                         {/*min_side*/ 1, /*lf32*/ true, /*lone_frame_stride*/ false, /*align16*/ true, /*front_rows*/ false}))
        return rc;
    if ((size_t)n_frames * points_per_frame >= ((size_t)1 << 31)) return fail(det, AGX_ERR_ARG, "at most 2^31 - 1 points per batch");
    HIP_TRY(det, hipSetDevice(det->device));
    begin_batch(det);  // and there is nothing of this one to be fetched
    const RefinePatchConsts *d_consts = nullptr;
    if (const int rc = ensure_patch_consts(det, &d_consts)) return rc;
    RefineWindowsArgs p{};
    p.frames = static_cast<const uint8_t *>(d_frames);
    p.frame_stride = (long long)frame_stride_bytes;
    p.row_stride = (int)row_stride_bytes;
    p.fmt = format;
    p.W = width;
    p.H = height;
    p.points = d_points;
    p.point_stride = point_stride_bytes;
    p.points_per_frame = points_per_frame;
    p.counts = d_counts;
    p.status_in = d_status_in;
    p.out = reinterpret_cast<float *>(d_out);
    p.status = d_status;
    p.factor = factor;
    p.scale = (float)factor;
    p.offset = 0.5f * (float)(factor - 1);
    p.radius = det->front_radius;  // the handle's sigma, as the chain's front has it
    static_assert(sizeof(p.w) == sizeof(det->front_w), "the taps of k_gauss_blur");
    std::memcpy(p.w, det->front_w, sizeof(p.w));
    const hipError_t e = (hipError_t)launch_refine_windows(p, d_consts + (half_size_patch - 1), half_size_patch, n_frames, det->stream);
    if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_refine_windows: ") + hipGetErrorString(e));
    return AGX_OK;
    });
}

int agx_rochade_refine_h(agx_detector *det, const void *pixels, int width, int height, size_t row_stride_bytes, int format, int image,
                         const void *points, uint32_t n_points, agx_saddle *out, uint32_t *status, uint32_t *n_refined, int half_size_patch)
{
    return agx_guard(det, [&]() -> int {
    if (!det) return AGX_ERR_ARG;
    if (half_size_patch < 1 || half_size_patch > REFINE_PATCH_MAX_HALF) return fail(det, AGX_ERR_ARG, "half_size_patch must be in 1 .. 4");
    if (!pixels || !n_refined || (n_points && (!points || !out || !status))) return fail(det, AGX_ERR_ARG, "null argument");
    if (image != AGX_REFINE_BLURRED && image != AGX_REFINE_PLANE) return fail(det, AGX_ERR_ARG, "image must be AGX_REFINE_BLURRED or AGX_REFINE_PLANE");
    if (image == AGX_REFINE_PLANE && format != AGX_LF32) return fail(det, AGX_ERR_FORMAT, "AGX_REFINE_PLANE takes an AGX_LF32 plane");
    if (image == AGX_REFINE_PLANE && (row_stride_bytes & 3)) return fail(det, AGX_ERR_ARG, "the row stride of an f32 plane must be a multiple of 4 bytes");
    FrameBatch b;
    int rc = stage_host_frame(det, pixels, width, height, row_stride_bytes, format, /*min_side*/ 1, /*lf32*/ true, /*upload*/ n_points != 0, b);
    if (rc) return rc;
    *n_refined = 0;
    if (!n_points) return AGX_OK;  // (the reference: an empty Vec; nothing was staged)
    agx_point *d_points = static_cast<agx_point *>(side_ensure(det, SB_REFINE_POINTS, (size_t)n_points * sizeof(agx_point), 0));
    if (!d_points) return fail(det, AGX_ERR_HIP, "hipMalloc: points");
    HIP_TRY(det, hipMemcpyAsync(d_points, points, (size_t)n_points * sizeof(agx_point), hipMemcpyHostToDevice, det->stream));
    rc = refine_points_enqueue_impl(det, b.frames, 1, width, height, b.row_stride, b.frame_stride, format, image, d_points, n_points, nullptr,
                                    nullptr, nullptr, half_size_patch);
    if (rc) return rc;
    rc = refine_points_fetch_impl(det, out, status);
    if (rc) return rc;
    uint32_t n = 0;
    for (uint32_t i = 0; i < n_points; ++i) n += status[i] == AGX_POINT_REFINED;
    *n_refined = n;
    return AGX_OK;
    });
}

int agx_rochade_refine(agx_detector *det, const void *pixels, int width, int height, size_t row_stride_bytes, int format, int image,
                       const void *points, uint32_t n_points, agx_saddle *out, uint32_t *status, uint32_t *n_refined)
{
    return agx_rochade_refine_h(det, pixels, width, height, row_stride_bytes, format, image, points, n_points, out, status, n_refined, 2);
}

}  // extern "C"

// ---- try_decode_quad of caller-given quads (src/detector.rs:448-476; csrc/detect_batch.cpp, tail_kernels.hip) ------------------
extern "C" {

int agx_decode_quads_enqueue(agx_detector *det, const void *d_frames, int n_frames, int width, int height, size_t row_stride_bytes,
                             size_t frame_stride_bytes, int format, const void *d_quads, size_t point_stride_bytes,
                             uint32_t quads_per_frame, const uint32_t *d_counts, const uint32_t *d_point_status, agx_tag *d_tags,
                             uint32_t *d_status, uint64_t *d_bits)
{
    return agx_guard(det, [&]() -> int {
    return decode_quads_enqueue_impl(det, d_frames, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format, d_quads,
                                     point_stride_bytes, quads_per_frame, d_counts, d_point_status, d_tags, d_status, d_bits);
    });
}

int agx_decode_quads_fetch(agx_detector *det, agx_tag *out, uint32_t *status, uint64_t *bits)
{
    return agx_guard(det, [&]() -> int { return decode_quads_fetch_impl(det, out, status, bits); });
}

int agx_decode_quads(agx_detector *det, const void *pixels, int width, int height, size_t row_stride_bytes, int format,
                     const void *quads, uint32_t n_quads, agx_tag *out, uint32_t *status, uint64_t *bits, uint32_t *n_decoded)
{
    return agx_guard(det, [&]() -> int {
    if (!det) return AGX_ERR_ARG;
    if (!pixels || !n_decoded || (n_quads && (!quads || !out || !status))) return fail(det, AGX_ERR_ARG, "null argument");
    FrameBatch b;
    int rc = stage_host_frame(det, pixels, width, height, row_stride_bytes, format, /*min_side*/ 1, /*lf32*/ false, /*upload*/ n_quads != 0, b);
    if (rc) return rc;
    *n_decoded = 0;
    if (!n_quads) return AGX_OK;  // (nothing was staged)
    void *d_quads = side_ensure(det, SB_DECODE_QUADS, (size_t)n_quads * 8 * sizeof(float), 0);
    if (!d_quads) return fail(det, AGX_ERR_HIP, "hipMalloc: quads");
    HIP_TRY(det, hipMemcpyAsync(d_quads, quads, (size_t)n_quads * 8 * sizeof(float), hipMemcpyHostToDevice, det->stream));
    rc = decode_quads_enqueue_impl(det, b.frames, 1, width, height, b.row_stride, b.frame_stride, format, d_quads, 8, n_quads, nullptr, nullptr,
                                   nullptr, nullptr, nullptr);
    if (rc) return rc;
    rc = decode_quads_fetch_impl(det, out, status, bits);
    if (rc) return rc;
    uint32_t n = 0;
    for (uint32_t i = 0; i < n_quads; ++i) n += status[i] == AGX_QUAD_DECODED;
    *n_decoded = n;
    return AGX_OK;
    });
}

int agx_decode_quads_tail(int family, const uint8_t *luma8, int width, int height, size_t row_stride_bytes, const void *quads,
                          uint32_t n_quads, agx_tag *out, uint32_t *status, uint64_t *bits, uint32_t *n_decoded)
{
    return agx_guard(nullptr, [&]() -> int {
    if (!luma8 || !n_decoded || (n_quads && (!quads || !out || !status)) || width < 1 || height < 1 || row_stride_bytes < (size_t)width)
        return AGX_ERR_ARG;
    FamilyInfo fam;
    if (!family_info(family, fam)) return AGX_ERR_FAMILY;
    uint32_t n = 0;
    for (uint32_t i = 0; i < n_quads; ++i) {
        float q[8];
        std::memcpy(q, static_cast<const char *>(quads) + (size_t)i * sizeof q, sizeof q);
        bool finite = true;
        for (float v : q) finite = finite && std::isfinite(v);
        agx_tag tag{};
        uint64_t b = 0;
        int id = 0;
        float corners[8];
        // a coordinate that is not finite: AGX_QUAD_OUTSIDE before anything is read (the reference's `as u32` would take NaN for 0)
        const int why = finite ? decode_quad(fam, luma8, (uint32_t)width, (uint32_t)height, row_stride_bytes, q, id, corners, b) : (int)AGX_QUAD_OUTSIDE;
        if (why == AGX_QUAD_DECODED) {
            tag.id = (uint32_t)id;
            std::memcpy(tag.xy, corners, sizeof corners);
            ++n;
        }
        out[i] = tag;
        status[i] = (uint32_t)why;
        if (bits) bits[i] = b;
    }
    *n_decoded = n;
    return AGX_OK;
    });
}

}  // extern "C"

// ---- the decode in three stages: decode_positions (src/detector.rs:42-72), bit_code (:74-122), best_tag (:142-169) -----------
// (csrc/detect_batch.cpp, decode_stages.hip; the host forms run the functions decode_quad is made of, csrc/host_tail.cpp)
extern "C" {

int agx_decode_positions_enqueue(agx_detector *det, const void *d_quads, size_t point_stride_bytes, int n_frames, uint32_t quads_per_frame,
                                 const uint32_t *d_counts, const uint32_t *d_point_status, uint32_t img_w, uint32_t img_h, int border_bits,
                                 int edge_bits, float margin, float *d_points, uint32_t *d_status)
{
    return agx_decode_positions_enqueue_m(det, d_quads, point_stride_bytes, n_frames, quads_per_frame, d_counts, d_point_status, img_w, img_h,
                                          border_bits, edge_bits, margin, d_points, d_status, AGX_TAG_MAP_AFFINE);
}

int agx_decode_positions_enqueue_m(agx_detector *det, const void *d_quads, size_t point_stride_bytes, int n_frames, uint32_t quads_per_frame,
                                   const uint32_t *d_counts, const uint32_t *d_point_status, uint32_t img_w, uint32_t img_h, int border_bits,
                                   int edge_bits, float margin, float *d_points, uint32_t *d_status, int model)
{
    return agx_guard(det, [&]() -> int {
    return decode_positions_enqueue_impl(det, d_quads, point_stride_bytes, n_frames, quads_per_frame, d_counts, d_point_status, img_w, img_h,
                                         border_bits, edge_bits, margin, d_points, d_status, model);
    });
}

int agx_decode_positions_tail(const void *quads, uint32_t n_quads, uint32_t img_w, uint32_t img_h, int border_bits, int edge_bits, float margin,
                              float *points, uint32_t *status)
{
    return agx_decode_positions_tail_m(quads, n_quads, img_w, img_h, border_bits, edge_bits, margin, points, status, AGX_TAG_MAP_AFFINE);
}

int agx_decode_positions_tail_m(const void *quads, uint32_t n_quads, uint32_t img_w, uint32_t img_h, int border_bits, int edge_bits, float margin,
                                float *points, uint32_t *status, int model)
{
    return agx_guard(nullptr, [&]() -> int {
    if ((n_quads && (!quads || !points || !status)) || !decode_square_ok(border_bits, edge_bits, margin) ||
        (model != AGX_TAG_MAP_AFFINE && model != AGX_TAG_MAP_HOMOGRAPHY))
        return AGX_ERR_ARG;
    const size_t per_slot = (size_t)(2 * edge_bits * edge_bits);
    for (uint32_t i = 0; i < n_quads; ++i) {
        float q[8], pts[2 * 64];
        std::memcpy(q, static_cast<const char *>(quads) + (size_t)i * sizeof q, sizeof q);
        bool finite = true;
        for (float v : q) finite = finite && std::isfinite(v);
        // a coordinate that is not finite: AGX_QUAD_OUTSIDE before anything else (the reference's `as u32` would take NaN for 0)
        int why = AGX_QUAD_OUTSIDE;
        if (finite)
            why = model == AGX_TAG_MAP_HOMOGRAPHY ? decode_positions_homography(img_w, img_h, q, border_bits, edge_bits, margin, pts)
                                                  : decode_positions(img_w, img_h, q, border_bits, edge_bits, margin, pts);
        if (why == AGX_QUAD_DECODED) std::memcpy(points + (size_t)i * per_slot, pts, per_slot * sizeof(float));
        status[i] = (uint32_t)why;
    }
    return AGX_OK;
    });
}

// tag_affine (src/image_util.rs:39-70) / tag_homography (src/image_util.rs:5-37) themselves (k_tag_maps is the device form)
int agx_tag_maps_enqueue(agx_detector *det, const void *d_quads, size_t point_stride_bytes, int n_frames, uint32_t quads_per_frame,
                         const uint32_t *d_counts, const uint32_t *d_point_status, int side_bits, float margin, int model, float *d_maps,
                         uint32_t *d_status)
{
    return agx_guard(det, [&]() -> int {
    return tag_maps_enqueue_impl(det, d_quads, point_stride_bytes, n_frames, quads_per_frame, d_counts, d_point_status, side_bits, margin, model,
                                 d_maps, d_status);
    });
}

int agx_tag_maps_tail(const void *quads, uint32_t n_quads, int side_bits, float margin, int model, float *maps, uint32_t *status)
{
    return agx_guard(nullptr, [&]() -> int {
    if ((n_quads && (!quads || !maps || !status)) || !tag_square_ok(side_bits, margin) || (model != AGX_TAG_MAP_AFFINE && model != AGX_TAG_MAP_HOMOGRAPHY))
        return AGX_ERR_ARG;
    for (uint32_t i = 0; i < n_quads; ++i) {
        float q[8], h[9];
        std::memcpy(q, static_cast<const char *>(quads) + (size_t)i * sizeof q, sizeof q);
        bool finite = true;
        for (float v : q) finite = finite && std::isfinite(v);
        uint32_t why = finite ? AGX_QUAD_DECODED : AGX_QUAD_OUTSIDE;
        if (finite) {
            if (model == AGX_TAG_MAP_HOMOGRAPHY) {
                if (!tag_homography(q, side_bits, margin, h)) why = AGX_QUAD_DEGENERATE;
            } else {
                tag_affine(q, side_bits, margin, h);
                h[6] = 0.0f;
                h[7] = 0.0f;
                h[8] = 1.0f;
            }
        }
        if (why == AGX_QUAD_DECODED) std::memcpy(maps + (size_t)i * 9, h, sizeof h);
        status[i] = why;
    }
    return AGX_OK;
    });
}

int agx_bit_code_enqueue(agx_detector *det, const void *d_frames, int n_frames, int width, int height, size_t row_stride_bytes,
                         size_t frame_stride_bytes, int format, const float *d_points, uint32_t points_per_slot, uint32_t quads_per_frame,
                         const uint32_t *d_counts, const uint32_t *d_status_in, int valid_brightness_threshold, uint32_t max_invalid_bit,
                         uint64_t *d_bits, uint32_t *d_status)
{
    return agx_guard(det, [&]() -> int {
    return bit_code_enqueue_impl(det, d_frames, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format, d_points, points_per_slot,
                                 quads_per_frame, d_counts, d_status_in, valid_brightness_threshold, max_invalid_bit, d_bits, d_status);
    });
}

int agx_bit_code_tail(const uint8_t *luma8, int width, int height, size_t row_stride_bytes, const float *points, uint32_t points_per_slot,
                      uint32_t n_slots, const uint32_t *status_in, int valid_brightness_threshold, uint32_t max_invalid_bit, uint64_t *bits,
                      uint32_t *status)
{
    return agx_guard(nullptr, [&]() -> int {
    if (!luma8 || width < 1 || height < 1 || row_stride_bytes < (size_t)width || (n_slots && (!points || !bits || !status)) || points_per_slot < 1 ||
        points_per_slot > 64 || valid_brightness_threshold < 0 || valid_brightness_threshold > 255)
        return AGX_ERR_ARG;
    for (uint32_t i = 0; i < n_slots; ++i) {
        uint64_t b = 0;
        uint32_t why = status_in ? status_in[i] : (uint32_t)AGX_QUAD_DECODED;
        if (why == AGX_QUAD_DECODED) {
            const float *pts = points + (size_t)i * 2 * points_per_slot;
            bool finite = true;
            for (uint32_t k = 0; k < 2 * points_per_slot; ++k) finite = finite && std::isfinite(pts[k]);
            // a sample coordinate that is not finite: AGX_QUAD_OUTSIDE before any read, as for a quad's corners
            why = finite ? (uint32_t)bit_code(luma8, (uint32_t)width, (uint32_t)height, row_stride_bytes, pts, (int)points_per_slot,
                                              valid_brightness_threshold, max_invalid_bit, b)
                         : (uint32_t)AGX_QUAD_OUTSIDE;
        }
        bits[i] = b;
        status[i] = why;
    }
    return AGX_OK;
    });
}

int agx_best_tag_enqueue(agx_detector *det, const uint64_t *d_bits, uint32_t n_slots, uint32_t quads_per_frame, const uint32_t *d_counts,
                         const uint32_t *d_status_in, int thres, const uint64_t *d_codes, uint32_t n_codes, int edge_bits, const void *d_quads,
                         size_t point_stride_bytes, uint32_t *d_ids, uint32_t *d_rotations, uint32_t *d_status, agx_tag *d_tags)
{
    return agx_guard(det, [&]() -> int {
    return best_tag_enqueue_impl(det, d_bits, n_slots, quads_per_frame, d_counts, d_status_in, thres, d_codes, n_codes, edge_bits, d_quads,
                                 point_stride_bytes, d_ids, d_rotations, d_status, d_tags);
    });
}

int agx_best_tag_tail(const uint64_t *bits, uint32_t n_slots, const uint32_t *status_in, int thres, int family, const uint64_t *codes,
                      uint32_t n_codes, int edge_bits, const void *quads, uint32_t *ids, uint32_t *rotations, uint32_t *status, agx_tag *tags)
{
    return agx_guard(nullptr, [&]() -> int {
    if ((n_slots && (!bits || !ids || !rotations || !status)) || thres < 0 || thres > 255 || edge_bits < 1 || edge_bits > 8 ||
        (codes ? (n_codes < 1 || n_codes > 65535) : n_codes != 0) || (quads == nullptr) != (tags == nullptr))
        return AGX_ERR_ARG;
    if (!codes) {
        FamilyInfo fam;
        if (!family_info(family, fam)) return AGX_ERR_FAMILY;
        codes = fam.codes;
        n_codes = (uint32_t)fam.n_codes;
    }
    for (uint32_t i = 0; i < n_slots; ++i) {
        uint32_t why = status_in ? status_in[i] : (uint32_t)AGX_QUAD_DECODED;
        int idx = 0, rot = 0;
        if (why == AGX_QUAD_DECODED && !best_tag(bits[i], thres, codes, (int)n_codes, edge_bits, idx, rot)) {
            why = AGX_QUAD_NO_MATCH;
            idx = rot = 0;
        }
        const bool hit = why == AGX_QUAD_DECODED;
        ids[i] = hit ? (uint32_t)idx : 0u;
        rotations[i] = hit ? (uint32_t)rot : 0u;
        status[i] = why;
        if (tags) {
            agx_tag tag{};
            if (hit) {  // rotate_left(rot) then reverse, :468-469
                const float *q = static_cast<const float *>(quads) + (size_t)i * 8;
                tag.id = (uint32_t)idx;
                for (int c = 0; c < 4; ++c) {
                    const int src = ((3 - c) + rot) & 3;
                    std::memcpy(&tag.xy[2 * c], q + 2 * src, 2 * sizeof(float));
                }
            }
            tags[i] = tag;
        }
    }
    return AGX_OK;
    });
}

}  // extern "C"

// ---- try_find_best_board of caller-given saddle lists (src/detector.rs:588-639; csrc/detect_batch.cpp, tail_kernels.hip) -------
// The ending of agx_find_board_tail, agx_grow_board_tail and agx_init_quads_tail: the host form's rows (slot numbers, four per
// quad) and status `st` for a caller with room for `cap` quads.  A board with more is AGX_BOARD_CAPACITY with its true count and
// no rows.  -> the status written.
static uint32_t tail_rows_out(int st, const std::vector<uint32_t> &rows, uint32_t *quads, uint32_t cap, uint32_t *n_quads, uint32_t *status)
{
    const uint32_t n = (uint32_t)(rows.size() / 4);
    if (st == AGX_BOARD_FOUND && n > cap) st = AGX_BOARD_CAPACITY;
    if (st == AGX_BOARD_FOUND && n) std::memcpy(quads, rows.data(), rows.size() * sizeof(uint32_t));
    *n_quads = st == AGX_BOARD_FOUND || st == AGX_BOARD_CAPACITY ? n : 0u;
    *status = (uint32_t)st;
    return (uint32_t)st;
}

extern "C" {

int agx_find_boards_enqueue(agx_detector *det, const void *d_saddles, size_t saddle_stride_bytes, int n_frames, uint32_t saddles_per_frame,
                            const uint32_t *d_counts, const void *d_frame_table, const uint32_t *d_point_status, uint32_t quads_per_frame,
                            uint32_t *d_quads, float *d_quad_points, uint32_t *d_n_quads, uint32_t *d_status)
{
    return agx_guard(det, [&]() -> int {
    return find_boards_enqueue_impl(det, d_saddles, saddle_stride_bytes, n_frames, saddles_per_frame, d_counts, d_frame_table, d_point_status,
                                    quads_per_frame, d_quads, d_quad_points, d_n_quads, d_status);
    });
}

int agx_find_boards_fetch(agx_detector *det, uint32_t *quads, float *quad_points, uint32_t *n_quads, uint32_t *status, int n_threads)
{
    return agx_guard(det, [&]() -> int { return find_boards_fetch_impl(det, quads, quad_points, n_quads, status, n_threads); });
}

int agx_find_board(agx_detector *det, const agx_saddle *saddles, uint32_t n_saddles, uint32_t *quads, uint32_t cap, uint32_t *n_quads,
                   uint32_t *status)
{
    return agx_guard(det, [&]() -> int {
    if (!det) return AGX_ERR_ARG;
    if (!n_quads || !status || (n_saddles && !saddles) || (cap && !quads)) return fail(det, AGX_ERR_ARG, "null argument");
    *n_quads = 0;
    *status = AGX_BOARD_NONE;
    if (!n_saddles) return AGX_OK;
    HIP_TRY(det, hipSetDevice(det->device));
    void *d_list = side_ensure(det, SB_FIND_SADDLES, (size_t)n_saddles * sizeof(agx_saddle), 0);
    if (!d_list) return fail(det, AGX_ERR_HIP, "hipMalloc: saddles");
    HIP_TRY(det, hipMemcpyAsync(d_list, saddles, (size_t)n_saddles * sizeof(agx_saddle), hipMemcpyHostToDevice, det->stream));
    // rows for the caller's cap: a board with more quads is AGX_BOARD_CAPACITY with its true count, as in a batch
    const uint32_t qpf = cap ? cap : 1u;
    int rc = find_boards_enqueue_impl(det, d_list, sizeof(agx_saddle), 1, n_saddles, nullptr, nullptr, nullptr, qpf, nullptr, nullptr, nullptr, nullptr);
    if (rc) return rc;
    std::vector<uint32_t> rows((size_t)qpf * 4);
    uint32_t n = 0, st = 0;
    rc = find_boards_fetch_impl(det, rows.data(), nullptr, &n, &st, 1);
    if (rc) return rc;
    if (st == AGX_BOARD_FOUND && n > cap) st = AGX_BOARD_CAPACITY;
    if (st == AGX_BOARD_FOUND && n) std::memcpy(quads, rows.data(), (size_t)n * 4 * sizeof(uint32_t));
    *n_quads = n;
    *status = st;
    return AGX_OK;
    });
}

int agx_find_board_tail(const agx_saddle *saddles, uint32_t n_saddles, uint32_t *quads, uint32_t cap, uint32_t *n_quads, uint32_t *status)
{
    return agx_guard(nullptr, [&]() -> int {
    if (!n_quads || !status || (n_saddles && !saddles) || (cap && !quads)) return AGX_ERR_ARG;
    std::vector<uint32_t> rows;
    const int st = find_board_in_slots(saddles, sizeof(agx_saddle), n_saddles, nullptr, rows);
    tail_rows_out(st, rows, quads, cap, n_quads, status);
    return AGX_OK;
    });
}

// ---- candidate quads of caller-given seed saddles (src/detector.rs:543-586; csrc/detect_batch.cpp, tail_kernels.hip: k_init_quads) ----
int agx_init_quads_enqueue(agx_detector *det, const void *d_saddles, size_t saddle_stride_bytes, int n_frames, uint32_t saddles_per_frame,
                           const uint32_t *d_counts, const void *d_frame_table, const uint32_t *d_point_status, const uint32_t *d_seed_saddles,
                           uint32_t seeds_per_frame, const uint32_t *d_seed_counts, uint32_t n_nearest, uint32_t quads_per_frame,
                           uint32_t *d_quads, float *d_quad_points, uint32_t *d_n_quads, uint32_t *d_status, uint32_t *d_seed_quad_counts,
                           uint32_t *d_seeds_out, uint32_t *d_n_seeds_out)
{
    return agx_guard(det, [&]() -> int {
    return init_quads_enqueue_impl(det, d_saddles, saddle_stride_bytes, n_frames, saddles_per_frame, d_counts, d_frame_table, d_point_status,
                                   d_seed_saddles, seeds_per_frame, d_seed_counts, n_nearest, quads_per_frame, d_quads, d_quad_points,
                                   d_n_quads, d_status, d_seed_quad_counts, d_seeds_out, d_n_seeds_out);
    });
}

int agx_init_quads_fetch(agx_detector *det, int n_threads)
{
    return agx_guard(det, [&]() -> int { return init_quads_fetch_impl(det, n_threads); });
}

int agx_init_quads_tail(const agx_saddle *saddles, uint32_t n_saddles, const uint32_t *point_status, const uint32_t *seed_saddles,
                        uint32_t n_seeds, uint32_t max_seeds, uint32_t n_nearest, uint32_t *quads, uint32_t cap, uint32_t *n_quads,
                        uint32_t *status, uint32_t *seed_quad_counts, uint32_t *seeds_out, uint32_t *n_seeds_out)
{
    return agx_guard(nullptr, [&]() -> int {
    if (!n_quads || !status || (n_saddles && !saddles) || (cap && !quads) || (n_seeds && !seed_saddles)) return AGX_ERR_ARG;
    if (!max_seeds || n_nearest < 2 || n_nearest > 64) return AGX_ERR_ARG;
    std::vector<uint32_t> rows, counts, seeds;
    const uint32_t st = tail_rows_out(init_quads_in_slots(saddles, sizeof(agx_saddle), n_saddles, point_status, seed_saddles, n_seeds, max_seeds,
                                                          n_nearest, rows, counts, seeds),
                                      rows, quads, cap, n_quads, status);
    if (n_seeds_out) *n_seeds_out = (uint32_t)seeds.size();
    if (st != AGX_BOARD_INPUT) {
        if (seed_quad_counts) std::memcpy(seed_quad_counts, counts.data(), counts.size() * sizeof(uint32_t));
        if (seeds_out && !seeds.empty()) std::memcpy(seeds_out, seeds.data(), seeds.size() * sizeof(uint32_t));
    }
    return AGX_OK;
    });
}

// ---- boards from the caller's seed quads (src/board.rs:26-112; csrc/detect_batch.cpp, tail_kernels.hip: k_grow_boards) ----------
int agx_grow_boards_enqueue(agx_detector *det, const void *d_saddles, size_t saddle_stride_bytes, int n_frames, uint32_t saddles_per_frame,
                            const uint32_t *d_counts, const void *d_frame_table, const uint32_t *d_point_status, const uint32_t *d_seed_quads,
                            uint32_t seeds_per_frame, const uint32_t *d_seed_counts, float spacing_ratio, uint32_t stop_score, int flags,
                            uint32_t quads_per_frame, uint32_t *d_quads, float *d_quad_points, uint32_t *d_n_quads, uint32_t *d_status,
                            uint32_t *d_seed_scores, uint32_t *d_best_seed)
{
    return agx_guard(det, [&]() -> int {
    return grow_boards_enqueue_impl(det, d_saddles, saddle_stride_bytes, n_frames, saddles_per_frame, d_counts, d_frame_table, d_point_status,
                                    d_seed_quads, seeds_per_frame, d_seed_counts, spacing_ratio, stop_score, flags, quads_per_frame, d_quads,
                                    d_quad_points, d_n_quads, d_status, d_seed_scores, d_best_seed);
    });
}

int agx_grow_boards_fetch(agx_detector *det, int n_threads)
{
    return agx_guard(det, [&]() -> int { return grow_boards_fetch_impl(det, n_threads); });
}

int agx_grow_board_tail(const agx_saddle *saddles, uint32_t n_saddles, const uint32_t *point_status, const uint32_t *seed_quads, uint32_t n_seeds,
                        float spacing_ratio, uint32_t stop_score, int flags, uint32_t *quads, uint32_t cap, uint32_t *n_quads, uint32_t *status,
                        uint32_t *seed_scores, uint32_t *best_seed)
{
    return agx_guard(nullptr, [&]() -> int {
    if (!n_quads || !status || (n_saddles && !saddles) || (cap && !quads) || (n_seeds && !seed_quads)) return AGX_ERR_ARG;
    if (!std::isfinite(spacing_ratio) || !(1.0f + spacing_ratio > 0.0f) || (flags & ~AGX_GROW_FIX_MISSING)) return AGX_ERR_ARG;
    std::vector<uint32_t> rows, scores;
    uint32_t best = 0;
    const uint32_t st = tail_rows_out(grow_boards_in_slots(saddles, sizeof(agx_saddle), n_saddles, point_status, seed_quads, n_seeds, spacing_ratio,
                                                           stop_score, flags, rows, scores, best),
                                      rows, quads, cap, n_quads, status);
    const bool some = st == AGX_BOARD_FOUND || st == AGX_BOARD_CAPACITY;
    if (some && seed_scores && n_seeds) std::memcpy(seed_scores, scores.data(), (size_t)n_seeds * sizeof(uint32_t));
    if (some && best_seed) *best_seed = best;
    return AGX_OK;
    });
}

// ---- caller points snapped to the nearest listed saddle (csrc/detect_batch.cpp, tail_kernels.hip: k_snap_points) ----------------
int agx_snap_points_enqueue(agx_detector *det, const void *d_saddles, size_t saddle_stride_bytes, int n_frames, uint32_t saddles_per_frame,
                            const uint32_t *d_counts, const void *d_frame_table, const uint32_t *d_point_status, const void *d_points,
                            size_t row_stride_bytes, size_t point_stride_bytes, uint32_t rows_per_frame, uint32_t points_per_row,
                            const uint32_t *d_row_counts, float max_dist_sq, int flags, uint32_t *d_slots, float *d_dist_sq, uint32_t *d_rows,
                            uint32_t *d_n_rows, uint32_t *d_row_index, uint32_t *d_status)
{
    return agx_guard(det, [&]() -> int {
    return snap_points_enqueue_impl(det, d_saddles, saddle_stride_bytes, n_frames, saddles_per_frame, d_counts, d_frame_table, d_point_status,
                                    d_points, row_stride_bytes, point_stride_bytes, rows_per_frame, points_per_row, d_row_counts, max_dist_sq,
                                    flags, d_slots, d_dist_sq, d_rows, d_n_rows, d_row_index, d_status);
    });
}

int agx_snap_points_tail(const agx_saddle *saddles, uint32_t n_saddles, const uint32_t *point_status, const void *points, size_t row_stride_bytes,
                         size_t point_stride_bytes, uint32_t n_rows, uint32_t points_per_row, float max_dist_sq, int flags, uint32_t *slots,
                         float *dist_sq, uint32_t *rows, uint32_t *n_rows_out, uint32_t *row_index, uint32_t *status)
{
    return agx_guard(nullptr, [&]() -> int {
    if (!n_rows_out || !status || (n_saddles && !saddles) || (n_rows && (!points || !slots || !rows))) return AGX_ERR_ARG;
    if (!snap_point_args_ok(row_stride_bytes, point_stride_bytes, points_per_row, max_dist_sq, flags)) return AGX_ERR_ARG;
    if (((uintptr_t)saddles | (uintptr_t)point_status | (uintptr_t)points | (uintptr_t)slots | (uintptr_t)dist_sq | (uintptr_t)rows |
         (uintptr_t)row_index) & 3)
        return AGX_ERR_ARG;
    if (n_rows >= (1u << 27)) return AGX_ERR_ARG;
    *status = snap_points(saddles, sizeof(agx_saddle), n_saddles, point_status, points, row_stride_bytes, point_stride_bytes, n_rows,
                          points_per_row, max_dist_sq, flags, slots, dist_sq, rows, n_rows_out, row_index);
    return AGX_OK;
    });
}

}  // extern "C"

// ---- gaussian_blur_f32 / hessian_response as planes (src/image_util.rs:110-206, :72-109; chain_kernels.hip) ---------------------
static int planes_enqueue_impl(agx_detector *det, const void *d_frames, int n_frames, int width, int height, size_t row_stride_bytes,
                               size_t frame_stride_bytes, int format, float sigma, float *d_blur, float *d_response,
                               size_t out_row_stride_bytes, size_t out_frame_stride_bytes)
{
    if (!det) return AGX_ERR_ARG;
    if (!d_blur && !d_response) return fail(det, AGX_ERR_ARG, "d_blur and d_response are both NULL");
    if (sigma != 0.0f && !blur_sigma_ok(sigma)) return fail(det, AGX_ERR_ARG, "sigma must be 0 (no blur) or positive and finite with ceil(2 sigma) <= 16");
    if (sigma == 0.0f && d_blur) return fail(det, AGX_ERR_ARG, "sigma 0 means no blur: d_blur must be NULL");
    FrameBatch b{d_frames, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format};
    if (const int rc = check_frame_batch(det, b, {/*min_side*/ 1, /*lf32*/ true, /*lone_frame_stride*/ false, /*align16*/ true, /*front_rows*/ true}))
        return rc;
    // (at most 0x7fffffff, as the frames' row stride: k_hessian_response reads the blur plane back with an int row stride in bytes)
    if (out_row_stride_bytes < 4 * (size_t)width || (out_row_stride_bytes & 3) || out_row_stride_bytes > 0x7fffffffu)
        return fail(det, AGX_ERR_ARG, "out_row_stride_bytes must be a multiple of 4, cover width floats and be below 2^31");
    if (out_frame_stride_bytes < (size_t)height * out_row_stride_bytes || (out_frame_stride_bytes & 3))
        return fail(det, AGX_ERR_ARG, "out_frame_stride_bytes must be a multiple of 4 and cover height rows");
    if (((uintptr_t)d_blur | (uintptr_t)d_response) & 3) return fail(det, AGX_ERR_ARG, "the output planes must be 4-byte aligned");
    HIP_TRY(det, hipSetDevice(det->device));
    begin_batch(det);  // and there is nothing of this one to be fetched
    if (format_front(format))  // as the chain: k_front_luma's integer luma plane, read as L8 / L16
        if (const int rc = front_luma_plane(det, b)) return rc;
    format = b.format;
    HessianArgs h{};
    h.src = static_cast<const uint8_t *>(b.frames);
    h.src_frame_stride = (long long)b.frame_stride;
    h.src_row_stride = (int)b.row_stride;
    int h_format = format;
    if (sigma != 0.0f) {
        GaussBlurArgs g{};
        g.src = h.src;
        g.src_frame_stride = h.src_frame_stride;
        g.src_row_stride = h.src_row_stride;
        g.W = width;
        g.H = height;
        g.dst = d_blur;
        g.dst_row_stride = (long long)(out_row_stride_bytes / 4);
        g.dst_frame_stride = (long long)(out_frame_stride_bytes / 4);
        if (!d_blur) {  // only the response is wanted: the blur goes to the workspace plane, tight
            g.dst = static_cast<float *>(side_ensure(det, SB_PLANES_BLUR, (size_t)n_frames * (size_t)width * (size_t)height * sizeof(float), 0));
            if (!g.dst) return fail(det, AGX_ERR_HIP, "hipMalloc: blur planes");
            g.dst_row_stride = width;
            g.dst_frame_stride = (long long)width * height;
        }
        g.radius = make_blur_weights(sigma, g.w);
        hipError_t e = (hipError_t)launch_gauss_blur(g, format, n_frames, det->stream);
        if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_gauss_blur: ") + hipGetErrorString(e));
        h.src = reinterpret_cast<const uint8_t *>(g.dst);
        h.src_frame_stride = g.dst_frame_stride * 4;
        h.src_row_stride = (int)(g.dst_row_stride * 4);
        h_format = AGX_LF32;
    }
    if (d_response) {
        h.W = width;
        h.H = height;
        h.dst = d_response;
        h.dst_row_stride = (long long)(out_row_stride_bytes / 4);
        h.dst_frame_stride = (long long)(out_frame_stride_bytes / 4);
        hipError_t e = (hipError_t)launch_hessian_response(h, h_format, n_frames, det->stream);
        if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_hessian_response: ") + hipGetErrorString(e));
    }
    return AGX_OK;
}

// agx_gaussian_blur_f32 / agx_hessian_response: upload, a batch of one, the plane (blur, or with want_response the response) down
static int planes_host_impl(agx_detector *det, const void *pixels, int width, int height, size_t row_stride_bytes, int format, float sigma,
                            bool want_response, float *out)
{
    if (!det) return AGX_ERR_ARG;
    if (!out) return fail(det, AGX_ERR_ARG, "null argument");
    FrameBatch b;
    int rc = stage_host_frame(det, pixels, width, height, row_stride_bytes, format, /*min_side*/ 1, /*lf32*/ true, /*upload*/ true, b);
    if (rc) return rc;
    const size_t plane_bytes = (size_t)width * (size_t)height * sizeof(float);
    float *d_plane = static_cast<float *>(side_ensure(det, SB_PLANES_OUT, plane_bytes, 0));
    if (!d_plane) return fail(det, AGX_ERR_HIP, "hipMalloc: plane");
    rc = planes_enqueue_impl(det, b.frames, 1, width, height, b.row_stride, b.frame_stride, format, sigma, want_response ? nullptr : d_plane,
                             want_response ? d_plane : nullptr, (size_t)width * sizeof(float), plane_bytes);
    if (rc) return rc;
    HIP_TRY(det, hipMemcpyAsync(out, d_plane, plane_bytes, hipMemcpyDeviceToHost, det->stream));
    HIP_TRY(det, hipStreamSynchronize(det->stream));
    return AGX_OK;
}

extern "C" {

int agx_planes_enqueue(agx_detector *det, const void *d_frames, int n_frames, int width, int height, size_t row_stride_bytes,
                       size_t frame_stride_bytes, int format, float sigma, float *d_blur, float *d_response,
                       size_t out_row_stride_bytes, size_t out_frame_stride_bytes)
{
    return agx_guard(det, [&]() -> int {
    return planes_enqueue_impl(det, d_frames, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format, sigma, d_blur,
                               d_response, out_row_stride_bytes, out_frame_stride_bytes);
    });
}

int agx_gaussian_blur_f32(agx_detector *det, const void *pixels, int width, int height, size_t row_stride_bytes, int format, float sigma,
                          float *out)
{
    return agx_guard(det, [&]() -> int {
    if (det && !blur_sigma_ok(sigma)) return fail(det, AGX_ERR_ARG, "sigma must be positive and finite with ceil(2 sigma) <= 16");
    return planes_host_impl(det, pixels, width, height, row_stride_bytes, format, sigma, false, out);
    });
}

int agx_hessian_response(agx_detector *det, const void *pixels, int width, int height, size_t row_stride_bytes, int format, float *out)
{
    return agx_guard(det, [&]() -> int {
    return planes_host_impl(det, pixels, width, height, row_stride_bytes, format, 0.0f, true, out);
    });
}

int agx_debug_blur_weights(float sigma, float *weights, int cap, int *radius)
{
    return agx_guard(nullptr, [&]() -> int {
    if (!weights || !radius || !blur_sigma_ok(sigma)) return AGX_ERR_ARG;
    *radius = blur_radius(sigma);
    if (cap < 2 * *radius + 1) return AGX_ERR_CAPACITY;
    make_blur_weights(sigma, weights);
    return AGX_OK;
    });
}

int agx_debug_refine_constants(int half_size_patch, float *cone, float *pmat, int cap_points, int *n_points)
{
    return agx_guard(nullptr, [&]() -> int {
    if (!cone || !pmat || !n_points || half_size_patch < 1 || half_size_patch > REFINE_PATCH_MAX_HALF) return AGX_ERR_ARG;
    const int ks = 2 * half_size_patch + 1;
    *n_points = ks * ks;
    if (cap_points < *n_points) return AGX_ERR_CAPACITY;
    RefinePatchConsts rc;
    make_refine_patch_consts(half_size_patch, rc);
    std::memcpy(cone, rc.cone, (size_t)*n_points * sizeof(float));
    std::memcpy(pmat, rc.pmat, (size_t)*n_points * 6 * sizeof(float));
    return AGX_OK;
    });
}

}  // extern "C"

// ---- cluster centres of caller-given response planes, the k / phi filter (src/detector.rs:414-429, :432-445; chain_kernels.hip) --
// The launches of the deferred plan's clustering (enqueue_chunk) behind a front that reads the caller's plane, and an emission of
// the cluster table instead of a refinement: k_plane_front x 2, k_verify_seeds, k_flood_refine<.., false>, k_generic_cluster,
// k_emit_clusters.  Nothing of it reads a.blur or a.frames.
// What the entry refuses, before anything is allocated, uploaded or replaced (`plane` is the batch's planes wherever they lie).
static int clusters_check_args(agx_detector *det, const float *plane, int n_frames, int width, int height, size_t row_stride_bytes,
                               size_t frame_stride_bytes, uint32_t clusters_per_frame, const agx_cluster_info *d_clusters,
                               const void *d_points, const uint32_t *d_counts, const uint32_t *d_status)
{
    const bool any = d_clusters || d_counts || d_status, all = d_clusters && d_counts && d_status;
    if (any != all) return fail(det, AGX_ERR_ARG, "d_clusters, d_counts and d_status: all or none");
    if (!clusters_per_frame || clusters_per_frame > EMIT_CLUSTERS_MAX) return fail(det, AGX_ERR_ARG, "clusters_per_frame must be in 1 .. 16384");
    if (((uintptr_t)d_clusters | (uintptr_t)d_points | (uintptr_t)d_counts | (uintptr_t)d_status) & 3)
        return fail(det, AGX_ERR_ARG, "the result buffers must be 4-byte aligned");
    return check_frame_batch(det, {plane, n_frames, width, height, row_stride_bytes, frame_stride_bytes, AGX_LF32},
                             {/*min_side*/ 2, /*lf32*/ true, /*lone_frame_stride*/ true, /*align16*/ false, /*front_rows*/ false});
}

static int clusters_enqueue_impl(agx_detector *det, const float *d_response, int n_frames, int width, int height, size_t row_stride_bytes,
                                 size_t frame_stride_bytes, uint32_t clusters_per_frame, agx_cluster_info *d_clusters, void *d_points,
                                 uint32_t *d_counts, uint32_t *d_status)
{
    if (!det) return AGX_ERR_ARG;
    if (const int rc = clusters_check_args(det, d_response, n_frames, width, height, row_stride_bytes, frame_stride_bytes, clusters_per_frame,
                                           d_clusters, d_points, d_counts, d_status))
        return rc;
    const bool all = d_clusters != nullptr;
    const size_t slots = (size_t)n_frames * clusters_per_frame;
    HIP_TRY(det, hipSetDevice(det->device));
    begin_batch(det);
    if (const int rc = ensure_workspace(det, n_frames, width, height)) return rc;
    EmitClustersArgs e{};
    e.per_frame = clusters_per_frame;
    if (!all) {
        if (!side_ensure(det, SB_CLUSTERS_ROWS, slots * sizeof(agx_cluster_info), 0) || !side_ensure(det, SB_CLUSTERS_COUNTS, (size_t)n_frames * 4, 0) ||
            !side_ensure(det, SB_CLUSTERS_STATUS, (size_t)n_frames * 4, 0) || (!d_points && !side_ensure(det, SB_CLUSTERS_POINTS, slots * sizeof(agx_point), 0)))
            return fail(det, AGX_ERR_HIP, "hipMalloc: cluster rows");
        e.rows = det->side[SB_CLUSTERS_ROWS].ptr<uint32_t>();
        e.counts = det->side[SB_CLUSTERS_COUNTS].ptr<uint32_t>();
        e.status = det->side[SB_CLUSTERS_STATUS].ptr<uint32_t>();
        e.points = d_points ? static_cast<float *>(d_points) : det->side[SB_CLUSTERS_POINTS].ptr<float>();
    } else {
        e.rows = reinterpret_cast<uint32_t *>(d_clusters);
        e.counts = d_counts;
        e.status = d_status;
        e.points = static_cast<float *>(d_points);
    }
    ChainArgs &a = det->args;
    a.frames = reinterpret_cast<const uint8_t *>(d_response);  // (for the record: no kernel of this batch reads it through `a`)
    a.frame_stride = (long long)frame_stride_bytes;
    a.row_stride = (int)row_stride_bytes;
    a.byte_rows = 0;
    a.fmt = AGX_LF32;
    a.W = width;
    a.H = height;
    a.n_frames = n_frames;
    a.plane = (long long)width * height;
    a.min_angle = det->params.min_saddle_angle;
    a.max_angle = det->params.max_saddle_angle;
    a.out = det->d_out_internal;
    a.out_total_cap = (uint32_t)std::min<size_t>((size_t)n_frames * a.cap_out, 0xffffffffu);
    a.frame_table = nullptr;
    det->external_out = false;
    det->out_in_host = false;
    a.force_generic = det->force_generic;
    a.sparse_after_verify = 0;
    a.dbg = 0;  // (the measurement switches instrument the chain's own batches)
    a.wave_times = nullptr;
    a.resp_dbg = nullptr;
    det->resp_stored = false;
    // the counters, as enqueue_blur_only: no kernel of this batch clears the other set, so neither is known to be clear afterwards
    const int p = det->ctr_cur ^ 1;
    const size_t need = (size_t)n_frames + 1;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(det->stream, &cap);
    if (cap == hipStreamCaptureStatusActive) {  // (a replayed graph clears its own set every time)
        HIP_TRY(det, (hipError_t)launch_clear_counters(det->d_ctr[p], need, det->stream));
    } else if (det->ctr_cleared[p] < need) {
        HIP_TRY(det, hipMemsetAsync(det->d_ctr[p], 0, need * sizeof(FrameCounters), det->stream));
    }
    det->ctr_cleared[0] = det->ctr_cleared[1] = 0;
    a.ctr = det->d_ctr[p];
    a.ctr_next = det->d_ctr[p ^ 1];
    a.total_out = &a.ctr[n_frames].min_key_inv;
    det->ctr_cur = p;
    const PlaneFrontArgs front{d_response, (long long)(frame_stride_bytes / 4), (long long)(row_stride_bytes / 4)};
    // profiling level 2: the two new kernels between events of their own (XT_*; an event pair costs the stream a gap on either
    // side, so the whole entry is measured with profiling off)
    const EventPair ev_front = extra_timer_begin(det, det->stream, XT_PLANE_FRONT);
    hipError_t err = (hipError_t)launch_plane_front(a, front, det->stream);
    extra_timer_end(det, det->stream, ev_front);
    if (err != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("launch k_plane_front: ") + hipGetErrorString(err));
    err = (hipError_t)launch_kernel(K_THRESHOLD, a, det->rc, det->stream, true);
    if (err != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("launch k_verify_seeds: ") + hipGetErrorString(err));
    err = (hipError_t)launch_kernel(K_FLOOD_REFINE, a, det->rc, det->stream, true);
    if (err != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("launch k_flood_refine: ") + hipGetErrorString(err));
    err = (hipError_t)launch_generic_cluster(a, det->stream);
    if (err != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("launch k_generic_cluster: ") + hipGetErrorString(err));
    const EventPair ev_emit = extra_timer_begin(det, det->stream, XT_EMIT_CLUSTERS);
    err = (hipError_t)launch_emit_clusters(a, e, det->stream);
    extra_timer_end(det, det->stream, ev_emit);
    if (err != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("launch k_emit_clusters: ") + hipGetErrorString(err));
    det->batch = BATCH_CLUSTERS;
    det->clusters.results = all ? RESULTS_CALLER : RESULTS_HOST;
    det->clusters.n_frames = n_frames;
    det->clusters.clusters_per_frame = clusters_per_frame;
    det->clusters.d_points = all ? nullptr : reinterpret_cast<const agx_point *>(e.points);
    return AGX_OK;
}

static int clusters_fetch_impl(agx_detector *det, agx_cluster_info *clusters, void *points, uint32_t *counts, uint32_t *status)
{
    if (!det) return AGX_ERR_ARG;
    if (const int other = refuse_other_batch(det, BATCH_CLUSTERS)) return other;
    const ClustersPending b = det->clusters;
    const bool to_host = b.results == RESULTS_HOST;
    if (to_host && (!clusters || !counts || !status)) return fail(det, AGX_ERR_ARG, "null output");  // (the batch stays in flight)
    HIP_TRY(det, hipSetDevice(det->device));
    det->batch = BATCH_NONE;  // resolved by this call, whatever it returns
    if (to_host) {
        const size_t F = (size_t)b.n_frames;
        HIP_TRY(det, hipMemcpyAsync(counts, det->side[SB_CLUSTERS_COUNTS].payload, F * 4, hipMemcpyDeviceToHost, det->stream));
        HIP_TRY(det, hipMemcpyAsync(status, det->side[SB_CLUSTERS_STATUS].payload, F * 4, hipMemcpyDeviceToHost, det->stream));
        HIP_TRY(det, hipStreamSynchronize(det->stream));
        // only the rows the batch wrote reach the caller's arrays; the points come from where this batch wrote them (the
        // caller's d_points or SB_CLUSTERS_POINTS: the slot may not exist, or be an earlier batch's, when d_points was given)
        const agx_cluster_info *d_rows = det->side[SB_CLUSTERS_ROWS].ptr<agx_cluster_info>();
        const agx_point *d_pts = points ? b.d_points : nullptr;
        for (size_t f = 0; f < F; ++f) {
            const size_t n = (status[f] & 0xffu) == AGX_CLUSTERS_OK ? std::min(counts[f], b.clusters_per_frame) : 0u, s0 = f * b.clusters_per_frame;
            if (!n) continue;
            HIP_TRY(det, hipMemcpyAsync(clusters + s0, d_rows + s0, n * sizeof(agx_cluster_info), hipMemcpyDeviceToHost, det->stream));
            if (d_pts) HIP_TRY(det, hipMemcpyAsync(static_cast<agx_point *>(points) + s0, d_pts + s0, n * sizeof(agx_point), hipMemcpyDeviceToHost, det->stream));
        }
    }
    HIP_TRY(det, hipStreamSynchronize(det->stream));
    harvest_events(det);
    return AGX_OK;
}

extern "C" {

int agx_clusters_enqueue(agx_detector *det, const float *d_response, int n_frames, int width, int height, size_t row_stride_bytes,
                         size_t frame_stride_bytes, uint32_t clusters_per_frame, agx_cluster_info *d_clusters, void *d_points,
                         uint32_t *d_counts, uint32_t *d_status)
{
    return agx_guard(det, [&]() -> int {
    return clusters_enqueue_impl(det, d_response, n_frames, width, height, row_stride_bytes, frame_stride_bytes, clusters_per_frame,
                                 d_clusters, d_points, d_counts, d_status);
    });
}

int agx_clusters_fetch(agx_detector *det, agx_cluster_info *clusters, void *points, uint32_t *counts, uint32_t *status)
{
    return agx_guard(det, [&]() -> int { return clusters_fetch_impl(det, clusters, points, counts, status); });
}

int agx_cluster_centers(agx_detector *det, const float *response, int width, int height, size_t row_stride_bytes, agx_cluster_info *out,
                        uint32_t cap, uint32_t *n_out, uint32_t *status)
{
    return agx_guard(det, [&]() -> int {
    if (!det) return AGX_ERR_ARG;
    if (!response || !out || !n_out || !status) return fail(det, AGX_ERR_ARG, "null argument");
    // the batch's own rules on the host plane, before the upload: whatever they refuse has waited for and uploaded nothing
    if (const int rc = clusters_check_args(det, response, 1, width, height, row_stride_bytes, row_stride_bytes * (size_t)std::max(height, 0), cap,
                                           nullptr, nullptr, nullptr, nullptr))
        return rc;
    HIP_TRY(det, hipSetDevice(det->device));
    const size_t pitch = (size_t)width * 4;
    float *d_plane = static_cast<float *>(side_ensure(det, SB_CLUSTERS_PLANE, pitch * (size_t)height, 0));
    if (!d_plane) return fail(det, AGX_ERR_HIP, "hipMalloc: response plane");
    HIP_TRY(det, hipMemcpy2DAsync(d_plane, pitch, response, row_stride_bytes, pitch, (size_t)height, hipMemcpyHostToDevice, det->stream));
    const int rc = clusters_enqueue_impl(det, d_plane, 1, width, height, pitch, pitch * (size_t)height, cap, nullptr, nullptr, nullptr, nullptr);
    if (rc) return rc;
    return clusters_fetch_impl(det, out, nullptr, n_out, status);
    });
}

int agx_filter_saddles_enqueue(agx_detector *det, const agx_saddle *d_records, uint32_t *d_status, int n_frames, uint32_t points_per_frame,
                               const uint32_t *d_counts)
{
    return agx_guard(det, [&]() -> int {
    if (!det) return AGX_ERR_ARG;
    if (!d_records || !d_status || n_frames <= 0) return fail(det, AGX_ERR_ARG, "null records, null status or n_frames <= 0");
    if (!points_per_frame) return fail(det, AGX_ERR_ARG, "points_per_frame must be > 0");
    if (((uintptr_t)d_records | (uintptr_t)d_status | (uintptr_t)d_counts) & 3) return fail(det, AGX_ERR_ARG, "records, status and counts must be 4-byte aligned");
    if ((size_t)n_frames * points_per_frame >= ((size_t)1 << 31)) return fail(det, AGX_ERR_ARG, "at most 2^31 - 1 slots per batch");
    HIP_TRY(det, hipSetDevice(det->device));
    begin_batch(det);  // and there is nothing of this one to be fetched
    const FilterSaddlesArgs f{reinterpret_cast<const float *>(d_records), d_status, d_counts, points_per_frame,
                              det->params.min_saddle_angle, det->params.max_saddle_angle, (uint32_t)AGX_POINT_FILTERED};
    hipError_t e = (hipError_t)launch_filter_saddles(f, n_frames, det->stream);
    if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_filter_saddles: ") + hipGetErrorString(e));
    return AGX_OK;
    });
}

int agx_filter_saddles_tail(const agx_params *params, const agx_saddle *records, uint32_t *status, uint32_t n)
{
    return agx_guard(nullptr, [&]() -> int {
    if (n && (!records || !status)) return AGX_ERR_ARG;
    agx_params prm;
    if (params) prm = *params;
    else agx_default_params(&prm);
    filter_saddles(prm, records, status, n);
    return AGX_OK;
    });
}

// One round of detect's loop behind its board search and decode (src/detector.rs:510-539): k_collect_tags, one wave per frame
int agx_collect_tags_enqueue(agx_detector *det, int n_frames, uint32_t quads_per_frame, const uint32_t *d_quads, const uint32_t *d_n_quads,
                             const uint32_t *d_board_status, const agx_tag *d_quad_tags, const uint32_t *d_quad_status,
                             uint32_t saddles_per_frame, const void *d_frame_table, uint32_t *d_point_status, uint32_t tags_per_frame,
                             agx_tag *d_tags, uint32_t *d_n_tags, uint32_t *d_tag_status, int reset)
{
    return agx_guard(det, [&]() -> int {
    if (!det) return AGX_ERR_ARG;
    if (!d_quads || !d_n_quads || !d_board_status || !d_quad_tags || !d_quad_status || !d_tags || !d_n_tags || !d_tag_status || n_frames <= 0)
        return fail(det, AGX_ERR_ARG, "a null array or n_frames <= 0");
    if (!quads_per_frame || !tags_per_frame) return fail(det, AGX_ERR_ARG, "quads_per_frame and tags_per_frame must be > 0");
    if (!d_frame_table && !saddles_per_frame) return fail(det, AGX_ERR_ARG, "saddles_per_frame must be > 0 without a frame table");
    if (((uintptr_t)d_quads | (uintptr_t)d_n_quads | (uintptr_t)d_board_status | (uintptr_t)d_quad_tags | (uintptr_t)d_quad_status |
         (uintptr_t)d_frame_table | (uintptr_t)d_point_status | (uintptr_t)d_tags | (uintptr_t)d_n_tags | (uintptr_t)d_tag_status) & 3)
        return fail(det, AGX_ERR_ARG, "every array must be 4-byte aligned");
    const size_t lim = (size_t)1 << 31, F = (size_t)n_frames;
    if (F * quads_per_frame >= lim || F * tags_per_frame >= lim || (!d_frame_table && F * saddles_per_frame >= lim))
        return fail(det, AGX_ERR_ARG, "at most 2^31 - 1 quad rows, tag rows and slots per batch");
    HIP_TRY(det, hipSetDevice(det->device));
    begin_batch(det);  // and there is nothing of this one to be fetched
    CollectTagsArgs c{};
    c.n_frames = n_frames;
    c.quads_per_frame = quads_per_frame;
    c.quads = d_quads;
    c.n_quads = d_n_quads;
    c.board_status = d_board_status;
    c.quad_tags = d_quad_tags;
    c.quad_status = d_quad_status;
    c.saddles_per_frame = saddles_per_frame;
    c.frame_table = static_cast<const uint32_t *>(d_frame_table);
    c.point_status = d_point_status;
    c.tags_per_frame = tags_per_frame;
    c.tags = d_tags;
    c.n_tags = d_n_tags;
    c.tag_status = d_tag_status;
    c.n_codes = det->fam.n_codes;
    c.reset = reset != 0;
    hipError_t e = (hipError_t)launch_collect_tags(c, det->stream);
    if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_collect_tags: ") + hipGetErrorString(e));
    return AGX_OK;
    });
}

int agx_collect_tags_tail(int family, uint32_t n_quads, const uint32_t *quads, uint32_t board_status, const agx_tag *quad_tags,
                          const uint32_t *quad_status, uint32_t n_slots, uint32_t *point_status, uint32_t tag_cap, agx_tag *tags,
                          uint32_t *n_tags, uint32_t *tag_status)
{
    return agx_guard(nullptr, [&]() -> int {
    FamilyInfo fam;
    if (!family_info(family, fam)) return AGX_ERR_FAMILY;
    if (!n_tags || !tag_status || !tags || !tag_cap) return AGX_ERR_ARG;
    if (board_status == AGX_BOARD_FOUND && n_quads && (!quads || !quad_tags || !quad_status)) return AGX_ERR_ARG;
    collect_tags(fam.n_codes, n_quads, quads, board_status, quad_tags, quad_status, n_slots, point_status, tag_cap, tags, n_tags, tag_status);  // src/detector.rs:510-539
    return AGX_OK;
    });
}

// ---- the board's homography from the tag table (board_fit.hip: k_board_fit; host_tail.cpp: board_fit) ---------------------------
// Every form builds the kernel's record from its C arguments, which come in the record's order, and board_fit_args_bad checks it:
// the enqueue's with device pointers, the tail's for its one frame, whose n_tags and tag_status are words of the call.
int agx_board_fit_enqueue(agx_detector *det, int n_frames, const agx_tag *d_tags, uint32_t tags_per_frame, const uint32_t *d_n_tags,
                          const uint32_t *d_tag_status, uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, int img_w,
                          int img_h, float max_err_sq, uint32_t max_drop, uint32_t min_tags, int flags, double *d_h, float *d_err_sq,
                          uint32_t *d_row_status, uint32_t *d_n_inliers, float *d_rms, agx_tag *d_pred, uint32_t *d_n_pred, uint32_t *d_status)
{
    return agx_guard(det, [&]() -> int {
    if (!det) return AGX_ERR_ARG;
    const BoardFitArgs b{n_frames, d_tags, tags_per_frame, d_n_tags, d_tag_status, cols, rows, first_id, spacing_ratio, img_w, img_h, max_err_sq,
                         max_drop, min_tags, flags, d_h, d_err_sq, d_row_status, d_n_inliers, d_rms, d_pred, d_n_pred, d_status};
    if (const char *why = board_fit_args_bad(b, true)) return fail(det, AGX_ERR_ARG, why);
    HIP_TRY(det, hipSetDevice(det->device));
    begin_batch(det);  // and there is nothing of this one to be fetched
    const hipError_t e = (hipError_t)launch_board_fit(b, det->stream);
    if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_board_fit: ") + hipGetErrorString(e));
    return AGX_OK;
    });
}

int agx_board_fit_tail(const agx_tag *tags, uint32_t tags_per_frame, uint32_t n_tags, uint32_t tag_status, uint32_t cols, uint32_t rows,
                       uint32_t first_id, float spacing_ratio, int img_w, int img_h, float max_err_sq, uint32_t max_drop, uint32_t min_tags,
                       int flags, double *h, float *err_sq, uint32_t *row_status, uint32_t *n_inliers, float *rms, agx_tag *pred,
                       uint32_t *n_pred, uint32_t *status)
{
    return agx_guard(nullptr, [&]() -> int {
    const BoardFitArgs b{1, tags, tags_per_frame, &n_tags, &tag_status, cols, rows, first_id, spacing_ratio, img_w, img_h, max_err_sq,
                         max_drop, min_tags, flags, h, err_sq, row_status, n_inliers, rms, pred, n_pred, status};
    if (board_fit_args_bad(b, false)) return AGX_ERR_ARG;
    *status = board_fit(b);
    return AGX_OK;
    });
}

// ---- the board's pose under a lens model (board_pose.hip: k_board_pose; host_tail.cpp: board_pose) ------------------------------
static_assert(sizeof(agx_camera) == 9 * sizeof(double), "agx_camera is nine doubles: the calls take it as const double *");
// the record likewise; camera is not null
static BoardPoseArgs board_pose_record(int n_frames, const agx_tag *tags, uint32_t tags_per_frame, const uint32_t *n_tags, const uint32_t *tag_status,
                                       uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, double tag_size, const double *camera,
                                       float max_err_sq, uint32_t max_drop, uint32_t min_tags, uint32_t iterations, int flags, double *pose,
                                       float *err_sq, uint32_t *row_status, uint32_t *n_inliers, float *rms, uint32_t *best_iter, agx_tag *pred,
                                       uint32_t *n_pred, uint32_t *status)
{
    agx_camera cam;
    std::memcpy(&cam, camera, sizeof cam);
    return BoardPoseArgs{n_frames, tags, tags_per_frame, n_tags, tag_status, cols, rows, first_id, spacing_ratio, tag_size, cam, max_err_sq, max_drop,
                         min_tags, iterations, flags, pose, err_sq, row_status, n_inliers, rms, best_iter, pred, n_pred, status};
}

int agx_board_pose_enqueue(agx_detector *det, int n_frames, const agx_tag *d_tags, uint32_t tags_per_frame, const uint32_t *d_n_tags,
                           const uint32_t *d_tag_status, uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, double tag_size,
                           const double *camera, float max_err_sq, uint32_t max_drop, uint32_t min_tags, uint32_t iterations, int flags,
                           double *d_pose, float *d_err_sq, uint32_t *d_row_status, uint32_t *d_n_inliers, float *d_rms, uint32_t *d_best_iter,
                           agx_tag *d_pred, uint32_t *d_n_pred, uint32_t *d_status)
{
    return agx_board_pose_enqueue_m(det, n_frames, d_tags, tags_per_frame, d_n_tags, d_tag_status, cols, rows, first_id, spacing_ratio, tag_size,
                                    AGX_LENS_RADTAN, camera, max_err_sq, max_drop, min_tags, iterations, flags, d_pose, d_err_sq, d_row_status,
                                    d_n_inliers, d_rms, d_best_iter, d_pred, d_n_pred, d_status);
}

int agx_board_pose_enqueue_m(agx_detector *det, int n_frames, const agx_tag *d_tags, uint32_t tags_per_frame, const uint32_t *d_n_tags,
                             const uint32_t *d_tag_status, uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, double tag_size,
                             int lens_model, const double *camera, float max_err_sq, uint32_t max_drop, uint32_t min_tags, uint32_t iterations,
                             int flags, double *d_pose, float *d_err_sq, uint32_t *d_row_status, uint32_t *d_n_inliers, float *d_rms,
                             uint32_t *d_best_iter, agx_tag *d_pred, uint32_t *d_n_pred, uint32_t *d_status)
{
    return agx_guard(det, [&]() -> int {
    if (!det) return AGX_ERR_ARG;
    if (!camera) return fail(det, AGX_ERR_ARG, "a null camera");
    const BoardPoseArgs b = board_pose_record(n_frames, d_tags, tags_per_frame, d_n_tags, d_tag_status, cols, rows, first_id, spacing_ratio, tag_size,
                                              camera, max_err_sq, max_drop, min_tags, iterations, flags, d_pose, d_err_sq, d_row_status, d_n_inliers,
                                              d_rms, d_best_iter, d_pred, d_n_pred, d_status);
    if (const char *why = board_pose_args_bad(b, lens_model, true)) return fail(det, AGX_ERR_ARG, why);
    HIP_TRY(det, hipSetDevice(det->device));
    begin_batch(det);  // and there is nothing of this one to be fetched
    const hipError_t e = (hipError_t)launch_board_pose(b, lens_model, det->stream);
    if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_board_pose: ") + hipGetErrorString(e));
    return AGX_OK;
    });
}

int agx_board_pose_tail(const agx_tag *tags, uint32_t tags_per_frame, uint32_t n_tags, uint32_t tag_status, uint32_t cols, uint32_t rows,
                        uint32_t first_id, float spacing_ratio, double tag_size, const double *camera, float max_err_sq, uint32_t max_drop,
                        uint32_t min_tags, uint32_t iterations, int flags, double *pose, float *err_sq, uint32_t *row_status, uint32_t *n_inliers,
                        float *rms, uint32_t *best_iter, agx_tag *pred, uint32_t *n_pred, uint32_t *status)
{
    return agx_board_pose_tail_m(tags, tags_per_frame, n_tags, tag_status, cols, rows, first_id, spacing_ratio, tag_size, AGX_LENS_RADTAN, camera,
                                 max_err_sq, max_drop, min_tags, iterations, flags, pose, err_sq, row_status, n_inliers, rms, best_iter, pred, n_pred,
                                 status);
}

int agx_board_pose_tail_m(const agx_tag *tags, uint32_t tags_per_frame, uint32_t n_tags, uint32_t tag_status, uint32_t cols, uint32_t rows,
                          uint32_t first_id, float spacing_ratio, double tag_size, int lens_model, const double *camera, float max_err_sq,
                          uint32_t max_drop, uint32_t min_tags, uint32_t iterations, int flags, double *pose, float *err_sq, uint32_t *row_status,
                          uint32_t *n_inliers, float *rms, uint32_t *best_iter, agx_tag *pred, uint32_t *n_pred, uint32_t *status)
{
    return agx_guard(nullptr, [&]() -> int {
    if (!camera) return AGX_ERR_ARG;
    const BoardPoseArgs b = board_pose_record(1, tags, tags_per_frame, &n_tags, &tag_status, cols, rows, first_id, spacing_ratio, tag_size, camera,
                                              max_err_sq, max_drop, min_tags, iterations, flags, pose, err_sq, row_status, n_inliers, rms, best_iter,
                                              pred, n_pred, status);
    if (board_pose_args_bad(b, lens_model, false)) return AGX_ERR_ARG;
    *status = board_pose(b, lens_model, nullptr);
    return AGX_OK;
    });
}

int agx_debug_board_pose_sums(const agx_tag *tags, uint32_t tags_per_frame, uint32_t n_tags, uint32_t tag_status, uint32_t cols, uint32_t rows,
                              uint32_t first_id, float spacing_ratio, double tag_size, const double *camera, float max_err_sq, uint32_t max_drop,
                              uint32_t min_tags, uint32_t iterations, int flags, uint32_t *status, double *iter_sums)
{
    return agx_debug_board_pose_sums_m(tags, tags_per_frame, n_tags, tag_status, cols, rows, first_id, spacing_ratio, tag_size, AGX_LENS_RADTAN,
                                       camera, max_err_sq, max_drop, min_tags, iterations, flags, status, iter_sums);
}

int agx_debug_board_pose_sums_m(const agx_tag *tags, uint32_t tags_per_frame, uint32_t n_tags, uint32_t tag_status, uint32_t cols, uint32_t rows,
                                uint32_t first_id, float spacing_ratio, double tag_size, int lens_model, const double *camera, float max_err_sq,
                                uint32_t max_drop, uint32_t min_tags, uint32_t iterations, int flags, uint32_t *status, double *iter_sums)
{
    return agx_guard(nullptr, [&]() -> int {
    if (!iter_sums || ((uintptr_t)iter_sums & 7) || !camera) return AGX_ERR_ARG;
    double pose[12];
    uint32_t n_inliers = 0, n_pred = 0, best_iter = 0, word = 0;
    float rms = 0.0f;
    agx_tag none;
    // the tail's outputs are this call's own; its three arrays stand on one element each until the record has passed and gives their sizes
    BoardPoseArgs b = board_pose_record(1, tags, tags_per_frame, &n_tags, &tag_status, cols, rows, first_id, spacing_ratio, tag_size, camera, max_err_sq,
                                        max_drop, min_tags, iterations, flags, pose, &rms, &word, &n_inliers, &rms, &best_iter, &none, &n_pred, status);
    if (board_pose_args_bad(b, lens_model, false)) return AGX_ERR_ARG;
    std::vector<float> err_sq(n_tags + 1);
    std::vector<uint32_t> row_status(n_tags + 1);
    std::vector<agx_tag> pred((size_t)cols * rows);
    b.err_sq = err_sq.data();
    b.row_status = row_status.data();
    b.pred = pred.data();
    *status = board_pose(b, lens_model, iter_sums);
    return AGX_OK;
    });
}

int agx_debug_pose_atan(const double *r, uint32_t n, double *out)
{
    return agx_guard(nullptr, [&]() -> int {
    if (n && (!r || !out)) return AGX_ERR_ARG;
    for (uint32_t i = 0; i < n; ++i)
        if (!f64_finite(r[i]) || !(r[i] >= 0.0)) return AGX_ERR_ARG;
    pose_atan_host(r, n, out);
    return AGX_OK;
    });
}

int agx_debug_pose_project(int lens_model, const double *camera, const double *xyz, uint32_t n, double *uv)
{
    return agx_guard(nullptr, [&]() -> int {
    if (!camera || (n && (!xyz || !uv))) return AGX_ERR_ARG;
    agx_camera cam;
    std::memcpy(&cam, camera, sizeof cam);
    if (!pose_args_ok(lens_model, cam, 1.0, 0)) return AGX_ERR_ARG;
    pose_project_host(lens_model, cam, xyz, n, uv);
    return AGX_OK;
    });
}

// ---- the camera from the batch (calibrate.hip: k_calib_blocks, k_calib_solve; calibrate_host.cpp) -------------------------------
static CalibArgs calib_record(int n_frames, const agx_tag *tags, uint32_t tags_per_frame, const uint32_t *n_tags, const uint32_t *tag_status, uint32_t cols,
                              uint32_t rows, uint32_t first_id, float spacing_ratio, double tag_size, const double *camera, uint32_t fixed_mask,
                              double damping, uint32_t iterations, uint32_t min_tags, uint32_t min_frames, int flags, const double *pose_in,
                              const uint32_t *row_status, const uint32_t *fit_status, double *camera_out, double *pose, float *frame_cost,
                              uint32_t *frame_n, void *report)
{
    agx_camera cam;
    std::memcpy(&cam, camera, sizeof cam);
    return CalibArgs{n_frames, tags, tags_per_frame, n_tags, tag_status, cols, rows, first_id, spacing_ratio, tag_size, cam, fixed_mask, damping,
                     iterations, min_tags, min_frames, flags, pose_in, row_status, fit_status, camera_out, pose, frame_cost, frame_n,
                     static_cast<agx_calib_report *>(report)};
}

int agx_calibrate_enqueue(agx_detector *det, int n_frames, const agx_tag *d_tags, uint32_t tags_per_frame, const uint32_t *d_n_tags,
                          const uint32_t *d_tag_status, uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, double tag_size,
                          int lens_model, const double *camera, uint32_t fixed_mask, double damping, uint32_t iterations, uint32_t min_tags,
                          uint32_t min_frames, int flags, const double *d_pose_in, const uint32_t *d_row_status, const uint32_t *d_fit_status,
                          double *d_camera, double *d_pose, float *d_frame_cost, uint32_t *d_frame_n, void *d_report)
{
    return agx_guard(det, [&]() -> int {
    if (!det) return AGX_ERR_ARG;
    if (!camera) return fail(det, AGX_ERR_ARG, "a null camera");
    const CalibArgs a = calib_record(n_frames, d_tags, tags_per_frame, d_n_tags, d_tag_status, cols, rows, first_id, spacing_ratio, tag_size, camera,
                                     fixed_mask, damping, iterations, min_tags, min_frames, flags, d_pose_in, d_row_status, d_fit_status, d_camera,
                                     d_pose, d_frame_cost, d_frame_n, d_report);
    if (const char *why = calib_args_bad(a, lens_model)) return fail(det, AGX_ERR_ARG, why);
    HIP_TRY(det, hipSetDevice(det->device));
    begin_batch(det);  // and there is nothing of this one to be fetched
    void *work = side_ensure(det, SB_CALIB_WORK, calib_work_bytes(n_frames), 0);
    if (!work) return fail(det, AGX_ERR_NOMEM, "the calibration's workspace");
    const hipError_t e = (hipError_t)launch_calibrate(a, lens_model, work, det->stream);
    if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_calib_blocks / k_calib_solve: ") + hipGetErrorString(e));
    return AGX_OK;
    });
}

int agx_calibrate_tail(int n_frames, const agx_tag *tags, uint32_t tags_per_frame, const uint32_t *n_tags, const uint32_t *tag_status, uint32_t cols,
                       uint32_t rows, uint32_t first_id, float spacing_ratio, double tag_size, int lens_model, const double *camera,
                       uint32_t fixed_mask, double damping, uint32_t iterations, uint32_t min_tags, uint32_t min_frames, int flags,
                       const double *pose_in, const uint32_t *row_status, const uint32_t *fit_status, double *camera_out, double *pose,
                       float *frame_cost, uint32_t *frame_n, void *report)
{
    return agx_guard(nullptr, [&]() -> int {
    if (!camera) return AGX_ERR_ARG;
    const CalibArgs a = calib_record(n_frames, tags, tags_per_frame, n_tags, tag_status, cols, rows, first_id, spacing_ratio, tag_size, camera, fixed_mask,
                                     damping, iterations, min_tags, min_frames, flags, pose_in, row_status, fit_status, camera_out, pose, frame_cost,
                                     frame_n, report);
    if (calib_args_bad(a, lens_model)) return AGX_ERR_ARG;
    calibrate_host(a, lens_model);
    return AGX_OK;
    });
}

int agx_calibrate_seed_tail(const double *h, const uint32_t *fit_status, uint32_t n, int img_w, int img_h, double *camera_out, uint32_t *status)
{
    return agx_guard(nullptr, [&]() -> int {
    if (!h || !fit_status || !camera_out || !status || !n || img_w < 1 || img_h < 1) return AGX_ERR_ARG;
    *status = calibrate_seed_host(h, fit_status, n, img_w, img_h, camera_out);
    return AGX_OK;
    });
}

int agx_debug_calib_param_jacobian(int lens_model, const double *camera, const double *xyz, uint32_t n, double *out)
{
    return agx_guard(nullptr, [&]() -> int {
    if (!camera || (n && (!xyz || !out))) return AGX_ERR_ARG;
    agx_camera cam;
    std::memcpy(&cam, camera, sizeof cam);
    if (!pose_args_ok(lens_model, cam, 1.0, 0)) return AGX_ERR_ARG;
    calib_param_jacobian_host(lens_model, cam, xyz, n, out);
    return AGX_OK;
    });
}

// ---- the rig from the batch (rig.hip: k_rig_blocks, k_rig_instants, k_rig_solve; rig_host.cpp) ---------------------------------
static bool rig_record(RigArgs &a, int n_cams, int n_instants, const agx_tag *tags, uint32_t tags_per_frame, const uint32_t *n_tags, const uint32_t *tag_status,
                       uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, double tag_size, const int *lens_models, const double *cameras,
                       double damping, uint32_t iterations, uint32_t min_tags, uint32_t min_cams, uint32_t min_instants, int flags, const double *pose_in,
                       const uint32_t *row_status, const uint32_t *fit_status, const double *extrinsics_in, double *extrinsics, double *rig_pose,
                       float *frame_cost, uint32_t *frame_n, uint32_t *cam_n, void *report)
{
    if (!lens_models || !cameras || n_cams < RIG_MIN_CAMS || n_cams > RIG_MAX_CAMS) return false;
    a = RigArgs{};
    a.n_cams = n_cams, a.n_instants = n_instants;
    a.tags = tags, a.tags_per_frame = tags_per_frame, a.n_tags = n_tags, a.tag_status = tag_status;
    a.cols = cols, a.rows = rows, a.first_id = first_id, a.spacing_ratio = spacing_ratio, a.tag_size = tag_size;
    for (int c = 0; c < n_cams; ++c) {
        a.lens[c] = lens_models[c];
        std::memcpy(&a.camera[c], cameras + 9 * c, sizeof(agx_camera));
    }
    a.damping = damping, a.iterations = iterations, a.min_tags = min_tags, a.min_cams = min_cams, a.min_instants = min_instants, a.flags = flags;
    a.pose_in = pose_in, a.row_status = row_status, a.fit_status = fit_status, a.ext_in = extrinsics_in, a.ext = extrinsics, a.rig_pose = rig_pose;
    a.frame_cost = frame_cost, a.frame_n = frame_n, a.cam_n = cam_n, a.report = static_cast<agx_rig_report *>(report);
    return true;
}

int agx_rig_calibrate_enqueue(agx_detector *det, int n_cams, int n_instants, const agx_tag *d_tags, uint32_t tags_per_frame, const uint32_t *d_n_tags,
                              const uint32_t *d_tag_status, uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, double tag_size,
                              const int *lens_models, const double *cameras, double damping, uint32_t iterations, uint32_t min_tags, uint32_t min_cams,
                              uint32_t min_instants, int flags, const double *d_pose_in, const uint32_t *d_row_status, const uint32_t *d_fit_status,
                              const double *d_extrinsics_in, double *d_extrinsics, double *d_rig_pose, float *d_frame_cost, uint32_t *d_frame_n,
                              uint32_t *d_cam_n, void *d_report)
{
    return agx_guard(det, [&]() -> int {
    if (!det) return AGX_ERR_ARG;
    RigArgs a;
    if (!rig_record(a, n_cams, n_instants, d_tags, tags_per_frame, d_n_tags, d_tag_status, cols, rows, first_id, spacing_ratio, tag_size, lens_models, cameras,
                    damping, iterations, min_tags, min_cams, min_instants, flags, d_pose_in, d_row_status, d_fit_status, d_extrinsics_in, d_extrinsics,
                    d_rig_pose, d_frame_cost, d_frame_n, d_cam_n, d_report))
        return fail(det, AGX_ERR_ARG, "n_cams in 2 .. 8, lens_models and cameras not null");
    if (const char *why = rig_args_bad(a, false)) return fail(det, AGX_ERR_ARG, why);
    HIP_TRY(det, hipSetDevice(det->device));
    begin_batch(det);  // and there is nothing of this one to be fetched
    void *work = side_ensure(det, SB_RIG_WORK, rig_work_bytes(n_cams, n_instants), 0);
    if (!work) return fail(det, AGX_ERR_NOMEM, "the rig calibration's workspace");
    const hipError_t e = (hipError_t)launch_rig_calibrate(a, work, det->stream);
    if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_rig_blocks / k_rig_instants / k_rig_solve: ") + hipGetErrorString(e));
    return AGX_OK;
    });
}

int agx_rig_calibrate_tail(int n_cams, int n_instants, const agx_tag *tags, uint32_t tags_per_frame, const uint32_t *n_tags, const uint32_t *tag_status,
                           uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, double tag_size, const int *lens_models,
                           const double *cameras, double damping, uint32_t iterations, uint32_t min_tags, uint32_t min_cams, uint32_t min_instants,
                           int flags, const double *pose_in, const uint32_t *row_status, const uint32_t *fit_status, const double *extrinsics_in,
                           double *extrinsics, double *rig_pose, float *frame_cost, uint32_t *frame_n, uint32_t *cam_n, void *report)
{
    return agx_guard(nullptr, [&]() -> int {
    RigArgs a;
    if (!rig_record(a, n_cams, n_instants, tags, tags_per_frame, n_tags, tag_status, cols, rows, first_id, spacing_ratio, tag_size, lens_models, cameras,
                    damping, iterations, min_tags, min_cams, min_instants, flags, pose_in, row_status, fit_status, extrinsics_in, extrinsics, rig_pose,
                    frame_cost, frame_n, cam_n, report))
        return AGX_ERR_ARG;
    if (rig_args_bad(a, true)) return AGX_ERR_ARG;
    rig_calibrate_host(a);
    return AGX_OK;
    });
}

int agx_rig_seed_tail(int n_cams, int n_instants, const double *pose, const uint32_t *fit_status, const uint32_t *frame_n, double *extrinsics_out,
                      uint32_t *cam_status)
{
    return agx_guard(nullptr, [&]() -> int {
    if (!pose || !fit_status || !extrinsics_out || !cam_status || n_cams < RIG_MIN_CAMS || n_cams > RIG_MAX_CAMS || n_instants < 1 ||
        (uint64_t)n_cams * (uint64_t)n_instants > CALIB_MAX_FRAMES)
        return AGX_ERR_ARG;
    rig_seed_host(n_cams, n_instants, pose, fit_status, frame_n, extrinsics_out, cam_status);
    return AGX_OK;
    });
}

int agx_debug_rig_jacobian(int lens_model, const double *camera, const double *extrinsic, const double *rig_pose, const double *XY, uint32_t n, double *out)
{
    return agx_guard(nullptr, [&]() -> int {
    if (!camera || !rig_pose || (n && (!XY || !out))) return AGX_ERR_ARG;
    agx_camera cam;
    std::memcpy(&cam, camera, sizeof cam);
    if (!pose_args_ok(lens_model, cam, 1.0, 0)) return AGX_ERR_ARG;
    rig_jacobian_host(lens_model, cam, extrinsic, rig_pose, XY, n, out);
    return AGX_OK;
    });
}

// ---- rectified batches (rectify.hip: k_rectify_map, k_remap, k_rectified_points and the host forms) -------------------------------
static const char *kRectifyGeomRule =
    AGX_LENS_CAMERA_RULE ", new_camera "
    "finite with fx' and fy' > 0, rotation NULL or finite";

static bool rectify_map_args(int lens_model, const double *camera, const double *new_camera, const double *rotation, int src_width,
                             int src_height, int dst_width, int dst_height, int *map, size_t map_row_stride_bytes, RectifyMapArgs &a,
                             const char **why)
{
    a.lens = lens_model;
    if (!rectify_geom(lens_model, camera, new_camera, rotation, a.g)) return *why = kRectifyGeomRule, false;
    a.src_w = src_width;
    a.src_h = src_height;
    a.dst_w = dst_width;
    a.dst_h = dst_height;
    a.map = map;
    a.map_stride = map_row_stride_bytes;
    return !(*why = rectify_map_args_bad(a));
}

int agx_rectify_map_enqueue(agx_detector *det, int lens_model, const double *camera, const double *new_camera, const double *rotation,
                            int src_width, int src_height, int dst_width, int dst_height, int *d_map, size_t map_row_stride_bytes)
{
    return agx_guard(det, [&]() -> int {
    if (!det) return AGX_ERR_ARG;
    RectifyMapArgs a{};
    const char *why = nullptr;
    if (!rectify_map_args(lens_model, camera, new_camera, rotation, src_width, src_height, dst_width, dst_height, d_map, map_row_stride_bytes, a, &why))
        return fail(det, AGX_ERR_ARG, why);
    HIP_TRY(det, hipSetDevice(det->device));
    begin_batch(det);  // and there is nothing of this one to be fetched
    const hipError_t e = (hipError_t)launch_rectify_map(a, det->stream);
    if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_rectify_map: ") + hipGetErrorString(e));
    return AGX_OK;
    });
}

int agx_rectify_map_tail(int lens_model, const double *camera, const double *new_camera, const double *rotation, int src_width, int src_height,
                         int dst_width, int dst_height, int *map, size_t map_row_stride_bytes)
{
    return agx_guard(nullptr, [&]() -> int {
    RectifyMapArgs a{};
    const char *why = nullptr;
    if (!rectify_map_args(lens_model, camera, new_camera, rotation, src_width, src_height, dst_width, dst_height, map, map_row_stride_bytes, a, &why))
        return AGX_ERR_ARG;
    rectify_map_host(a);
    return AGX_OK;
    });
}

static RemapArgs remap_args(const void *src, int n_frames, int src_width, int src_height, size_t src_row_stride_bytes, size_t src_frame_stride_bytes,
                            int format, const int *map, size_t map_row_stride_bytes, int dst_width, int dst_height, void *dst,
                            size_t dst_row_stride_bytes, size_t dst_frame_stride_bytes, uint32_t border)
{
    RemapArgs a{};
    a.src = src;
    a.n_frames = n_frames;
    a.src_w = src_width;
    a.src_h = src_height;
    a.src_row_stride = src_row_stride_bytes;
    a.src_frame_stride = src_frame_stride_bytes;
    a.format = format;
    a.map = map;
    a.map_stride = map_row_stride_bytes;
    a.dst_w = dst_width;
    a.dst_h = dst_height;
    a.dst = dst;
    a.dst_row_stride = dst_row_stride_bytes;
    a.dst_frame_stride = dst_frame_stride_bytes;
    a.border = border;
    return a;
}

int agx_remap_enqueue(agx_detector *det, const void *d_src, int n_frames, int src_width, int src_height, size_t src_row_stride_bytes,
                      size_t src_frame_stride_bytes, int format, const int *d_map, size_t map_row_stride_bytes, int dst_width, int dst_height,
                      void *d_dst, size_t dst_row_stride_bytes, size_t dst_frame_stride_bytes, uint32_t border)
{
    return agx_guard(det, [&]() -> int {
    if (!det) return AGX_ERR_ARG;
    const RemapArgs a = remap_args(d_src, n_frames, src_width, src_height, src_row_stride_bytes, src_frame_stride_bytes, format, d_map,
                                   map_row_stride_bytes, dst_width, dst_height, d_dst, dst_row_stride_bytes, dst_frame_stride_bytes, border);
    if (const char *why = remap_args_bad(a)) return fail(det, AGX_ERR_ARG, why);
    HIP_TRY(det, hipSetDevice(det->device));
    begin_batch(det);  // and there is nothing of this one to be fetched
    const hipError_t e = (hipError_t)launch_remap(a, det->stream);
    if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_remap: ") + hipGetErrorString(e));
    return AGX_OK;
    });
}

int agx_remap_tail(const void *src, int n_frames, int src_width, int src_height, size_t src_row_stride_bytes, size_t src_frame_stride_bytes,
                   int format, const int *map, size_t map_row_stride_bytes, int dst_width, int dst_height, void *dst, size_t dst_row_stride_bytes,
                   size_t dst_frame_stride_bytes, uint32_t border)
{
    return agx_guard(nullptr, [&]() -> int {
    const RemapArgs a = remap_args(src, n_frames, src_width, src_height, src_row_stride_bytes, src_frame_stride_bytes, format, map,
                                   map_row_stride_bytes, dst_width, dst_height, dst, dst_row_stride_bytes, dst_frame_stride_bytes, border);
    if (remap_args_bad(a)) return AGX_ERR_ARG;
    remap_host(a);
    return AGX_OK;
    });
}

// ---- decimated batches (decimate.hip: k_decimate and the host form) ---------------------------------------------------------------
static DecimateArgs decimate_args(const void *src, int n_frames, int width, int height, size_t row_stride_bytes, size_t frame_stride_bytes,
                                  int format, int factor, void *dst, size_t dst_row_stride_bytes, size_t dst_frame_stride_bytes)
{
    DecimateArgs a{};
    a.src = src;
    a.n_frames = n_frames;
    a.src_w = width;
    a.src_h = height;
    a.src_row_stride = row_stride_bytes;
    a.src_frame_stride = frame_stride_bytes;
    a.format = format;
    a.factor = factor;
    a.dst = dst;
    a.dst_row_stride = dst_row_stride_bytes;
    a.dst_frame_stride = dst_frame_stride_bytes;
    return a;
}

int agx_decimate_enqueue(agx_detector *det, const void *d_src, int n_frames, int width, int height, size_t row_stride_bytes,
                         size_t frame_stride_bytes, int format, int factor, void *d_dst, size_t dst_row_stride_bytes,
                         size_t dst_frame_stride_bytes)
{
    return agx_guard(det, [&]() -> int {
    if (!det) return AGX_ERR_ARG;
    if (format != AGX_L8 && format != AGX_L16) return fail(det, AGX_ERR_FORMAT, "format must be AGX_L8 or AGX_L16");
    const DecimateArgs a = decimate_args(d_src, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format, factor, d_dst,
                                         dst_row_stride_bytes, dst_frame_stride_bytes);
    if (const char *why = decimate_args_bad(a)) return fail(det, AGX_ERR_ARG, why);
    HIP_TRY(det, hipSetDevice(det->device));
    begin_batch(det);  // and there is nothing of this one to be fetched
    const hipError_t e = (hipError_t)launch_decimate(a, det->stream);
    if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_decimate: ") + hipGetErrorString(e));
    return AGX_OK;
    });
}

int agx_decimate_tail(const void *src, int n_frames, int width, int height, size_t row_stride_bytes, size_t frame_stride_bytes, int format,
                      int factor, void *dst, size_t dst_row_stride_bytes, size_t dst_frame_stride_bytes)
{
    return agx_guard(nullptr, [&]() -> int {
    if (format != AGX_L8 && format != AGX_L16) return AGX_ERR_FORMAT;
    const DecimateArgs a = decimate_args(src, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format, factor, dst,
                                         dst_row_stride_bytes, dst_frame_stride_bytes);
    if (decimate_args_bad(a)) return AGX_ERR_ARG;
    decimate_host(a);
    return AGX_OK;
    });
}

static bool rectified_points_args(int lens_model, const double *camera, const double *new_camera, const double *rotation, const void *points,
                                  size_t point_stride_bytes, uint32_t n_points, void *out, size_t out_stride_bytes, RectifiedPointsArgs &a,
                                  const char **why)
{
    a.lens = lens_model;
    if (!rectify_geom(lens_model, camera, new_camera, rotation, a.g)) return *why = kRectifyGeomRule, false;
    a.points = points;
    a.stride = point_stride_bytes;
    a.n = n_points;
    a.out = out;
    a.out_stride = out_stride_bytes;
    return !(*why = rectified_points_args_bad(a));
}

int agx_rectified_points_enqueue(agx_detector *det, int lens_model, const double *camera, const double *new_camera, const double *rotation,
                                 const void *d_points, size_t point_stride_bytes, uint32_t n_points, void *d_out, size_t out_stride_bytes)
{
    return agx_guard(det, [&]() -> int {
    if (!det) return AGX_ERR_ARG;
    RectifiedPointsArgs a{};
    const char *why = nullptr;
    if (!rectified_points_args(lens_model, camera, new_camera, rotation, d_points, point_stride_bytes, n_points, d_out, out_stride_bytes, a, &why))
        return fail(det, AGX_ERR_ARG, why);
    HIP_TRY(det, hipSetDevice(det->device));
    begin_batch(det);  // and there is nothing of this one to be fetched
    const hipError_t e = (hipError_t)launch_rectified_points(a, det->stream);
    if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_rectified_points: ") + hipGetErrorString(e));
    return AGX_OK;
    });
}

int agx_rectified_points_tail(int lens_model, const double *camera, const double *new_camera, const double *rotation, const void *points,
                              size_t point_stride_bytes, uint32_t n_points, void *out, size_t out_stride_bytes)
{
    return agx_guard(nullptr, [&]() -> int {
    RectifiedPointsArgs a{};
    const char *why = nullptr;
    if (!rectified_points_args(lens_model, camera, new_camera, rotation, points, point_stride_bytes, n_points, out, out_stride_bytes, a, &why))
        return AGX_ERR_ARG;
    rectified_points_host(a);
    return AGX_OK;
    });
}

// ---- the board through pose and lens model (render.hip: k_render_boards and the host form) -----------------------------------------
static_assert(sizeof(agx_render_params) == 24, "agx_render_params is six 32-bit fields: the calls take it as const void *");
// the kernel's record from the C arguments; AGX_OK, or the status with *why the text of an AGX_ERR_ARG
static int render_record(int n_frames, int width, int height, size_t row_stride_bytes, size_t frame_stride_bytes, int format, int family,
                         uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, double tag_size, int lens_model, const double *camera,
                         const double *poses, const void *params, void *frames, agx_tag *truth, uint32_t *n_truth, uint32_t *status, bool device,
                         RenderArgs &a, const char **why)
{
    if (!camera || !params) return *why = "a null camera or params", AGX_ERR_ARG;
    agx_camera cam;
    agx_render_params p;
    std::memcpy(&cam, camera, sizeof cam);
    std::memcpy(&p, params, sizeof p);
    int edge = 0, border = 0;
    uint32_t n_codes = 0;
    if (!render_family(family, edge, border, n_codes)) return *why = "an unknown family", AGX_ERR_FAMILY;
    a.lens = lens_model;
    a.n_frames = n_frames;
    a.width = width;
    a.height = height;
    a.row_stride = row_stride_bytes;
    a.frame_stride = frame_stride_bytes;
    a.format = format;
    a.family = family;
    a.poses = poses;
    a.frames = frames;
    a.truth = truth;
    a.n_truth = n_truth;
    a.status = status;
    // (the geometry of a layout that is refused is not used: cols = 0 must not divide)
    a.g = render_geom(lens_model, cam, cols, (uint64_t)cols * rows <= FIT_MAX_BOARD ? rows : 0, first_id, spacing_ratio, tag_size, edge, border, p);
    return (*why = render_args_bad(a, cam, p, device)) ? AGX_ERR_ARG : AGX_OK;
}

int agx_render_boards_enqueue(agx_detector *det, int n_frames, int width, int height, size_t row_stride_bytes, size_t frame_stride_bytes,
                              int format, int family, uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, double tag_size,
                              int lens_model, const double *camera, const double *d_poses, const void *params, void *d_frames, agx_tag *d_truth,
                              uint32_t *d_n_truth, uint32_t *d_status)
{
    return agx_guard(det, [&]() -> int {
    if (!det) return AGX_ERR_ARG;
    RenderArgs a{};
    const char *why = nullptr;
    if (const int st = render_record(n_frames, width, height, row_stride_bytes, frame_stride_bytes, format, family, cols, rows, first_id, spacing_ratio,
                                     tag_size, lens_model, camera, d_poses, params, d_frames, d_truth, d_n_truth, d_status, true, a, &why))
        return fail(det, st, why);
    HIP_TRY(det, hipSetDevice(det->device));
    begin_batch(det);  // and there is nothing of this one to be fetched
    const hipError_t e = (hipError_t)launch_render_boards(a, det->stream);
    if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_render_boards: ") + hipGetErrorString(e));
    return AGX_OK;
    });
}

int agx_render_boards_tail(int width, int height, size_t row_stride_bytes, int format, int family, uint32_t cols, uint32_t rows, uint32_t first_id,
                           float spacing_ratio, double tag_size, int lens_model, const double *camera, const double *pose, const void *params,
                           void *frame, agx_tag *truth, uint32_t *n_truth, uint32_t *status)
{
    return agx_guard(nullptr, [&]() -> int {
    RenderArgs a{};
    const char *why = nullptr;
    if (const int st = render_record(1, width, height, row_stride_bytes, row_stride_bytes * (size_t)(height > 0 ? height : 0), format, family, cols, rows,
                                     first_id, spacing_ratio, tag_size, lens_model, camera, pose, params, frame, truth, n_truth, status, false, a, &why))
        return st;
    render_boards_host(a);
    return AGX_OK;
    });
}

}  // extern "C"

int agx::group_detect_enqueue(agx_detector *det, const void *d_frames, int n_frames, int width, int height, size_t row_stride_bytes,
                              size_t frame_stride_bytes, int format, uint32_t cap_per_frame, uint32_t *d_table, agx_tag *d_slab,
                              uint32_t slab_records)
{
    return agx_guard(det, [&]() -> int {
    return detect_enqueue_checked(det, d_frames, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format, cap_per_frame,
                                  RESULTS_GROUP, d_slab, d_table, nullptr, slab_records);
    });
}

int agx::group_detect_fetch(agx_detector *det, const char *back, agx_tag *out, uint32_t *counts, int *frame_status, int n_threads)
{
    return agx_guard(det, [&]() -> int {
    det->last_error.clear();
    const int rc = group_detect_fetch_impl(det, back, out, counts, frame_status, n_threads);
    if (rc == AGX_ERR_NOMEM) det->last_error = "out of host memory or threads";
    else if (rc == AGX_ERR_STATE) det->last_error = "the group's batch is no longer the one in flight on this detector";
    else if (rc != AGX_OK && det->last_error.empty()) det->last_error = agx_status_string(rc);
    return rc;
    });
}

int agx::fetch_compact(agx_detector *det, const agx_saddle **records, uint32_t *counts, uint32_t *offsets, int *status)
{
    const int n = chain_in_flight(det) ? det->args.n_frames : 0;
    // cap 0: counts and status only (a frame with any saddles reads "capacity" against cap 0: the real status is
    // derived from the counters below, with no limit on the list's length)
    int rc = saddles_fetch_impl(det, nullptr, 0, counts, status);
    if (rc != AGX_OK && rc != AGX_ERR_CAPACITY) return rc;
    for (int f = 0; f < n; ++f) {
        const FrameCounters &c = det->h_ctr[f];
        status[f] = frame_status_of(c, 0xffffffffu);
        counts[f] = status[f] == AGX_OK ? c.n_out : 0;
        offsets[f] = c.out_offset;
    }
    *records = reinterpret_cast<const agx_saddle *>(det->h_out);
    det->last_error.clear();
    return AGX_OK;
}

void agx::abandon_batch(agx_detector *det)
{
    (void)hipStreamSynchronize(det->stream);
    harvest_events(det);
    det->batch = BATCH_NONE;
}

namespace {
// The single frame of the last agx_refined_saddle_points call again, into a larger buffer (its
// list is still in the pinned host mirror).
int refetch_single(agx_detector *det, agx_saddle *out, uint32_t cap, uint32_t *n_out)
{
    const FrameCounters &c = det->h_ctr[0];
    *n_out = c.n_out;
    if (c.n_out > cap) return AGX_ERR_CAPACITY;
    if (c.n_out) std::memcpy(out, det->h_out + (size_t)c.out_offset * 5, (size_t)c.n_out * sizeof(agx_saddle));
    det->last_error.clear();
    return AGX_OK;
}

// agx_refined_saddle_points; with want_luma8 (L16 / RGB8 only) the u8 luma of the frame is computed on the
// device behind the chain and is in SB_LUMA_H (tight [H][W]) when this returns.
int refined_saddle_points_impl(agx_detector *det, const void *pixels, int width, int height, size_t row_stride_bytes,
                               int format, agx_saddle *out, uint32_t cap, uint32_t *n_out, bool want_luma8)
{
    if (!det || !n_out) return fail(det, AGX_ERR_ARG, "null argument");
    FrameBatch b;
    int rc = stage_host_frame(det, pixels, width, height, row_stride_bytes, format, /*min_side*/ 2, /*lf32*/ true, /*upload*/ true, b);
    if (rc) return rc;
    const void *d_stage = b.frames;
    const size_t pitch = b.row_stride, need = b.frame_stride;
    rc = agx_saddles_batch_enqueue(det, d_stage, 1, width, height, pitch, need, format);
    if (rc) return rc;
    if (want_luma8) {  // stream-ordered behind the chain; the fetch below waits for the stream
        const size_t lb = (size_t)width * (size_t)height;
        if (!side_ensure_pair(det, SB_LUMA_D, lb, 0, SB_LUMA_H, lb, 1)) return fail(det, AGX_ERR_HIP, "hipMalloc / hipHostMalloc: luma planes");
        uint8_t *d_luma = det->side[SB_LUMA_D].ptr<uint8_t>();
        hipError_t e = (hipError_t)launch_luma8(d_stage, pitch, need, 1, format, d_luma, width, height, det->stream);
        if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_luma8: ") + hipGetErrorString(e));
        HIP_TRY(det, hipMemcpyAsync(det->side[SB_LUMA_H].payload, d_luma, lb, hipMemcpyDeviceToHost, det->stream));
    }
    // one frame: the pinned host mirror of the batch fetch holds the list; a too-small `cap` reports
    // the needed size
    uint32_t count = 0;
    int st = AGX_OK;
    rc = agx_saddles_batch_fetch(det, nullptr, 0, &count, &st);  // cap 0: counts and status only
    if (rc && rc != AGX_ERR_CAPACITY) return rc;
    if (frame_status_of(det->h_ctr[0], 0xffffffffu) != AGX_OK) return AGX_ERR_CAPACITY;  // a list overflowed: last_error set by fetch
    rc = refetch_single(det, out, cap, n_out);
    return rc == AGX_ERR_CAPACITY ? fail(det, rc, "output capacity too small") : rc;
}
}  // namespace

extern "C" {

int agx_refined_saddle_points(agx_detector *det, const void *pixels, int width, int height, size_t row_stride_bytes,
                              int format, agx_saddle *out, uint32_t cap, uint32_t *n_out)
{
    return agx_guard(det, [&]() -> int {
    return refined_saddle_points_impl(det, pixels, width, height, row_stride_bytes, format, out, cap, n_out, false);
    });
}

int agx_debug_angle_pairs(const float *vectors, size_t n, float *exact, float *approx, uint8_t *has_approx)
{
    return agx_guard(nullptr, [&]() -> int {
    if (!vectors || !exact || !approx || !has_approx) return AGX_ERR_ARG;
    debug_angle_pairs(vectors, n, exact, approx, has_approx);
    return AGX_OK;
    });
}

int agx_debug_angle_pairs_coarse(const float *vectors, size_t n, float *coarse, uint8_t *has_coarse)
{
    return agx_guard(nullptr, [&]() -> int {
    if (!vectors || !coarse || !has_coarse) return AGX_ERR_ARG;
    debug_angle_pairs(vectors, n, nullptr, nullptr, nullptr, coarse, has_coarse);
    return AGX_OK;
    });
}

int agx_debug_white_block_angles(const float *triples, size_t n, float *reference, double *binary64)
{
    return agx_guard(nullptr, [&]() -> int {
    if (!triples || !reference || !binary64) return AGX_ERR_ARG;
    debug_white_block_angles(triples, n, reference, binary64);
    return AGX_OK;
    });
}

int agx_debug_libm_atan2f_check(uint64_t n, uint64_t seed, uint64_t *mismatches)
{
    return agx_guard(nullptr, [&]() -> int {
    if (!mismatches) return AGX_ERR_ARG;
    *mismatches = libm_atan2f_mismatches(n, seed);
    return AGX_OK;
    });
}

int agx_luma8(const void *pixels, int width, int height, size_t row_stride_bytes, int format, uint8_t *out)
{
    return agx_guard(nullptr, [&]() -> int {
    if (!pixels || !out || width <= 0 || height <= 0) return AGX_ERR_ARG;
    return luma8(pixels, width, height, row_stride_bytes, format, out);
    });
}

int agx_detect_from_saddles(const agx_detector *det, const agx_saddle *saddles, uint32_t n_saddles,
                            const uint8_t *luma, int width, int height, size_t row_stride_bytes, agx_tag *out,
                            uint32_t cap, uint32_t *n_out)
{
    return agx_guard(det, [&]() -> int {
    if (!det || !luma || !n_out || (!saddles && n_saddles) || (!out && cap)) return AGX_ERR_ARG;
    std::vector<agx_saddle> refined(saddles, saddles + n_saddles);
    std::vector<agx_tag> tags;
    detect_tail(det->fam, det->params.max_num_of_boards, std::move(refined), luma, width, height, row_stride_bytes,
                tags, det->tail_workers);
    *n_out = (uint32_t)tags.size();
    if (tags.size() > cap) return AGX_ERR_CAPACITY;
    if (!tags.empty()) std::memcpy(out, tags.data(), tags.size() * sizeof(agx_tag));
    return AGX_OK;
    });
}

int agx_detect_tail(int family, const agx_params *params, const agx_saddle *saddles, uint32_t n_saddles,
                    const uint8_t *luma, int width, int height, size_t row_stride_bytes, agx_tag *out, uint32_t cap,
                    uint32_t *n_out)
{
    return agx_guard(nullptr, [&]() -> int {
    return agx_detect_tail_threads(family, params, saddles, n_saddles, luma, width, height, row_stride_bytes, out, cap,
                                   n_out, 1);
    });
}

int agx_detect_tail_threads(int family, const agx_params *params, const agx_saddle *saddles, uint32_t n_saddles,
                            const uint8_t *luma, int width, int height, size_t row_stride_bytes, agx_tag *out,
                            uint32_t cap, uint32_t *n_out, int n_threads)
{
    return agx_guard(nullptr, [&]() -> int {
    if (!luma || !n_out || (!saddles && n_saddles) || (!out && cap) || width < 1 || height < 1) return AGX_ERR_ARG;
    FamilyInfo fam;
    if (!family_info(family, fam)) return AGX_ERR_FAMILY;
    agx_params prm;
    if (params) prm = *params;
    else agx_default_params(&prm);
    std::vector<agx_saddle> refined(saddles, saddles + n_saddles);
    std::vector<agx_tag> tags;
    struct Del {
        void operator()(TailWorkers *w) const { destroy_tail_workers(w); }
    };
    std::unique_ptr<TailWorkers, Del> workers(create_tail_workers(n_threads));  // threads of this call only (nullptr for <= 1)
    detect_tail(fam, prm.max_num_of_boards, std::move(refined), luma, width, height, row_stride_bytes, tags, workers.get());
    *n_out = (uint32_t)tags.size();
    if (tags.size() > cap) return AGX_ERR_CAPACITY;
    if (!tags.empty()) std::memcpy(out, tags.data(), tags.size() * sizeof(agx_tag));
    return AGX_OK;
    });
}

int agx_detect(agx_detector *det, const void *pixels, int width, int height, size_t row_stride_bytes, int format,
               agx_tag *out, uint32_t cap, uint32_t *n_out)
{
    return agx_guard(det, [&]() -> int {
    if (!det || !pixels || !n_out) return fail(det, AGX_ERR_ARG, "null argument");
    if (!format_px_bytes(format)) return fail(det, AGX_ERR_FORMAT, "format must be one of AGX_L8 .. AGX_RGBA16 (agx_format)");
    if (width < 2 || height < 2) return fail(det, AGX_ERR_ARG, "width and height must be >= 2");
    if (format == AGX_LF32) return fail(det, AGX_ERR_FORMAT, "an f32 luma plane carries no u8 luma for the decode: use agx_detect_planes");
    // detector.rs:507-508: u8 luma for the decode, saddle chain on the device.  L8 is its own luma; for
    // L16 / RGB8 the conversion (the integer formulas of luma8()) runs on the device behind the chain -- the
    // frame is there anyway -- and comes back with the saddles
    const bool device_luma = format != AGX_L8;
    std::vector<agx_saddle> &saddles = det->scratch_saddles;
    if (saddles.size() < 16384) saddles.resize(16384);
    uint32_t ns = 0;
    int rc = refined_saddle_points_impl(det, pixels, width, height, row_stride_bytes, format, saddles.data(),
                                        (uint32_t)saddles.size(), &ns, device_luma);
    if (rc == AGX_ERR_CAPACITY && ns > saddles.size()) {  // longer list than ever before: the batch is still fetchable
        saddles.resize(ns);
        rc = refetch_single(det, saddles.data(), (uint32_t)saddles.size(), &ns);
    }
    if (rc) return rc;
    const uint8_t *grey = device_luma ? det->side[SB_LUMA_H].ptr<uint8_t>() : (const uint8_t *)pixels;
    const size_t grey_stride = device_luma ? (size_t)width : row_stride_bytes;
    return agx_detect_from_saddles(det, saddles.data(), ns, grey, width, height, grey_stride, out, cap, n_out);
    });
}

int agx_detect_planes(agx_detector *det, const float *luma32f, size_t stride32f_bytes, const uint8_t *luma8,
                      size_t stride8_bytes, int width, int height, agx_tag *out, uint32_t cap, uint32_t *n_out)
{
    return agx_guard(det, [&]() -> int {
    if (!det || !luma32f || !luma8 || !n_out) return fail(det, AGX_ERR_ARG, "null argument");
    if (width < 2 || height < 2) return fail(det, AGX_ERR_ARG, "width and height must be >= 2");
    if (stride8_bytes < (size_t)width) return fail(det, AGX_ERR_ARG, "row stride smaller than a row");
    std::vector<agx_saddle> &saddles = det->scratch_saddles;
    if (saddles.size() < 16384) saddles.resize(16384);
    uint32_t ns = 0;
    int rc = agx_refined_saddle_points(det, luma32f, width, height, stride32f_bytes, AGX_LF32, saddles.data(),
                                       (uint32_t)saddles.size(), &ns);
    if (rc == AGX_ERR_CAPACITY && ns > saddles.size()) {  // longer list than ever before: the batch is still fetchable
        saddles.resize(ns);
        rc = refetch_single(det, saddles.data(), (uint32_t)saddles.size(), &ns);
    }
    if (rc) return rc;
    return agx_detect_from_saddles(det, saddles.data(), ns, luma8, width, height, stride8_bytes, out, cap, n_out);
    });
}

int agx_profile_enable(agx_detector *det, int on)
{
    if (!det) return AGX_ERR_ARG;
    det->profiling = on < 0 ? 0 : (on > 2 ? 2 : on);
    return AGX_OK;
}

int agx_profile_reset(agx_detector *det)
{
    return agx_guard(det, [&]() -> int {
    if (!det) return AGX_ERR_ARG;
    HIP_TRY(det, hipSetDevice(det->device));
    HIP_TRY(det, hipStreamSynchronize(det->stream));
    harvest_events(det);
    for (int k = 0; k < K_COUNT; ++k) {
        det->prof_ms[k] = 0.0;
        det->prof_launches[k] = 0;
    }
    det->prof_batches = 0;
    return AGX_OK;
    });
}

int agx_profile_read(agx_detector *det, const char **names, double *ms_total, uint64_t *launches)
{
    return agx_guard(det, [&]() -> int {
    if (!det) return AGX_ERR_ARG;
    HIP_TRY(det, hipSetDevice(det->device));
    HIP_TRY(det, hipStreamSynchronize(det->stream));
    harvest_events(det);
    for (int k = 0; k < AGX_N_KERNELS; ++k) {  // the chain has K_COUNT launches; the entries behind them stay empty
        if (names) names[k] = k < K_COUNT ? kKernelNames[k] : nullptr;
        if (ms_total) ms_total[k] = k < K_COUNT ? det->prof_ms[k] : 0.0;
        if (launches) launches[k] = k < K_COUNT ? det->prof_launches[k] : 0;
    }
    return AGX_OK;
    });
}

int agx_detector_constants(const agx_detector *det, float *blur_w7, float *cone25, float *pmat150)
{
    return agx_guard(det, [&]() -> int {
    // det == NULL: compute them afresh (they do not depend on the family or the device)
    float w[7];
    RefineConsts rc;
    if (det) {
        std::memcpy(w, det->blur_w, sizeof w);
        rc = det->rc;
    } else {
        make_blur_weights(1.5f, w);
        make_refine_consts(rc);
    }
    if (blur_w7) std::memcpy(blur_w7, w, sizeof w);
    if (cone25) std::memcpy(cone25, rc.cone, sizeof rc.cone);
    if (pmat150) std::memcpy(pmat150, rc.pmat, sizeof rc.pmat);
    return AGX_OK;
    });
}

namespace {
// AGX_DBG_REDZONES: {buffers, damaged guard bytes, first damaged buffer, its offset (from the payload start, as int32),
// device address of buffer 0's payload (lo, hi)}.  Buffers = the chain's workspace in allocation order, then the side
// buffers that exist, in the order of their slots (staging, luma planes, the device tail's code list / tag rows / frame table,
// .., agx_planes_enqueue's blur planes) -- the pinned HOST ones' guards are read in place.
int fetch_redzones(agx_detector *det, void *host_out, size_t cap_bytes, size_t *n_items)
{
    *n_items = 6;
    if (cap_bytes < 6 * sizeof(uint32_t)) return AGX_ERR_CAPACITY;
    HIP_TRY(det, hipSetDevice(det->device));
    HIP_TRY(det, hipStreamSynchronize(det->stream));
    const size_t rz = det->redzone;
    const uint64_t first_payload = det->device_allocs.empty() ? 0ull : (uint64_t)(uintptr_t)((char *)det->device_allocs[0] + rz);
    uint32_t v[6] = {0u, 0u, 0xffffffffu, 0u, (uint32_t)first_payload, (uint32_t)(first_payload >> 32)};
    std::vector<uint8_t> zone(rz);
    auto check = [&](const void *base, size_t bytes, bool host) -> int {
        const uint32_t index = v[0]++;
        for (int side = 0; rz && side < 2; ++side) {
            const char *src = (const char *)base + (side ? rz + bytes : 0);
            if (host) std::memcpy(zone.data(), src, rz);
            else HIP_TRY(det, hipMemcpy(zone.data(), src, rz, hipMemcpyDeviceToHost));
            for (size_t b = 0; b < rz; ++b)
                if (zone[b] != 0xA5 && v[1]++ == 0) {
                    v[2] = index;
                    v[3] = (uint32_t)(int32_t)(side ? (long long)(bytes + b) : (long long)b - (long long)rz);
                }
        }
        return AGX_OK;
    };
    for (size_t i = 0; i < det->device_allocs.size(); ++i)
        if (int rc = check(det->device_allocs[i], det->alloc_bytes[i], false)) return rc;
    for (const SideBuf &b : det->side)
        if (b.base)
            if (int rc = check(b.base, b.bytes, b.host)) return rc;
    std::memcpy(host_out, v, sizeof v);
    return AGX_OK;
}
}  // namespace

int agx_debug_fetch(agx_detector *det, int frame, int what, void *host_out, size_t cap_bytes, size_t *n_items)
{
    return agx_guard(det, [&]() -> int {
    if (!det || !host_out || !n_items) return fail(det, AGX_ERR_ARG, "null argument");
    if (what == AGX_DBG_REDZONES) return fetch_redzones(det, host_out, cap_bytes, n_items);  // (no batch needed: agx_detect_batch leaves none)
    if (what == AGX_DBG_TAIL_TABLE_ADDR) {  // tests of the guard check: {host address, payload bytes} of the device tail's frame table
        *n_items = 2;
        if (cap_bytes < 2 * sizeof(uint64_t)) return AGX_ERR_CAPACITY;
        const SideBuf &table = det->side[SB_TAIL_TABLE];
        if (!table.base) return fail(det, AGX_ERR_STATE, "no device tail has run on this handle");
        const uint64_t v[2] = {(uint64_t)(uintptr_t)table.payload, (uint64_t)table.bytes};
        std::memcpy(host_out, v, sizeof v);
        return AGX_OK;
    }
    if (!chain_in_flight(det)) return fail(det, AGX_ERR_STATE, "no batch enqueued");
    const ChainArgs &a = det->args;
    if (frame < 0 || frame >= a.n_frames) return fail(det, AGX_ERR_ARG, "frame out of range");
    HIP_TRY(det, hipSetDevice(det->device));
    HIP_TRY(det, hipStreamSynchronize(det->stream));
    const size_t plane = (size_t)a.plane;
    FrameCounters c;
    HIP_TRY(det, hipMemcpy(&c, a.ctr + frame, sizeof c, hipMemcpyDeviceToHost));
    switch (what) {
    case AGX_DBG_BLUR: {
        *n_items = plane;
        if (cap_bytes < plane * sizeof(float)) return AGX_ERR_CAPACITY;
        HIP_TRY(det, hipMemcpy(host_out, a.blur + (size_t)frame * plane, plane * sizeof(float), hipMemcpyDeviceToHost));
        return AGX_OK;
    }
    case AGX_DBG_RESP: {
        // the response K1 evaluated in registers, stored by its "store_response" instantiation
        *n_items = plane;
        if (cap_bytes < plane * sizeof(float)) return AGX_ERR_CAPACITY;
        if (!det->resp_stored)
            return fail(det, AGX_ERR_STATE, "AGX_DBG_RESP needs option store_response=1 before the batch is enqueued");
        HIP_TRY(det, hipMemcpy(host_out, det->side[SB_RESP_STORE].ptr<float>() + (size_t)frame * plane, plane * sizeof(float), hipMemcpyDeviceToHost));
        return AGX_OK;
    }
    case AGX_DBG_RESP_RECOMPUTED: {
        // cross-check: the response recomputed from the stored blur plane by a separate kernel
        *n_items = plane;
        if (cap_bytes < plane * sizeof(float)) return AGX_ERR_CAPACITY;
        float *d_resp = static_cast<float *>(side_ensure(det, SB_DBG_RESP, plane * sizeof(float), 0));
        if (!d_resp) return fail(det, AGX_ERR_HIP, "hipMalloc: response plane");
        hipError_t e = (hipError_t)launch_debug_resp(a, frame, d_resp, det->stream);
        if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_debug_resp: ") + hipGetErrorString(e));
        HIP_TRY(det, hipStreamSynchronize(det->stream));
        HIP_TRY(det, hipMemcpy(host_out, d_resp, plane * sizeof(float), hipMemcpyDeviceToHost));
        return AGX_OK;
    }
    case AGX_DBG_COUNTERS: {
        // flags, seeds, second-tier seeds, clusters, generic candidates, generic roots, refined, out
        *n_items = 8;
        if (cap_bytes < 8 * sizeof(uint32_t)) return AGX_ERR_CAPACITY;
        const uint32_t v[8] = {c.flags, c.n_seeds, c.n_big, c.n_clusters + c.n_clusters2, c.n_cand, c.n_roots, c.n_refined, c.n_out};
        std::memcpy(host_out, v, sizeof v);
        return AGX_OK;
    }
    case 9: {  // AGX_DBG_LUMA8: the u8 luma the device computed for the last agx_detect on an L16 / RGB8 image
        const size_t lb = (size_t)a.W * (size_t)a.H;
        *n_items = lb;
        if (det->side[SB_LUMA_H].bytes < lb) return fail(det, AGX_ERR_STATE, "no device luma: agx_detect on an L16 / RGB8 image first");
        if (cap_bytes < lb) return AGX_ERR_CAPACITY;
        std::memcpy(host_out, det->side[SB_LUMA_H].payload, lb);
        return AGX_OK;
    }
    case 10: {  // wave timeline (debug_ablation & 4096): `frame` selects the kernel (1 = verify, 2 = flood, 3 = refine);
                // cap_bytes / 16 records of {start, end} (100 MHz ticks), one per workgroup in launch order
        if (!a.wave_times || frame < 1 || frame > 3) return fail(det, AGX_ERR_STATE, "wave timeline needs debug_ablation & 4096 on the last batch");
        const size_t n = std::min<size_t>(cap_bytes / 16, WAVE_TIMES_STRIDE);
        *n_items = n;
        HIP_TRY(det, hipMemcpy(host_out, a.wave_times + 2 * (size_t)(frame - 1) * WAVE_TIMES_STRIDE, n * 16, hipMemcpyDeviceToHost));
        return AGX_OK;
    }
    case 7: {  // verify statistics (debug_ablation & 128), 20 x uint32
        *n_items = 20;
        if (cap_bytes < 20 * sizeof(uint32_t)) return AGX_ERR_CAPACITY;
        std::memcpy(host_out, c.stats, sizeof c.stats);
        return AGX_OK;
    }
    case AGX_DBG_MIN: {
        *n_items = 1;
        if (cap_bytes < sizeof(float)) return AGX_ERR_CAPACITY;
        uint32_t key = ~c.min_key_inv;
        uint32_t u = (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
        std::memcpy(host_out, &u, sizeof u);
        return AGX_OK;
    }
    case AGX_DBG_CENTERS: {
        const uint32_t n = std::min(c.n_clusters + c.n_clusters2, a.cap_roots);
        *n_items = n;
        if (cap_bytes < (size_t)n * sizeof(agx_cluster_info)) return AGX_ERR_CAPACITY;
        std::vector<uint32_t> key(n), cnt(n), sx(n), sy(n);
        const size_t cb = (size_t)frame * a.cap_roots;
        HIP_TRY(det, hipMemcpy(key.data(), a.clu_key + cb, (size_t)n * 4, hipMemcpyDeviceToHost));
        HIP_TRY(det, hipMemcpy(cnt.data(), a.clu_cnt + cb, (size_t)n * 4, hipMemcpyDeviceToHost));
        HIP_TRY(det, hipMemcpy(sx.data(), a.clu_sx + cb, (size_t)n * 4, hipMemcpyDeviceToHost));
        HIP_TRY(det, hipMemcpy(sy.data(), a.clu_sy + cb, (size_t)n * 4, hipMemcpyDeviceToHost));
        std::vector<agx_cluster_info> info(n);
        for (uint32_t i = 0; i < n; ++i) {
            info[i].first_index = key[i];
            info[i].size = cnt[i];
            std::memcpy(&info[i].cx, &sx[i], 4);  // K4 leaves the f32 centroid here
            std::memcpy(&info[i].cy, &sy[i], 4);
        }
        std::sort(info.begin(), info.end(),
                  [](const agx_cluster_info &p, const agx_cluster_info &q) { return p.first_index < q.first_index; });
        std::memcpy(host_out, info.data(), (size_t)n * sizeof(agx_cluster_info));
        return AGX_OK;
    }
    case AGX_DBG_REFINED: {
        const uint32_t n = c.n_refined;
        *n_items = n;
        if (cap_bytes < (size_t)n * sizeof(agx_saddle)) return AGX_ERR_CAPACITY;
        std::vector<RefinedRec> rec(n);
        HIP_TRY(det, hipMemcpy(rec.data(), a.refined + (size_t)frame * a.cap_roots, (size_t)n * sizeof(RefinedRec),
                               hipMemcpyDeviceToHost));
        std::sort(rec.begin(), rec.end(), [](const RefinedRec &p, const RefinedRec &q) { return p.key < q.key; });
        agx_saddle *o = (agx_saddle *)host_out;
        for (uint32_t i = 0; i < n; ++i) o[i] = {rec[i].x, rec[i].y, rec[i].k, rec[i].theta, rec[i].phi};
        return AGX_OK;
    }
    default: return fail(det, AGX_ERR_ARG, "unknown debug item");
    }
    });
}

}  // extern "C"
