// render.hip -- the board through pose and lens model: k_render_boards<LENS> (agx_render_boards_enqueue) and its host form
// (agx_render_boards_tail).  Every number is render_math.h's in both forms: the two give the same bytes.
//
// k_render_boards: a workgroup of 256 lanes covers a tile of one frame (blockIdx.y) -- 256 consecutive quads of the row-major
// list of 4-pixel quads, k_remap's numbering, so a wave covers 256 adjacent pixels or several short rows and no lane idles on a
// width that is no multiple of 256.  The frame's pose is read through a uniform address (scalar loads), the prepared camera and
// the layout are kernel arguments (scalar registers), and the layout's rows cols <= 640 code words go to LDS once per workgroup.
// Every workgroup derives the frame's status from the pose by the same statements (uniform, before its first store); the frame's
// first workgroup also writes d_status, d_n_truth and the truth rows (pose_predict<LENS>: the pose kernel's d_pred bytes).
// A lane classifies the S x S samples of its four pixels one after the other (binary64: the inverse of the forward projection per
// sample), counts white and black samples in integers, shades in uint32, and stores one dword (two for L16) where the
// destination's pointer and strides are multiples of the quad's size and all four pixels are written; byte / half-word stores for
// the last pixels of a row whose width is no multiple of 4, for any other destination, and under AGX_RENDER_KEEP_BACKGROUND for
// a quad of which some pixel has no sample on the page (that pixel is not written at all).  No scratch, no atomics.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "render.h"
#include "render_math.h"

namespace agx {
namespace {

#include "tag_families_data.inc"

constexpr unsigned RENDER_BLOCK = 256;

// the family's code table (the .inc's arrays are constants: the device code reads its own copy of them)
AGX_HD const uint64_t *render_codes(int family)
{
    switch (family) {
    case AGX_T16H5: return kT16H5;
    case AGX_T25H7: return kT25H7;
    case AGX_T25H9: return kT25H9;
    default: return kT36H11;  // AGX_T36H11, AGX_T36H11B1
    }
}

AGX_HD Pose render_pose(const double *p)
{
    Pose o;
#pragma unroll
    for (int i = 0; i < 9; ++i) o.R[i] = p[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) o.t[i] = p[9 + i];
    return o;
}

// the frame's status words and truth rows; lane of n lanes
template <int LENS>
AGX_HD void render_truth(const RenderArgs &a, const Pose &pose, uint32_t f, uint32_t st, uint32_t lane, uint32_t n)
{
    const uint32_t nb = a.g.g.n_board;
    if (lane == 0) {
        a.status[f] = st;
        a.n_truth[f] = st == AGX_RENDER_OK ? nb : 0u;
    }
    if (st != AGX_RENDER_OK) return;
    uint32_t *rows = reinterpret_cast<uint32_t *>(a.truth + (size_t)f * nb);
    for (uint32_t t = lane; t < nb; t += n) {
        float xy[8];
        pose_predict<LENS>(a.g.g, a.g.tag_size, a.g.cam, pose, t, xy);
        uint32_t *row = rows + 9u * (size_t)t;
        row[0] = a.g.g.first_id + t;
#pragma unroll
        for (int j = 0; j < 8; ++j) row[1 + j] = f32_bits(xy[j]);
    }
}

template <int LENS, typename T>
__global__ void __launch_bounds__(RENDER_BLOCK) k_render_boards(RenderArgs a, uint32_t quads_per_row, uint32_t n_quads, int dst_vec)
{
    __shared__ uint64_t s_codes[RENDER_MAX_CODES];
    const uint32_t f = blockIdx.y;
    const Pose pose = render_pose(a.poses + 12u * (size_t)f);
    const uint64_t *table = render_codes(a.family) + a.g.g.first_id;
    for (uint32_t t = threadIdx.x; t < a.g.g.n_board; t += RENDER_BLOCK) s_codes[t] = table[t];  // (n_board <= RENDER_MAX_CODES)
    __syncthreads();
    const uint32_t st = render_frame_status<LENS>(a.g, pose);
    if (blockIdx.x == 0) render_truth<LENS>(a, pose, f, st, threadIdx.x, RENDER_BLOCK);
    const bool keep = (a.g.flags & AGX_RENDER_KEEP_BACKGROUND) != 0;
    if (st == AGX_RENDER_INPUT || (st == AGX_RENDER_EMPTY && keep)) return;
    const uint32_t q = blockIdx.x * RENDER_BLOCK + threadIdx.x;
    if (q >= n_quads) return;
    const uint32_t row = q / quads_per_row, x = (q - row * quads_per_row) * RENDER_PX;  // row < height, x < width
    const uint32_t left = (uint32_t)a.width - x, npx = left < (uint32_t)RENDER_PX ? left : (uint32_t)RENDER_PX;
    constexpr uint32_t BITS = 8u * (uint32_t)sizeof(T);
    constexpr uint64_t MASK = (1ull << BITS) - 1ull;
    unsigned char *d = static_cast<unsigned char *>(a.frames) + (size_t)f * a.frame_stride + (size_t)row * a.row_stride + (size_t)x * sizeof(T);
    const bool whole = dst_vec && npx == (uint32_t)RENDER_PX;
    uint64_t cur = 0;  // the quad's pixels as they are (under AGX_RENDER_KEEP_BACKGROUND)
    if (keep) {
        if (whole) {
            if constexpr (sizeof(T) == 1) {
                cur = *reinterpret_cast<const uint32_t *>(d);
            } else {
                const uint2 w = *reinterpret_cast<const uint2 *>(d);
                cur = (uint64_t)w.x | ((uint64_t)w.y << 32);
            }
        } else {
#pragma unroll 1
            for (uint32_t k = 0; k < npx; ++k) cur |= (uint64_t)reinterpret_cast<const T *>(d)[k] << (k * BITS);
        }
    }
    uint64_t out = 0;
    uint32_t written = 0;
#pragma unroll 1
    for (uint32_t k = 0; k < npx; ++k) {
        uint32_t n_w = 0, n_b = 0;
        if (st == AGX_RENDER_OK) render_pixel<LENS>(a.g, pose, s_codes, x + k, row, n_w, n_b);
        const uint32_t bg = keep ? (uint32_t)((cur >> (k * BITS)) & MASK) : a.g.background;
        out |= (uint64_t)render_shade(a.g, n_w, n_b, bg) << (k * BITS);
        if (!keep || n_w + n_b) written |= 1u << k;
    }
    if (whole && written == 15u) {
        if constexpr (sizeof(T) == 1) {
            *reinterpret_cast<uint32_t *>(d) = (uint32_t)out;
        } else {
            *reinterpret_cast<uint2 *>(d) = make_uint2((uint32_t)out, (uint32_t)(out >> 32));
        }
    } else {
#pragma unroll 1
        for (uint32_t k = 0; k < npx; ++k)
            if ((written >> k) & 1u) reinterpret_cast<T *>(d)[k] = (T)((out >> (k * BITS)) & MASK);
    }
}

}  // namespace

bool render_family(int family, int &edge, int &border, uint32_t &n_codes)
{
    switch (family) {  // src/detector.rs:369-405
    case AGX_T16H5: edge = 4, border = 2, n_codes = 30; return true;
    case AGX_T25H7: edge = 5, border = 2, n_codes = 242; return true;
    case AGX_T25H9: edge = 5, border = 2, n_codes = 35; return true;
    case AGX_T36H11: edge = 6, border = 2, n_codes = 587; return true;
    case AGX_T36H11B1: edge = 6, border = 1, n_codes = 587; return true;
    default: return false;
    }
}

const char *render_args_bad(const RenderArgs &a, const agx_camera &camera, const agx_render_params &p, bool device)
{
    if (!a.poses || !a.frames || !a.truth || !a.n_truth || !a.status) return "a null array";
    if (device ? (a.n_frames < 1 || a.n_frames > 65535) : a.n_frames != 1) return "n_frames must be in 1 .. 65535";
    if (a.format != AGX_L8 && a.format != AGX_L16) return "format must be AGX_L8 or AGX_L16";
    if (a.width < 1 || a.width > RENDER_MAX_SIDE || a.height < 1 || a.height > RENDER_MAX_SIDE) return "width and height must be in 1 .. 16384";
    const size_t px = a.format == AGX_L16 ? 2 : 1;
    if (a.row_stride < (size_t)a.width * px || a.row_stride > 0x7fffffffu || a.row_stride * (size_t)a.height > 0x7fffffffu)
        return "a row stride must cover a row and a frame must be below 2^31 bytes";
    if (a.n_frames > 1 && a.frame_stride < a.row_stride * (size_t)a.height) return "a frame stride must cover a frame";
    if (px == 2 && (((uintptr_t)a.frames | a.row_stride | (a.n_frames > 1 ? a.frame_stride : 0)) & 1)) return "16-bit pixels must be 2-byte aligned";
    const uint32_t cols = a.g.g.cols, rows = cols ? a.g.g.n_board / cols : 0;
    if (!cols || !rows || (uint64_t)cols * rows > FIT_MAX_BOARD || !(a.g.s >= 0.0) || !f64_finite(a.g.s))
        return "rows * cols in 1 .. 4096, spacing_ratio finite and >= 0";
    if (!pose_args_ok(a.lens, camera, a.g.tag_size, 0)) return AGX_LENS_CAMERA_RULE ", tag_size finite and > 0";
    int edge, border;
    uint32_t n_codes;
    if (!render_family(a.family, edge, border, n_codes)) return "an unknown family";
    if ((uint64_t)a.g.g.first_id + (uint64_t)cols * rows > n_codes) return "the family's code table is shorter than first_id + rows * cols";
    if (p.supersample < 1 || p.supersample > (uint32_t)RENDER_MAX_SUPERSAMPLE) return "supersample must be in 1 .. 4";
    const uint32_t top = a.format == AGX_L16 ? 65535u : 255u;
    if (p.black > top || p.white > top || p.background > top) return "black, white and background must be below 256 (AGX_L8) or 65536 (AGX_L16)";
    if (!f32_finite(p.page_margin) || !(p.page_margin >= 0.0f)) return "page_margin must be finite and >= 0";
    if (p.flags & ~(uint32_t)AGX_RENDER_KEEP_BACKGROUND) return "flags AGX_RENDER_KEEP_BACKGROUND or 0";
    if (((uintptr_t)a.poses & 7) || (((uintptr_t)a.truth | (uintptr_t)a.n_truth | (uintptr_t)a.status) & 3))
        return "the poses must be 8-byte aligned, the truth rows, counts and statuses 4-byte aligned";
    return nullptr;
}

int launch_render_boards(const RenderArgs &a, void *stream)
{
    const uint32_t quads_per_row = ((uint32_t)a.width + RENDER_PX - 1) / RENDER_PX, n_quads = quads_per_row * (uint32_t)a.height;  // <= 2^26
    const size_t quad_bytes = (size_t)RENDER_PX * (a.format == AGX_L16 ? 2 : 1);
    const int dst_vec = (((uintptr_t)a.frames | a.row_stride | (a.n_frames > 1 ? a.frame_stride : 0)) % quad_bytes) == 0;
    const dim3 grid((n_quads + RENDER_BLOCK - 1) / RENDER_BLOCK, (unsigned)a.n_frames);
    with_lens(a.lens, [&](auto L) {
        constexpr int LENS = decltype(L)::value;
        if (a.format == AGX_L16)
            hipLaunchKernelGGL((k_render_boards<LENS, uint16_t>), grid, dim3(RENDER_BLOCK), 0, (hipStream_t)stream, a, quads_per_row, n_quads, dst_vec);
        else
            hipLaunchKernelGGL((k_render_boards<LENS, uint8_t>), grid, dim3(RENDER_BLOCK), 0, (hipStream_t)stream, a, quads_per_row, n_quads, dst_vec);
    });
    return (int)hipGetLastError();
}

// ---- the host form -----------------------------------------------------------------------------------------------------------------
namespace {

template <int LENS, typename T>
void render_boards_host_t(const RenderArgs &a)
{
    const uint64_t *codes = render_codes(a.family) + a.g.g.first_id;
    const bool keep = (a.g.flags & AGX_RENDER_KEEP_BACKGROUND) != 0;
    for (int f = 0; f < a.n_frames; ++f) {
        const Pose pose = render_pose(a.poses + 12u * (size_t)f);
        const uint32_t st = render_frame_status<LENS>(a.g, pose);
        render_truth<LENS>(a, pose, (uint32_t)f, st, 0, 1);
        if (st == AGX_RENDER_INPUT || (st == AGX_RENDER_EMPTY && keep)) continue;
        for (int row = 0; row < a.height; ++row) {
            T *d = reinterpret_cast<T *>(static_cast<unsigned char *>(a.frames) + (size_t)f * a.frame_stride + (size_t)row * a.row_stride);
            for (int col = 0; col < a.width; ++col) {
                uint32_t n_w = 0, n_b = 0;
                if (st == AGX_RENDER_OK) render_pixel<LENS>(a.g, pose, codes, (uint32_t)col, (uint32_t)row, n_w, n_b);
                if (keep && !(n_w + n_b)) continue;
                d[col] = (T)render_shade(a.g, n_w, n_b, keep ? (uint32_t)d[col] : a.g.background);
            }
        }
    }
}

}  // namespace

void render_boards_host(const RenderArgs &a)
{
    with_lens(a.lens, [&](auto L) {
        constexpr int LENS = decltype(L)::value;
        if (a.format == AGX_L16) render_boards_host_t<LENS, uint16_t>(a);
        else render_boards_host_t<LENS, uint8_t>(a);
    });
}

}  // namespace agx
