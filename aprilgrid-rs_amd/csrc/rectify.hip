// rectify.hip -- rectified batches: k_rectify_map (agx_rectify_map_enqueue), k_remap (agx_remap_enqueue), k_rectified_points
// (agx_rectified_points_enqueue) and their host forms.  Every number is rectify_math.h's in both forms: the two give the same bytes.
//
// k_rectify_map, k_rectified_points: one lane per destination pixel / per point, binary64 through board_pose_math.h's projection.
// Once per camera and once per tag table: not the hot path.
//
// k_remap, the hot path: a bandwidth-bound gather with no floating-point operation.  A lane owns REMAP_PX = 4 adjacent destination
// pixels of one row and a workgroup REMAP_FRAMES_PER_GROUP = 16 frames (blockIdx.y): the lane loads its four 8-byte map entries
// once (32 contiguous bytes), turns each into two row offsets, a column step and two weights (remap_tap: 24 registers for the
// four), and applies them to the group's frames in turn -- 16 byte (or half-word) gathers and one dword (two for L16) store per
// frame.  The map is read once per frame group, so at 16 frames it costs 0.5 byte per destination pixel and frame beside the
// 1 byte in and 1 byte out, and the 8 MB map of a 1280 x 800 target comes out of the cache behind the first group.  The lanes are
// numbered along the rows (quad q of the row-major list of 4-pixel quads), so a wave covers 256 adjacent destination pixels, or
// several short rows: no lane idles on a width that is no multiple of 256, and the gathered source bytes of a wave are neighbours.
// Offsets are 32-bit from the frame's first pixel (a frame is below 2^31 bytes), which leaves the frame's address in scalar
// registers.  A destination whose pointer and strides are multiples of the quad's size takes whole-dword stores; any other, and
// the last pixels of a row whose width is no multiple of 4, byte / half-word stores.  No LDS: every source byte is used by at
// most four neighbouring taps, which the vector cache already serves.  An entry outside the source reads pixel (0, 0) and stores
// `border`: no branch in the loop, no address outside the frame.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rectify.h"
#include "rectify_math.h"

namespace agx {
namespace {

constexpr unsigned RECT_BLOCK = 256;

template <int LENS>
__global__ void __launch_bounds__(RECT_BLOCK) k_rectify_map(RectifyMapArgs a)
{
    const uint32_t i = blockIdx.x * RECT_BLOCK + threadIdx.x;  // (dst_w * dst_h <= 2^28)
    if (i >= (uint32_t)a.dst_w * (uint32_t)a.dst_h) return;
    const uint32_t row = i / (uint32_t)a.dst_w, col = i - row * (uint32_t)a.dst_w;
    double u = 0.0, v = 0.0;
    const bool ok = rectify_point<LENS>(a.g, (double)col, (double)row, u, v);
    int32_t mx, my;
    rectify_entry(ok, u, v, a.src_w, a.src_h, mx, my);
    int2 *e = reinterpret_cast<int2 *>(reinterpret_cast<unsigned char *>(a.map) + (size_t)row * a.map_stride) + col;
    *e = make_int2(mx, my);
}

template <int LENS>
__global__ void __launch_bounds__(RECT_BLOCK) k_rectified_points(RectifiedPointsArgs a)
{
    const uint32_t i = blockIdx.x * RECT_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const float *p = reinterpret_cast<const float *>(static_cast<const unsigned char *>(a.points) + (size_t)i * a.stride);
    const float x = p[0], y = p[1];  // (read before the store: in place is allowed)
    float u, v;
    rectify_point_f32<LENS>(a.g, x, y, u, v);
    float *o = reinterpret_cast<float *>(static_cast<unsigned char *>(a.out) + (size_t)i * a.out_stride);
    o[0] = u;
    o[1] = v;
}

template <typename T>
__global__ void __launch_bounds__(RECT_BLOCK) k_remap(RemapArgs a, uint32_t quads_per_row, uint32_t n_quads, int dst_vec)
{
    const uint32_t q = blockIdx.x * RECT_BLOCK + threadIdx.x;
    if (q >= n_quads) return;
    const uint32_t row = q / quads_per_row, x = (q - row * quads_per_row) * REMAP_PX;  // row < dst_h, x < dst_w
    const uint32_t left = (uint32_t)a.dst_w - x, npx = left < (uint32_t)REMAP_PX ? left : (uint32_t)REMAP_PX;
    const int2 *m = reinterpret_cast<const int2 *>(reinterpret_cast<const unsigned char *>(a.map) + (size_t)row * a.map_stride) + x;
    RemapTap tap[REMAP_PX];
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)REMAP_PX; ++k) {
        int2 e = make_int2(RECT_NONE, RECT_NONE);
        if (k < npx) e = m[k];  // (x + k < dst_w: inside the map's row)
        tap[k] = remap_tap(e.x, e.y, a.src_w, a.src_h, (uint32_t)a.src_row_stride, (uint32_t)sizeof(T));
    }
    const uint32_t f0 = blockIdx.y * (uint32_t)REMAP_FRAMES_PER_GROUP;
    const uint32_t fe = f0 + (uint32_t)REMAP_FRAMES_PER_GROUP, f1 = fe < (uint32_t)a.n_frames ? fe : (uint32_t)a.n_frames;
    const uint32_t d_off = row * (uint32_t)a.dst_row_stride + x * (uint32_t)sizeof(T);  // (a frame is below 2^31 bytes)
    const bool whole = dst_vec && npx == (uint32_t)REMAP_PX;
    for (uint32_t f = f0; f < f1; ++f) {
        const unsigned char *src = static_cast<const unsigned char *>(a.src) + (size_t)f * a.src_frame_stride;
        unsigned char *d = static_cast<unsigned char *>(a.dst) + (size_t)f * a.dst_frame_stride + d_off;
        uint32_t v[REMAP_PX];
#pragma unroll
        for (int k = 0; k < REMAP_PX; ++k) v[k] = remap_blend<T>(src, tap[k], a.border);
        if (whole) {
            if constexpr (sizeof(T) == 1) {
                *reinterpret_cast<uint32_t *>(d) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
            } else {
                *reinterpret_cast<uint2 *>(d) = make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16));
            }
        } else {
#pragma unroll
            for (uint32_t k = 0; k < (uint32_t)REMAP_PX; ++k)
                if (k < npx) reinterpret_cast<T *>(d)[k] = (T)v[k];
        }
    }
}

inline bool side_ok(int v, int max) { return v >= 1 && v <= max; }

// a batch of L8 / L16 frames of w x h with n frames: strides cover a row / a frame, a frame below 2^31 bytes, 16-bit alignment
const char *frames_bad(const void *p, int n, int w, int h, size_t row, size_t frame, int format)
{
    const size_t px = format == AGX_L16 ? 2 : 1;
    if (row < (size_t)w * px || row > 0x7fffffffu || row * (size_t)h > 0x7fffffffu) return "a row stride must cover a row and a frame must be below 2^31 bytes";
    if (n > 1 && frame < row * (size_t)h) return "a frame stride must cover a frame";
    if (px == 2 && (((uintptr_t)p | row | (n > 1 ? frame : 0)) & 1)) return "16-bit pixels must be 2-byte aligned";
    return nullptr;
}

}  // namespace

const char *rectify_map_args_bad(const RectifyMapArgs &a)
{
    if (!a.map) return "a null map";
    if (!side_ok(a.src_w, RECT_MAX_SIDE) || !side_ok(a.src_h, RECT_MAX_SIDE) || !side_ok(a.dst_w, RECT_MAX_SIDE) || !side_ok(a.dst_h, RECT_MAX_SIDE))
        return "source and target sizes must be in 1 .. 16384";
    if ((a.map_stride & 7) || a.map_stride < 8 * (size_t)a.dst_w || ((uintptr_t)a.map & 7))
        return "the map must be 8-byte aligned and its row stride a multiple of 8 that covers 8 dst_width bytes";
    return nullptr;
}

const char *remap_args_bad(const RemapArgs &a)
{
    if (!a.src || !a.dst || !a.map) return "a null batch or map";
    if (a.n_frames < 1 || a.n_frames > 65535) return "n_frames must be in 1 .. 65535";
    if (a.format != AGX_L8 && a.format != AGX_L16) return "format must be AGX_L8 or AGX_L16";
    if (!side_ok(a.src_w, 65000) || !side_ok(a.src_h, 65000) || (long long)a.src_w * a.src_h >= (1ll << 30))
        return "the source's sides must be in 1 .. 65000 and its frame below 2^30 px";
    if (!side_ok(a.dst_w, RECT_MAX_SIDE) || !side_ok(a.dst_h, RECT_MAX_SIDE)) return "the target's sides must be in 1 .. 16384";
    if (const char *bad = frames_bad(a.src, a.n_frames, a.src_w, a.src_h, a.src_row_stride, a.src_frame_stride, a.format)) return bad;
    if (const char *bad = frames_bad(a.dst, a.n_frames, a.dst_w, a.dst_h, a.dst_row_stride, a.dst_frame_stride, a.format)) return bad;
    if ((a.map_stride & 7) || a.map_stride < 8 * (size_t)a.dst_w || ((uintptr_t)a.map & 7))
        return "the map must be 8-byte aligned and its row stride a multiple of 8 that covers 8 dst_width bytes";
    if (a.border > (a.format == AGX_L16 ? 65535u : 255u)) return "border must be below 256 (AGX_L8) or 65536 (AGX_L16)";
    return nullptr;
}

const char *rectified_points_args_bad(const RectifiedPointsArgs &a)
{
    if (a.n && (!a.points || !a.out)) return "a null point list";
    if (a.n >= (1u << 30)) return "at most 2^30 - 1 points";
    if ((a.stride & 3) || a.stride < 8 || (a.out_stride & 3) || a.out_stride < 8 || (((uintptr_t)a.points | (uintptr_t)a.out) & 3))
        return "point lists must be 4-byte aligned with strides that are multiples of 4 and at least 8";
    return nullptr;
}

int launch_rectify_map(const RectifyMapArgs &a, void *stream)
{
    if (rectify_map_args_bad(a)) return (int)hipErrorInvalidValue;
    const unsigned grid = (unsigned)(((size_t)a.dst_w * a.dst_h + RECT_BLOCK - 1) / RECT_BLOCK);
    with_lens(a.lens, [&](auto L) { hipLaunchKernelGGL(k_rectify_map<decltype(L)::value>, dim3(grid), dim3(RECT_BLOCK), 0, (hipStream_t)stream, a); });
    return (int)hipGetLastError();
}

int launch_rectified_points(const RectifiedPointsArgs &a, void *stream)
{
    if (rectified_points_args_bad(a)) return (int)hipErrorInvalidValue;
    if (!a.n) return (int)hipSuccess;
    const unsigned grid = (a.n + RECT_BLOCK - 1) / RECT_BLOCK;
    with_lens(a.lens, [&](auto L) { hipLaunchKernelGGL(k_rectified_points<decltype(L)::value>, dim3(grid), dim3(RECT_BLOCK), 0, (hipStream_t)stream, a); });
    return (int)hipGetLastError();
}

int launch_remap(const RemapArgs &a, void *stream)
{
    if (remap_args_bad(a)) return (int)hipErrorInvalidValue;
    const uint32_t quads_per_row = ((uint32_t)a.dst_w + REMAP_PX - 1) / REMAP_PX, n_quads = quads_per_row * (uint32_t)a.dst_h;  // <= 2^26
    const size_t quad_bytes = (size_t)REMAP_PX * (a.format == AGX_L16 ? 2 : 1);
    const int dst_vec = (((uintptr_t)a.dst | a.dst_row_stride | (a.n_frames > 1 ? a.dst_frame_stride : 0)) % quad_bytes) == 0;
    const dim3 grid((n_quads + RECT_BLOCK - 1) / RECT_BLOCK, ((unsigned)a.n_frames + REMAP_FRAMES_PER_GROUP - 1) / REMAP_FRAMES_PER_GROUP);
    if (a.format == AGX_L16)
        hipLaunchKernelGGL(k_remap<uint16_t>, grid, dim3(RECT_BLOCK), 0, (hipStream_t)stream, a, quads_per_row, n_quads, dst_vec);
    else
        hipLaunchKernelGGL(k_remap<uint8_t>, grid, dim3(RECT_BLOCK), 0, (hipStream_t)stream, a, quads_per_row, n_quads, dst_vec);
    return (int)hipGetLastError();
}

// ---- the host forms ---------------------------------------------------------------------------------------------------------------
namespace {

template <int LENS>
void rectify_map_host_t(const RectifyMapArgs &a)
{
    for (int row = 0; row < a.dst_h; ++row) {
        int32_t *e = reinterpret_cast<int32_t *>(reinterpret_cast<unsigned char *>(a.map) + (size_t)row * a.map_stride);
        for (int col = 0; col < a.dst_w; ++col) {
            double u = 0.0, v = 0.0;
            const bool ok = rectify_point<LENS>(a.g, (double)col, (double)row, u, v);
            rectify_entry(ok, u, v, a.src_w, a.src_h, e[2 * col], e[2 * col + 1]);
        }
    }
}

template <int LENS>
void rectified_points_host_t(const RectifiedPointsArgs &a)
{
    for (uint32_t i = 0; i < a.n; ++i) {
        const float *p = reinterpret_cast<const float *>(static_cast<const unsigned char *>(a.points) + (size_t)i * a.stride);
        const float x = p[0], y = p[1];
        float u, v;
        rectify_point_f32<LENS>(a.g, x, y, u, v);
        float *o = reinterpret_cast<float *>(static_cast<unsigned char *>(a.out) + (size_t)i * a.out_stride);
        o[0] = u;
        o[1] = v;
    }
}

template <typename T>
void remap_host_t(const RemapArgs &a)
{
    for (int row = 0; row < a.dst_h; ++row) {
        const int32_t *m = reinterpret_cast<const int32_t *>(reinterpret_cast<const unsigned char *>(a.map) + (size_t)row * a.map_stride);
        for (int col = 0; col < a.dst_w; ++col) {
            const RemapTap tap = remap_tap(m[2 * col], m[2 * col + 1], a.src_w, a.src_h, (uint32_t)a.src_row_stride, (uint32_t)sizeof(T));
            for (int f = 0; f < a.n_frames; ++f) {
                const unsigned char *src = static_cast<const unsigned char *>(a.src) + (size_t)f * a.src_frame_stride;
                T *d = reinterpret_cast<T *>(static_cast<unsigned char *>(a.dst) + (size_t)f * a.dst_frame_stride + (size_t)row * a.dst_row_stride);
                d[col] = (T)remap_blend<T>(src, tap, a.border);
            }
        }
    }
}

}  // namespace

void rectify_map_host(const RectifyMapArgs &a)
{
    with_lens(a.lens, [&](auto L) { rectify_map_host_t<decltype(L)::value>(a); });
}

void rectified_points_host(const RectifiedPointsArgs &a)
{
    with_lens(a.lens, [&](auto L) { rectified_points_host_t<decltype(L)::value>(a); });
}

void remap_host(const RemapArgs &a)
{
    if (a.format == AGX_L16) remap_host_t<uint16_t>(a);
    else remap_host_t<uint8_t>(a);
}

}  // namespace agx
