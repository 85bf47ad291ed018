// decimate.hip -- k_decimate (agx_decimate_enqueue) and its host form: a batch of L8 / L16 frames averaged down by a factor F in
// 2 .. 4, out(X, Y) = (sum of the F x F source pixels + F F / 2) / (F F) in uint32 (decimate_math.h).  The two forms give the
// same bytes.
//
// The kernel is bound by bytes: F F source bytes in, one out, no reuse between lanes, so no LDS and nothing kept beyond four
// sums.  A lane owns DECIMATE_PX = 4 adjacent output pixels of one row: their source is, in each of F source rows, one
// segment of 4 F pixels (8 .. 32 bytes), adjacent to the next lane's -- a wave reads 256 F adjacent pixels of a row.  Each segment
// is read once, by loads of LW = 16, 8 or 4 bytes: the widest that divides the segment and the source's alignment (pointer, row
// stride and, with more than one frame, frame stride); a source with none of these (LW = 0), and the last lane of a row whose
// output width is no multiple of 4 (a whole segment could reach past the row's src_w pixels), read pixel by pixel -- the same
// sums.  A destination whose pointer and strides are multiples of the quad's size takes one dword (two for L16) per lane, any
// other, and the short last quad, pixel stores: never a byte beyond the row's output pixels is written.
// Block (64, 4): 64 quads of 4 output rows; grid (quads / 64, rows / 4, frames).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "decimate.h"

namespace agx {
namespace {

constexpr unsigned DEC_BX = 64, DEC_BY = 4;

template <int LW>
struct DecLoad;
template <>
struct DecLoad<4> {
    typedef uint32_t type;
};
template <>
struct DecLoad<8> {
    typedef uint2 type;
};
template <>
struct DecLoad<16> {
    typedef uint4 type;
};

// pixel k of a segment held as dwords
template <typename T>
__device__ __forceinline__ uint32_t seg_px(const uint32_t *seg, int k)
{
    if constexpr (sizeof(T) == 1) return (seg[k >> 2] >> (8 * (k & 3))) & 0xffu;
    else return (seg[k >> 1] >> (16 * (k & 1))) & 0xffffu;
}

template <typename T, int F, int LW>
__global__ void __launch_bounds__(DEC_BX *DEC_BY) k_decimate(DecimateArgs a, uint32_t quads_per_row, int dst_vec)
{
    const uint32_t q = blockIdx.x * DEC_BX + threadIdx.x, Y = blockIdx.y * DEC_BY + threadIdx.y;
    const uint32_t out_w = (uint32_t)a.src_w / (uint32_t)F, out_h = (uint32_t)a.src_h / (uint32_t)F;
    if (q >= quads_per_row || Y >= out_h) return;
    const uint32_t X0 = q * (uint32_t)DECIMATE_PX, left = out_w - X0, npx = left < (uint32_t)DECIMATE_PX ? left : (uint32_t)DECIMATE_PX;
    const unsigned char *frame = static_cast<const unsigned char *>(a.src) + (size_t)blockIdx.z * a.src_frame_stride;
    constexpr int SEG_BYTES = DECIMATE_PX * F * (int)sizeof(T), SEG_DW = SEG_BYTES / 4;
    uint32_t v[DECIMATE_PX] = {0u, 0u, 0u, 0u};
    if (LW != 0 && npx == (uint32_t)DECIMATE_PX) {
        // (4 q + 4) F <= out_w F <= src_w: the segment lies inside the row's pixels
        const unsigned char *seg0 = frame + (size_t)Y * F * a.src_row_stride + (size_t)X0 * F * sizeof(T);
        uint32_t sum[DECIMATE_PX] = {0u, 0u, 0u, 0u};
        if constexpr (LW != 0) {
            typedef typename DecLoad<LW>::type load_t;
            constexpr int N_LOADS = SEG_BYTES / LW, DW_PER_LOAD = LW / 4;
            load_t raw[F][N_LOADS];
#pragma unroll
            for (int dy = 0; dy < F; ++dy)
#pragma unroll
                for (int e = 0; e < N_LOADS; ++e) raw[dy][e] = reinterpret_cast<const load_t *>(seg0 + (size_t)dy * a.src_row_stride)[e];
#pragma unroll
            for (int dy = 0; dy < F; ++dy) {
                uint32_t seg[SEG_DW];
#pragma unroll
                for (int e = 0; e < N_LOADS; ++e) {
                    if constexpr (LW == 4) {
                        seg[e] = raw[dy][e];
                    } else if constexpr (LW == 8) {
                        seg[DW_PER_LOAD * e] = raw[dy][e].x;
                        seg[DW_PER_LOAD * e + 1] = raw[dy][e].y;
                    } else {
                        seg[DW_PER_LOAD * e] = raw[dy][e].x;
                        seg[DW_PER_LOAD * e + 1] = raw[dy][e].y;
                        seg[DW_PER_LOAD * e + 2] = raw[dy][e].z;
                        seg[DW_PER_LOAD * e + 3] = raw[dy][e].w;
                    }
                }
#pragma unroll
                for (int j = 0; j < DECIMATE_PX; ++j)
#pragma unroll
                    for (int dx = 0; dx < F; ++dx) sum[j] += seg_px<T>(seg, j * F + dx);
            }
        }
#pragma unroll
        for (int j = 0; j < DECIMATE_PX; ++j) v[j] = decimate_mean<F>(sum[j]);
    } else {
#pragma unroll
        for (uint32_t j = 0; j < (uint32_t)DECIMATE_PX; ++j)
            if (j < npx) v[j] = decimate_px<T, F>(frame, a.src_row_stride, X0 + j, Y);
    }
    unsigned char *d = static_cast<unsigned char *>(a.dst) + (size_t)blockIdx.z * a.dst_frame_stride + (size_t)Y * a.dst_row_stride +
                       (size_t)X0 * sizeof(T);
    if (dst_vec && npx == (uint32_t)DECIMATE_PX) {
        if constexpr (sizeof(T) == 1) {
            *reinterpret_cast<uint32_t *>(d) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        } else {
            *reinterpret_cast<uint2 *>(d) = make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16));
        }
    } else {
#pragma unroll
        for (uint32_t j = 0; j < (uint32_t)DECIMATE_PX; ++j)
            if (j < npx) reinterpret_cast<T *>(d)[j] = (T)v[j];
    }
}

// strides cover a row / a frame, 16-bit pixels are 2-byte aligned
const char *frames_bad(const void *p, int n, int w, int h, size_t row, size_t frame, size_t px)
{
    if (row < (size_t)w * px || row > 0x7fffffffu) return "a row stride must cover a row and be below 2^31";
    if (n > 1 && frame < row * (size_t)h) return "a frame stride must cover a frame";
    if (px == 2 && (((uintptr_t)p | row | (n > 1 ? frame : 0)) & 1)) return "16-bit pixels must be 2-byte aligned";
    return nullptr;
}

template <typename T, int F, int LW>
void launch_one(const DecimateArgs &a, const dim3 &grid, uint32_t quads_per_row, int dst_vec, hipStream_t s)
{
    hipLaunchKernelGGL((k_decimate<T, F, LW>), grid, dim3(DEC_BX, DEC_BY), 0, s, a, quads_per_row, dst_vec);
}

template <typename T, int F>
void launch_tf(const DecimateArgs &a, const dim3 &grid, uint32_t quads_per_row, int dst_vec, hipStream_t s)
{
    constexpr size_t SEG_BYTES = (size_t)DECIMATE_PX * F * sizeof(T);
    const size_t low = (uintptr_t)a.src | a.src_row_stride | (a.n_frames > 1 ? a.src_frame_stride : 0);
    if constexpr (SEG_BYTES % 16 == 0)
        if (low % 16 == 0) return launch_one<T, F, 16>(a, grid, quads_per_row, dst_vec, s);
    if constexpr (SEG_BYTES % 8 == 0)
        if (low % 8 == 0) return launch_one<T, F, 8>(a, grid, quads_per_row, dst_vec, s);
    if (low % 4 == 0) return launch_one<T, F, 4>(a, grid, quads_per_row, dst_vec, s);
    launch_one<T, F, 0>(a, grid, quads_per_row, dst_vec, s);
}

template <typename T>
void launch_t(const DecimateArgs &a, const dim3 &grid, uint32_t quads_per_row, int dst_vec, hipStream_t s)
{
    if (a.factor == 2) launch_tf<T, 2>(a, grid, quads_per_row, dst_vec, s);
    else if (a.factor == 3) launch_tf<T, 3>(a, grid, quads_per_row, dst_vec, s);
    else launch_tf<T, 4>(a, grid, quads_per_row, dst_vec, s);
}

template <typename T, int F>
void decimate_host_tf(const DecimateArgs &a)
{
    const uint32_t out_w = (uint32_t)decimate_out_w(a), out_h = (uint32_t)decimate_out_h(a);
    for (int f = 0; f < a.n_frames; ++f) {
        const unsigned char *frame = static_cast<const unsigned char *>(a.src) + (size_t)f * a.src_frame_stride;
        unsigned char *out = static_cast<unsigned char *>(a.dst) + (size_t)f * a.dst_frame_stride;
        for (uint32_t Y = 0; Y < out_h; ++Y) {
            T *d = reinterpret_cast<T *>(out + (size_t)Y * a.dst_row_stride);
            for (uint32_t X = 0; X < out_w; ++X) d[X] = (T)decimate_px<T, F>(frame, a.src_row_stride, X, Y);
        }
    }
}

template <typename T>
void decimate_host_t(const DecimateArgs &a)
{
    if (a.factor == 2) decimate_host_tf<T, 2>(a);
    else if (a.factor == 3) decimate_host_tf<T, 3>(a);
    else decimate_host_tf<T, 4>(a);
}

}  // namespace

const char *decimate_args_bad(const DecimateArgs &a)
{
    if (!a.src || !a.dst) return "a null batch";
    if (a.n_frames < 1 || a.n_frames > 65535) return "n_frames must be in 1 .. 65535";
    if (a.factor < DECIMATE_MIN_FACTOR || a.factor > DECIMATE_MAX_FACTOR) return "factor must be in 2 .. 4";
    if (a.src_w < a.factor || a.src_h < a.factor) return "width and height must be at least the factor";
    if (a.src_w > 65000 || a.src_h > 65000 || (long long)a.src_w * a.src_h >= (1ll << 30))
        return "the source's sides must be at most 65000 and its frame below 2^30 px";
    const size_t px = a.format == AGX_L16 ? 2 : 1;
    if (const char *bad = frames_bad(a.src, a.n_frames, a.src_w, a.src_h, a.src_row_stride, a.src_frame_stride, px)) return bad;
    if (const char *bad = frames_bad(a.dst, a.n_frames, decimate_out_w(a), decimate_out_h(a), a.dst_row_stride, a.dst_frame_stride, px)) return bad;
    return nullptr;
}

int launch_decimate(const DecimateArgs &a, void *stream)
{
    if (decimate_args_bad(a) || (a.format != AGX_L8 && a.format != AGX_L16)) return (int)hipErrorInvalidValue;
    const uint32_t out_w = (uint32_t)decimate_out_w(a), out_h = (uint32_t)decimate_out_h(a);
    const uint32_t quads_per_row = (out_w + DECIMATE_PX - 1) / DECIMATE_PX;
    const size_t quad_bytes = (size_t)DECIMATE_PX * (a.format == AGX_L16 ? 2 : 1);
    const int dst_vec = (((uintptr_t)a.dst | a.dst_row_stride | (a.n_frames > 1 ? a.dst_frame_stride : 0)) % quad_bytes) == 0;
    const dim3 grid((quads_per_row + DEC_BX - 1) / DEC_BX, (out_h + DEC_BY - 1) / DEC_BY, (unsigned)a.n_frames);  // y <= 16250
    if (a.format == AGX_L16) launch_t<uint16_t>(a, grid, quads_per_row, dst_vec, (hipStream_t)stream);
    else launch_t<uint8_t>(a, grid, quads_per_row, dst_vec, (hipStream_t)stream);
    return (int)hipGetLastError();
}

void decimate_host(const DecimateArgs &a)
{
    if (a.format == AGX_L16) decimate_host_t<uint16_t>(a);
    else decimate_host_t<uint8_t>(a);
}

}  // namespace agx
