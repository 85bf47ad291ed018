// decimate_math.h -- the arithmetic of agx_decimate_enqueue (k_decimate, decimate.hip) and agx_decimate_tail, written once for
// both: an output pixel is the mean of its F x F source pixels, in uint32, round half up.  No floating point.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define AGX_DECIMATE_HD __host__ __device__ __forceinline__
#else
#define AGX_DECIMATE_HD inline
#endif

namespace agx {

constexpr int DECIMATE_MIN_FACTOR = 2, DECIMATE_MAX_FACTOR = 4;

// (sum + F F / 2) / (F F): the sum of sixteen 16-bit pixels is below 2^20, so nothing wraps
template <int F>
AGX_DECIMATE_HD uint32_t decimate_mean(uint32_t sum)
{
    return (sum + (uint32_t)(F * F / 2)) / (uint32_t)(F * F);
}

// output pixel (X, Y) of a frame: T = uint8_t (AGX_L8) or uint16_t (AGX_L16); rows `row_stride` bytes apart
template <typename T, int F>
AGX_DECIMATE_HD uint32_t decimate_px(const unsigned char *frame, size_t row_stride, uint32_t X, uint32_t Y)
{
    uint32_t sum = 0;
    for (int dy = 0; dy < F; ++dy) {
        const T *row = reinterpret_cast<const T *>(frame + ((size_t)Y * F + (size_t)dy) * row_stride) + (size_t)X * F;
        for (int dx = 0; dx < F; ++dx) sum += row[dx];
    }
    return decimate_mean<F>(sum);
}

}  // namespace agx
