// decode_stages.hip -- the three stages of try_decode_quad (reference src/detector.rs:448-476) as kernels of their own, each
// with the arguments of the crate's pub fn it restates:
//   k_decode_positions   decode_positions (detector.rs:42-72): the sample points of every quad slot, stored
//   k_bit_code           bit_code (:74-122) over ANY list of up to 64 sample points per slot
//   k_best_tag           best_tag (:142-169) against ANY code list of up to 65535 codes
// k_decode_quads (tail_kernels.hip) stays the fused form with the reference's constants; these three chained give its bytes
// (tests/test_gpu_decode_stages.py).  The arithmetic is the project's: tag_affine is the closed form of host_tail.cpp (binary64,
// rounded once) with `margin` where the fused kernel has 0.5, the samples are h0*fx + h1*fy + h2*1.0f left to right in binary32
// (-ffp-contract=off), roundings are f32::round and Rust's saturating `as u32`.
// Geometry of all three: a ROW of 16 lanes per slot, four slots per wave, 256 threads (16 slots at a time), grid-stride over the
// slots.  A row's lanes take every branch together, so the row-wide DPP reductions see all of their lanes.  Every store is a
// per-lane global store; slots at or beyond a frame's count are skipped before anything is read or written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "decode_stages.h"

namespace agx {
namespace {

using u64 = uint64_t;
constexpr int DS_THREADS = 256;
constexpr unsigned DS_MAX_GRID = 2048;  // (256 CUs x 8 workgroups; the rest by the stride)

__device__ __forceinline__ bool ds_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ float ds_round(float x)  // f32::round
{
    if (!(fabsf(x) < 8388608.0f)) return x;
    float t = (float)(int32_t)x;
    const float d = x - t;
    if (d >= 0.5f) t += 1.0f;
    else if (d <= -0.5f) t -= 1.0f;
    return t;
}
__device__ __forceinline__ uint32_t ds_as_u32(float v)  // Rust `as u32`
{
    if (!(v > 0.0f)) return 0u;
    if (v >= 4294967296.0f) return 0xffffffffu;
    return (uint32_t)v;
}
template <int CTRL>
__device__ __forceinline__ uint32_t ds_dpp(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xf, 0xf, false);
}
// reduction over the lane's row of 16, in every lane of the row (DPP: no LDS crossbar)
template <typename F>
__device__ __forceinline__ uint32_t ds_row_reduce(uint32_t v, F f)
{
    v = f(v, ds_dpp<0xB1>(v));      // quad_perm [1, 0, 3, 2]
    v = f(v, ds_dpp<0x4E>(v));      // quad_perm [2, 3, 0, 1]
    v = f(v, ds_dpp<0x141>(v));     // row_half_mirror
    return f(v, ds_dpp<0x140>(v));  // row_mirror
}
__device__ __forceinline__ uint32_t ds_min(uint32_t x, uint32_t y) { return x < y ? x : y; }
__device__ __forceinline__ uint32_t ds_max(uint32_t x, uint32_t y) { return x > y ? x : y; }
__device__ __forceinline__ uint32_t ds_or(uint32_t x, uint32_t y) { return x | y; }
__device__ __forceinline__ uint32_t ds_add(uint32_t x, uint32_t y) { return x + y; }

// the frame's count says the slot does not exist (a count above quads_per_frame: every slot of the frame does)
__device__ __forceinline__ bool ds_beyond_count(const uint32_t *counts, uint32_t slot, uint32_t quads_per_frame)
{
    if (!counts) return false;
    const uint32_t f = slot / quads_per_frame;
    return slot - f * quads_per_frame >= counts[f];
}

// ---- agx_decode_positions_enqueue: decode_positions (detector.rs:42-72) ----------------------------------------------------------
// Every lane of the row evaluates the slot's affine (a few dozen binary64 operations) and stores the samples l, l + 16, ...: the
// row's stores of a pass are 128 consecutive bytes.  No pixel is read.  256 threads, no LDS.
__global__ void __launch_bounds__(DS_THREADS, 4) k_decode_positions(DecodePositionsArgs d)
{
    const int l = (int)(threadIdx.x & 15u);
    // (the launcher: n_slots < 2^31 and at most 2048 workgroups, so neither the product nor slot + step wraps)
    const uint32_t n_slots = (uint32_t)d.n_frames * d.quads_per_frame, step = gridDim.x * (DS_THREADS / 16);
    const int nb = d.edge * d.edge;
    for (uint32_t slot = blockIdx.x * (DS_THREADS / 16) + (threadIdx.x >> 4); slot < n_slots; slot += step) {
        if (ds_beyond_count(d.counts, slot, d.quads_per_frame)) continue;
        const uint8_t *pts = d.quads + (u64)slot * 4u * (u64)d.point_stride;
        uint32_t why = AGX_QUAD_DECODED;
        if (d.point_status) {
            const uint32_t *ps = d.point_status + (u64)slot * 4u;
            if ((ps[0] | ps[1] | ps[2] | ps[3]) != 0u) why = AGX_QUAD_SKIPPED;  // (AGX_POINT_REFINED is 0)
        }
        if (why == AGX_QUAD_DECODED) {
            float q[8];
            bool finite = true, outside = false;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const float *pp = reinterpret_cast<const float *>(pts + (size_t)p * d.point_stride);
                q[2 * p] = pp[0];
                q[2 * p + 1] = pp[1];
                finite = finite && ds_finite(q[2 * p]) && ds_finite(q[2 * p + 1]);
                outside = outside || ds_as_u32(ds_round(q[2 * p])) >= d.W || ds_as_u32(ds_round(q[2 * p + 1])) >= d.H;  // :50-56
            }
            if (!finite || outside) {
                why = AGX_QUAD_OUTSIDE;
            } else {
                // tag_affine: least squares over the corners of an axis-aligned square, in binary64, rounded once (host_tail.cpp)
                float aff[6];
                const int side_bits = d.border * 2 + d.edge;
                const double S = (double)((float)side_bits - 1.0f + d.margin), m = (double)d.margin;
                const double cc = 0.5 * (S - m), aa = 0.5 * (S + m);
                const double su[4] = {-aa, -aa, aa, aa}, sv[4] = {-aa, aa, aa, -aa};
#pragma unroll
                for (int axis = 0; axis < 2; ++axis) {
                    double gu = 0, gv = 0, mean = 0;
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const double t = q[2 * p + axis];
                        gu += su[p] * t;
                        gv += sv[p] * t;
                        mean += t;
                    }
                    const double hu = gu / (4.0 * aa * aa), hv = gv / (4.0 * aa * aa);
                    aff[3 * axis + 0] = (float)hu;
                    aff[3 * axis + 1] = (float)hv;
                    aff[3 * axis + 2] = (float)(mean / 4.0 - hu * cc - hv * cc);
                }
                float *out = d.points + (u64)slot * (u64)(2 * nb);
                for (int n = l; n < nb; n += 16) {  // the reference's order: x outer, y inner
                    const float fx = (float)(d.border + n / d.edge), fy = (float)(d.border + n % d.edge);
                    out[2 * n] = aff[0] * fx + aff[1] * fy + aff[2] * 1.0f;
                    out[2 * n + 1] = aff[3] * fx + aff[4] * fy + aff[5] * 1.0f;
                }
            }
        }
        if (l == 0) d.status[slot] = why;
    }
}

// ---- agx_bit_code_enqueue: bit_code (detector.rs:74-122) -------------------------------------------------------------------------
// SIXTEEN lanes per slot: lane l takes the samples l, l + 16, l + 32, l + 48 of the up to 64, its four loads side by side; min, max,
// the outside flag, the invalid count and the two halves of the bits are reduced over the row by DPP (quad_bits8_why's scheme at
// twice the width).  A sample outside the image ends the reference's loop with None: here it is remembered and the coordinates
// are clamped, so every load is inside the frame.  256 threads, no LDS.
__global__ void __launch_bounds__(DS_THREADS, 4) k_bit_code(BitCodeArgs a)
{
    const int l = (int)(threadIdx.x & 15u);
    const uint32_t n_slots = (uint32_t)a.n_frames * a.quads_per_frame, step = gridDim.x * (DS_THREADS / 16);
    const uint32_t w = (uint32_t)a.W, h = (uint32_t)a.H;
    const int nb = (int)a.points_per_slot;
    for (uint32_t slot = blockIdx.x * (DS_THREADS / 16) + (threadIdx.x >> 4); slot < n_slots; slot += step) {
        if (ds_beyond_count(a.counts, slot, a.quads_per_frame)) continue;
        uint32_t why = a.status_in ? a.status_in[slot] : (uint32_t)AGX_QUAD_DECODED;  // (read before the word is written: they may be one array)
        u64 bits = 0;
        if (why == AGX_QUAD_DECODED) {
            const float *pp = a.points + (u64)slot * (u64)(2 * nb);
            const uint8_t *luma = a.luma + (long long)(slot / a.quads_per_frame) * a.luma_frame_stride;
            bool outside = false;
            int lo = 255, hi = 0;
            int vals[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int n = l + 16 * k;
                const bool valid = n < nb;
                const int nn = valid ? n : 0;
                const float px = pp[2 * nn], py = pp[2 * nn + 1];
                uint32_t ix = ds_as_u32(ds_round(px)), iy = ds_as_u32(ds_round(py));
                // a coordinate that is not finite is outside (the project's rule, as for a quad's corners); :84-93
                outside = outside || (valid && (!ds_finite(px) || !ds_finite(py) || ix >= w || iy >= h));
                ix = ix < w ? ix : w - 1;
                iy = iy < h ? iy : h - 1;
                const int b = luma[(size_t)iy * (size_t)a.luma_row_stride + ix];
                vals[k] = valid ? b : -1;
                lo = valid && b < lo ? b : lo;
                hi = valid && b > hi ? b : hi;
            }
            lo = (int)ds_row_reduce((uint32_t)lo, ds_min);
            hi = (int)ds_row_reduce((uint32_t)hi, ds_max);
            outside = ds_row_reduce(outside ? 1u : 0u, ds_or) != 0u;
            if (outside) {
                why = AGX_QUAD_OUTSIDE;  // (the sixteen alike)
            } else if (hi - lo < 50) {
                why = AGX_QUAD_LOW_CONTRAST;  // :97-99
            } else {
                const int mid = (int)(uint8_t)ds_as_u32(ds_round(((float)lo + (float)hi) / 2.0f));  // :100
                uint32_t invalid = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (vals[k] >= 0) {  // the first sample is the most significant bit
                        const int b = vals[k], dd = mid - b;
                        if ((dd < 0 ? -dd : dd) < a.threshold) ++invalid;
                        if (b > mid) bits |= 1ull << (nb - 1 - (l + 16 * k));
                    }
                invalid = ds_row_reduce(invalid, ds_add);
                bits = (u64)ds_row_reduce((uint32_t)(bits >> 32), ds_or) << 32 | ds_row_reduce((uint32_t)bits, ds_or);
                if (invalid > a.max_invalid) {  // :117-118
                    why = AGX_QUAD_AMBIGUOUS;
                    bits = 0;
                }
            }
        }
        if (l == 0) a.status[slot] = why;
        else if (l == 1) a.bits[slot] = bits;
    }
}

// ---- agx_best_tag_enqueue: best_tag (detector.rs:142-169) ------------------------------------------------------------------------
// rotate_bits (detector.rs:124-140) by a row of 16 lanes: output bit `count` is input bit r + c * edge with
// count = (edge - 1 - r) * edge + c; every lane sets the output bits l, l + 16, l + 32, l + 48.  Only the low edge * edge bits
// survive a rotation, as in the reference.
__device__ __forceinline__ u64 ds_rotate_bits_row(u64 bits, int edge, int l)
{
    u64 out = 0;
    for (int count = l; count < edge * edge; count += 16) {
        const int r = edge - 1 - count / edge, cc = count % edge;
        out |= ((bits >> (r + cc * edge)) & 1ull) << count;
    }
    return (u64)ds_row_reduce((uint32_t)(out >> 32), ds_or) << 32 | ds_row_reduce((uint32_t)out, ds_or);
}

// The reference scans the list once per rotation until one matches; here ONE scan serves the four rotations (every lane takes
// every 16th code; per rotation the first code with the smallest distance = the smallest (distance << 16 | index) key: a
// distance is at most 64 and the launcher admits at most 65535 codes), then the rotations are looked at in the reference's order.
// The XOR of rotation 0 counts all 64 bits of `bits`.  LDS: a list of at most BT_LDS_CODES codes is staged once per workgroup (5120
// bytes, k_decode_quads' table); a longer one is read where it lies -- every row reads all of it, from L2 after the first.
template <bool LDS>
__global__ void __launch_bounds__(DS_THREADS, 4) k_best_tag(BestTagArgs t)
{
    const u64 *codes = t.codes;
    if constexpr (LDS) {
        __shared__ u64 lds_codes[BT_LDS_CODES];
        for (uint32_t i = threadIdx.x; i < t.n_codes && i < (uint32_t)BT_LDS_CODES; i += DS_THREADS) lds_codes[i] = t.codes[i];
        __syncthreads();
        codes = lds_codes;
    }
    const int l = (int)(threadIdx.x & 15u);
    const uint32_t step = gridDim.x * (DS_THREADS / 16);  // (the launcher: n_slots < 2^31, at most 2048 workgroups)
    for (uint32_t slot = blockIdx.x * (DS_THREADS / 16) + (threadIdx.x >> 4); slot < t.n_slots; slot += step) {
        if (ds_beyond_count(t.counts, slot, t.quads_per_frame)) continue;
        uint32_t why = t.status_in ? t.status_in[slot] : (uint32_t)AGX_QUAD_DECODED;  // (read before the word is written)
        uint32_t id = 0, rot = 0;
        if (why == AGX_QUAD_DECODED) {
            const u64 b0 = t.bits[slot], b1 = ds_rotate_bits_row(b0, t.edge, l), b2 = ds_rotate_bits_row(b1, t.edge, l),
                      b3 = ds_rotate_bits_row(b2, t.edge, l);
            uint32_t m0 = 0xffffffffu, m1 = 0xffffffffu, m2 = 0xffffffffu, m3 = 0xffffffffu;
#pragma unroll 2
            for (uint32_t i = (uint32_t)l; i < t.n_codes; i += 16u) {
                const u64 code = codes[i];
                m0 = ds_min(m0, (uint32_t)__popcll(code ^ b0) << 16 | i);
                m1 = ds_min(m1, (uint32_t)__popcll(code ^ b1) << 16 | i);
                m2 = ds_min(m2, (uint32_t)__popcll(code ^ b2) << 16 | i);
                m3 = ds_min(m3, (uint32_t)__popcll(code ^ b3) << 16 | i);
            }
            const uint32_t ms[4] = {ds_row_reduce(m0, ds_min), ds_row_reduce(m1, ds_min), ds_row_reduce(m2, ds_min), ds_row_reduce(m3, ds_min)};
            why = AGX_QUAD_NO_MATCH;
#pragma unroll
            for (int rotated = 3; rotated >= 0; --rotated)  // (descending: the first rotation that matches is the one kept)
                if ((ms[rotated] >> 16) < t.thres) {
                    id = ms[rotated] & 0xffffu;
                    rot = (uint32_t)rotated;
                    why = AGX_QUAD_DECODED;
                }
        }
        const bool hit = why == AGX_QUAD_DECODED;
        if (l == 0) {
            t.status[slot] = why;
        } else if (l == 1) {
            t.ids[slot] = id;
        } else if (l == 2) {
            t.rotations[slot] = rot;
        } else if (l < 12 && t.tags) {  // lanes 3 .. 11: the nine words of the slot's agx_tag, k_decode_quads' record
            const int j = l - 3;
            uint32_t wd = 0;
            if (hit) {
                if (j == 0) {
                    wd = id;
                } else {  // rotate_left(rot) then reverse, :468-469
                    const int i = (j - 1) >> 1, c = (j - 1) & 1, src = ((3 - i) + (int)rot) & 3;
                    wd = reinterpret_cast<const uint32_t *>(t.quads + ((u64)slot * 4u + (u64)src) * (u64)t.point_stride)[c];
                }
            }
            reinterpret_cast<uint32_t *>(t.tags + slot)[j] = wd;
        }
    }
}

unsigned ds_grid(unsigned long long n_slots)
{
    const unsigned long long per_wg = DS_THREADS / 16;
    return (unsigned)std::min<unsigned long long>((n_slots + per_wg - 1) / per_wg, (unsigned long long)DS_MAX_GRID);
}

}  // namespace

int launch_decode_positions(const DecodePositionsArgs &p, void *stream)
{
    const unsigned long long n_slots = (unsigned long long)(p.n_frames > 0 ? p.n_frames : 0) * p.quads_per_frame;
    if (!n_slots || n_slots >= (1ull << 31) || !p.quads || !p.points || !p.status || p.point_stride < 8 || (p.point_stride & 3) || p.edge < 1 ||
        p.edge > 8 || p.border < 0 || p.border > 16)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_decode_positions, dim3(ds_grid(n_slots)), dim3(DS_THREADS), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

int launch_bit_code(const BitCodeArgs &b, void *stream)
{
    const unsigned long long n_slots = (unsigned long long)(b.n_frames > 0 ? b.n_frames : 0) * b.quads_per_frame;
    if (!n_slots || n_slots >= (1ull << 31) || !b.luma || !b.points || !b.bits || !b.status || b.points_per_slot < 1 || b.points_per_slot > 64 ||
        b.W < 1 || b.H < 1)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bit_code, dim3(ds_grid(n_slots)), dim3(DS_THREADS), 0, (hipStream_t)stream, b);
    return (int)hipGetLastError();
}

int launch_best_tag(const BestTagArgs &t, void *stream)
{
    if (!t.n_slots || t.n_slots >= (1u << 31) || !t.bits || !t.codes || t.n_codes < 1 || t.n_codes > 65535 || t.edge < 1 || t.edge > 8 || !t.ids ||
        !t.rotations || !t.status || (t.counts && !t.quads_per_frame) || (t.tags && (!t.quads || t.point_stride < 8 || (t.point_stride & 3))))
        return (int)hipErrorInvalidValue;
    if (t.n_codes <= (uint32_t)BT_LDS_CODES) hipLaunchKernelGGL(k_best_tag<true>, dim3(ds_grid(t.n_slots)), dim3(DS_THREADS), 0, (hipStream_t)stream, t);
    else hipLaunchKernelGGL(k_best_tag<false>, dim3(ds_grid(t.n_slots)), dim3(DS_THREADS), 0, (hipStream_t)stream, t);
    return (int)hipGetLastError();
}

}  // namespace agx
