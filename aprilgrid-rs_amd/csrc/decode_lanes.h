// decode_lanes.h -- the tag decode by groups of 8 or 16 lanes (reference src/detector.rs:74-169, 448-476), device only: what the
// fused form (tail_kernels.hip: k_board_tail, k_decode_quads) and the staged form (decode_stages.hip: k_bit_code, k_best_tag)
// both run, so that the staged kernels give the fused kernel's bytes by construction.  The scalar arithmetic is decode_math.h.
// A group's lanes take every branch together, so the DPP reductions see all of their lanes.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/aprilgrid_amd.h"
#include "decode_math.h"

namespace agx {

typedef unsigned long long u64;

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xf, 0xf, false);
}
// reduction over the lane's aligned group of N = 4, 8 or 16 lanes (a quad, half a row, a row), in every lane of the group (DPP:
// no LDS crossbar)
template <int N, typename F>
__device__ __forceinline__ uint32_t lanes_reduce(uint32_t v, F f)
{
    static_assert(N == 4 || N == 8 || N == 16, "a quad, half a row or a row");
    v = f(v, dpp_u<0xB1>(v));                          // quad_perm [1, 0, 3, 2]
    v = f(v, dpp_u<0x4E>(v));                          // quad_perm [2, 3, 0, 1]
    if constexpr (N >= 8) v = f(v, dpp_u<0x141>(v));   // row_half_mirror
    if constexpr (N >= 16) v = f(v, dpp_u<0x140>(v));  // row_mirror
    return v;
}
__device__ __forceinline__ uint32_t u_min(uint32_t x, uint32_t y) { return y < x ? y : x; }
__device__ __forceinline__ uint32_t u_max(uint32_t x, uint32_t y) { return x > y ? x : y; }
__device__ __forceinline__ uint32_t u_or(uint32_t x, uint32_t y) { return x | y; }
__device__ __forceinline__ uint32_t u_add(uint32_t x, uint32_t y) { return x + y; }

// the frame's count says the slot does not exist (a count above quads_per_frame: every slot of the frame does)
__device__ __forceinline__ bool slot_beyond_count(const uint32_t *counts, uint32_t slot, uint32_t quads_per_frame)
{
    if (!counts) return false;
    const uint32_t f = slot / quads_per_frame;
    return slot - f * quads_per_frame >= counts[f];
}

// bit_code (detector.rs:74-122) of nb <= LANES * PASSES samples by a group of LANES lanes: lane `sub` of the group takes the
// samples sub, sub + LANES, ..., their loads side by side; point(n, px, py) gives sample n's coordinates and whether they may be
// used at all.  A sample outside the image ends the reference's loop with None: here it is remembered (as `outside` is, which
// the caller may bring along) and the coordinates are clamped, so every load is inside the frame.  -> AGX_QUAD_DECODED (0) and
// the bits in every lane of the group (the first sample is the most significant of the nb), else the reason for None in the
// order the reference meets them (AGX_QUAD_OUTSIDE, _LOW_CONTRAST, _AMBIGUOUS), bits_out untouched
template <int LANES, int PASSES, typename P>
__device__ __forceinline__ int bit_code_lanes(const uint8_t *luma, uint32_t w, uint32_t h, int pitch, int sub, int nb, int threshold,
                                              uint32_t max_invalid, bool outside, P point, u64 &bits_out)
{
    int lo = 255, hi = 0;
    int vals[PASSES];
#pragma unroll
    for (int k = 0; k < PASSES; ++k) {
        const int n = sub + LANES * k;
        const bool valid = n < nb;
        float px, py;
        const bool ok = point(valid ? n : 0, px, py);
        uint32_t ix = f32_as_u32(round_half_away(px)), iy = f32_as_u32(round_half_away(py));
        outside = outside || (valid && (!ok || ix >= w || iy >= h));
        ix = ix < w ? ix : w - 1;
        iy = iy < h ? iy : h - 1;
        const int b = luma[(size_t)iy * (size_t)pitch + ix];
        vals[k] = valid ? b : -1;
        lo = valid && b < lo ? b : lo;
        hi = valid && b > hi ? b : hi;
    }
    lo = (int)lanes_reduce<LANES>((uint32_t)lo, u_min);
    hi = (int)lanes_reduce<LANES>((uint32_t)hi, u_max);
    outside = lanes_reduce<LANES>(outside ? 1u : 0u, u_or) != 0;
    if (outside) return AGX_QUAD_OUTSIDE;  // (the group alike)
    if (hi - lo < 50) return AGX_QUAD_LOW_CONTRAST;
    const int mid = (int)(uint8_t)f32_as_u32(round_half_away(((float)lo + (float)hi) / 2.0f));
    u64 bits = 0;
    uint32_t invalid = 0;
#pragma unroll
    for (int k = 0; k < PASSES; ++k)
        if (vals[k] >= 0) {  // the first sample is the most significant bit
            const int b = vals[k], d = mid - b;
            if ((d < 0 ? -d : d) < threshold) ++invalid;
            if (b > mid) bits |= 1ull << (nb - 1 - (sub + LANES * k));
        }
    invalid = lanes_reduce<LANES>(invalid, u_add);
    if (invalid > max_invalid) return AGX_QUAD_AMBIGUOUS;
    bits_out = (u64)lanes_reduce<LANES>((uint32_t)(bits >> 32), u_or) << 32 | lanes_reduce<LANES>((uint32_t)bits, u_or);
    return AGX_QUAD_DECODED;
}

// rotate_bits (detector.rs:124-140) by a row of 16 lanes: output bit `count` is input bit r + c * edge with
// count = (edge - 1 - r) * edge + c; every lane sets the output bits l, l + 16, l + 32, l + 48.  Only the low edge * edge bits
// survive a rotation, as in the reference.
__device__ __forceinline__ u64 rotate_bits_row(u64 bits, int edge, int l)
{
    u64 out = 0;
    for (int count = l; count < edge * edge; count += 16) {
        const int r = edge - 1 - count / edge, cc = count % edge;
        out |= ((bits >> (r + cc * edge)) & 1ull) << count;
    }
    return (u64)lanes_reduce<16>((uint32_t)(out >> 32), u_or) << 32 | lanes_reduce<16>((uint32_t)out, u_or);
}

// best_tag (detector.rs:142-169) by a row of 16 lanes.  The reference scans the list once per rotation until one matches; here
// ONE scan serves the four rotations (every lane takes every 16th code; per rotation the first code with the smallest distance =
// the smallest (distance << 16 | index) key: a distance is at most 64 and a list has at most 65535 codes) -> ms[rotation], in
// every lane of the row.  The XOR of rotation 0 counts all 64 bits of b0.
template <typename C>  // (a 64-bit unsigned type: the kernels' u64, the argument structs' uint64_t)
__device__ __forceinline__ void best_tag_scan(const C *codes, int n_codes, u64 b0, int edge, int l, uint32_t ms[4])
{
    static_assert(sizeof(C) == 8, "a code is 64 bits");
    const u64 b1 = rotate_bits_row(b0, edge, l), b2 = rotate_bits_row(b1, edge, l), b3 = rotate_bits_row(b2, edge, l);
    uint32_t m0 = 0xffffffffu, m1 = 0xffffffffu, m2 = 0xffffffffu, m3 = 0xffffffffu;
#pragma unroll 2
    for (int i = l; i < n_codes; i += 16) {
        const u64 code = codes[i];
        const uint32_t k0 = (uint32_t)__popcll(code ^ b0) << 16 | (uint32_t)i, k1 = (uint32_t)__popcll(code ^ b1) << 16 | (uint32_t)i;
        const uint32_t k2 = (uint32_t)__popcll(code ^ b2) << 16 | (uint32_t)i, k3 = (uint32_t)__popcll(code ^ b3) << 16 | (uint32_t)i;
        m0 = k0 < m0 ? k0 : m0;
        m1 = k1 < m1 ? k1 : m1;
        m2 = k2 < m2 ? k2 : m2;
        m3 = k3 < m3 ? k3 : m3;
    }
    ms[0] = lanes_reduce<16>(m0, u_min);
    ms[1] = lanes_reduce<16>(m1, u_min);
    ms[2] = lanes_reduce<16>(m2, u_min);
    ms[3] = lanes_reduce<16>(m3, u_min);
}
// ... then the rotations are looked at in the reference's order: the first whose best distance is below thres -- the reference's
// (index, rotation); false = None
__device__ __forceinline__ bool pick_rotation(const uint32_t ms[4], uint32_t thres, int &idx, int &rot)
{
#pragma unroll
    for (int rotated = 0; rotated < 4; ++rotated)
        if ((ms[rotated] >> 16) < thres) {
            idx = (int)(ms[rotated] & 0xffffu);
            rot = rotated;
            return true;
        }
    return false;
}

// word j = 0 .. 8 of a slot's agx_tag: the id, then the corners after rotate_left(rot) and reverse (:468-469), read from the
// slot's four points (pts, point_stride bytes apart) in their rotated order -- no register array is indexed by the rotation;
// zeros unless the quad decoded
__device__ __forceinline__ uint32_t tag_word(int j, bool hit, int id, int rot, const uint8_t *pts, uint32_t point_stride)
{
    if (!hit) return 0u;
    if (j == 0) return (uint32_t)id;
    const int i = (j - 1) >> 1, c = (j - 1) & 1, src = ((3 - i) + rot) & 3;
    return reinterpret_cast<const uint32_t *>(pts + (size_t)src * point_stride)[c];
}

}  // namespace agx
