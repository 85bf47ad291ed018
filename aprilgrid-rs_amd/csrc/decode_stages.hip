// decode_stages.hip -- the three stages of try_decode_quad (reference src/detector.rs:448-476) as kernels of their own, each
// with the arguments of the crate's pub fn it restates:
//   k_decode_positions   decode_positions (detector.rs:42-72): the sample points of every quad slot, stored
//   k_bit_code           bit_code (:74-122) over ANY list of up to 64 sample points per slot
//   k_best_tag           best_tag (:142-169) against ANY code list of up to 65535 codes
// and the sampling model opened (image_util.rs:5-37, :39-70):
//   k_positions_homography   decode_positions with tag_homography in tag_affine's place (agx_decode_positions_enqueue_m)
//   k_tag_maps               tag_affine / tag_homography themselves, a 3 x 3 matrix per slot (agx_tag_maps_enqueue)
// k_decode_quads (tail_kernels.hip) stays the fused form with the reference's constants; these three chained give its bytes
// (tests/test_gpu_decode_stages.py), and the two forms run the same code: the scalar arithmetic of decode_math.h (tag_affine,
// binary64 and rounded once, with `margin` where the fused kernel passes 0.5; f32::round; Rust's saturating `as u32`; the finite
// test), which the host tail runs too, and the lane-group sampler, rotation, code scan and tag store of decode_lanes.h.  The
// samples are h0*fx + h1*fy + h2*1.0f left to right in binary32 (-ffp-contract=off).
// Geometry of all three: a ROW of 16 lanes per slot, four slots per wave, 256 threads (16 slots at a time), grid-stride over the
// slots.  A row's lanes take every branch together, so the row-wide DPP reductions see all of their lanes.  Every store is a
// per-lane global store; slots at or beyond a frame's count are skipped before anything is read or written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "decode_lanes.h"
#include "decode_stages.h"

namespace agx {
namespace {

constexpr int DS_THREADS = 256;
constexpr unsigned DS_MAX_GRID = 2048;  // (256 CUs x 8 workgroups; the rest by the stride)

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
        if (slot_beyond_count(d.counts, slot, d.quads_per_frame)) continue;
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
                finite = finite && f32_finite(q[2 * p]) && f32_finite(q[2 * p + 1]);
                outside = outside || f32_as_u32(round_half_away(q[2 * p])) >= d.W || f32_as_u32(round_half_away(q[2 * p + 1])) >= d.H;  // :50-56
            }
            if (!finite || outside) {
                why = AGX_QUAD_OUTSIDE;
            } else {
                float aff[6];
                tag_affine(q, d.border * 2 + d.edge, d.margin, aff);
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

// ---- agx_decode_positions_enqueue_m at AGX_TAG_MAP_HOMOGRAPHY, agx_tag_maps_enqueue (image_util.rs:5-37, :39-70) ---------------
// The front of a slot as k_decode_positions has it: the point statuses, then the four corners -> AGX_QUAD_DECODED and q, or
// AGX_QUAD_SKIPPED / AGX_QUAD_OUTSIDE.  image: the corners are tested against W x H (:50-56) too.
__device__ __forceinline__ uint32_t slot_corners(const uint8_t *quads, uint32_t point_stride, const uint32_t *point_status, uint32_t slot, bool image,
                                                 uint32_t W, uint32_t H, float q[8])
{
    if (point_status) {
        const uint32_t *ps = point_status + (u64)slot * 4u;
        if ((ps[0] | ps[1] | ps[2] | ps[3]) != 0u) return AGX_QUAD_SKIPPED;  // (AGX_POINT_REFINED is 0)
    }
    const uint8_t *pts = quads + (u64)slot * 4u * (u64)point_stride;
    bool finite = true, outside = false;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const float *pp = reinterpret_cast<const float *>(pts + (size_t)p * point_stride);
        q[2 * p] = pp[0];
        q[2 * p + 1] = pp[1];
        finite = finite && f32_finite(q[2 * p]) && f32_finite(q[2 * p + 1]);
        outside = outside || (image && (f32_as_u32(round_half_away(q[2 * p])) >= W || f32_as_u32(round_half_away(q[2 * p + 1])) >= H));
    }
    return !finite || outside ? (uint32_t)AGX_QUAD_OUTSIDE : (uint32_t)AGX_QUAD_DECODED;
}

// k_decode_positions' scheme.  Every lane of the row evaluates the slot's map -- the closed form's three binary64 divisions
// included: the row's lanes issue together, so one lane evaluating for the others would take the wave the same time and add
// nine broadcasts.  A pass first decides the slot (every sample's w), the row's verdict by DPP, then a second pass stores.
__global__ void __launch_bounds__(DS_THREADS, 4) k_positions_homography(DecodePositionsArgs d)
{
    const int l = (int)(threadIdx.x & 15u);
    const uint32_t n_slots = (uint32_t)d.n_frames * d.quads_per_frame, step = gridDim.x * (DS_THREADS / 16);
    const int nb = d.edge * d.edge;
    for (uint32_t slot = blockIdx.x * (DS_THREADS / 16) + (threadIdx.x >> 4); slot < n_slots; slot += step) {
        if (slot_beyond_count(d.counts, slot, d.quads_per_frame)) continue;
        float q[8], h[9];
        uint32_t why = slot_corners(d.quads, d.point_stride, d.point_status, slot, true, d.W, d.H, q);
        if (why == AGX_QUAD_DECODED && !tag_homography(q, d.border * 2 + d.edge, d.margin, h)) why = AGX_QUAD_DEGENERATE;
        if (why == AGX_QUAD_DECODED) {  // (the row alike: its lanes read the same corners)
            uint32_t bad = 0;
            for (int n = l; n < nb; n += 16)
                if (!homography_w_ok(homography_w(h, (float)(d.border + n / d.edge), (float)(d.border + n % d.edge)))) bad = 1;
            if (lanes_reduce<16>(bad, u_or)) {
                why = AGX_QUAD_OUTSIDE;
            } else {
                float *out = d.points + (u64)slot * (u64)(2 * nb);
                for (int n = l; n < nb; n += 16) {  // the reference's order: x outer, y inner
                    const float fx = (float)(d.border + n / d.edge), fy = (float)(d.border + n % d.edge);
                    float px, py;
                    homography_point(h, fx, fy, homography_w(h, fx, fy), px, py);
                    out[2 * n] = px;
                    out[2 * n + 1] = py;
                }
            }
        }
        if (l == 0) d.status[slot] = why;
    }
}

// tag_affine / tag_homography of every slot: lanes 0 .. 8 store the nine words of the slot's matrix (36 consecutive bytes), lane
// 9 the status.  No image size: neither function takes one.
__global__ void __launch_bounds__(DS_THREADS, 4) k_tag_maps(TagMapsArgs t)
{
    const int l = (int)(threadIdx.x & 15u);
    const uint32_t n_slots = (uint32_t)t.n_frames * t.quads_per_frame, step = gridDim.x * (DS_THREADS / 16);
    for (uint32_t slot = blockIdx.x * (DS_THREADS / 16) + (threadIdx.x >> 4); slot < n_slots; slot += step) {
        if (slot_beyond_count(t.counts, slot, t.quads_per_frame)) continue;
        float q[8], h[9];
        uint32_t why = slot_corners(t.quads, t.point_stride, t.point_status, slot, false, 0u, 0u, q);
        if (why == AGX_QUAD_DECODED) {
            if (t.model == AGX_TAG_MAP_HOMOGRAPHY) {
                if (!tag_homography(q, t.side_bits, t.margin, h)) why = AGX_QUAD_DEGENERATE;
            } else {
                tag_affine(q, t.side_bits, t.margin, h);
                h[6] = 0.0f;
                h[7] = 0.0f;
                h[8] = 1.0f;
            }
        }
        if (why == AGX_QUAD_DECODED && l < 9) {
            float v = h[0];  // (no register array is indexed by the lane)
#pragma unroll
            for (int j = 1; j < 9; ++j) v = l == j ? h[j] : v;
            t.maps[(u64)slot * 9u + (u64)l] = v;
        }
        if (l == 9) t.status[slot] = why;
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
        if (slot_beyond_count(a.counts, slot, a.quads_per_frame)) continue;
        uint32_t why = a.status_in ? a.status_in[slot] : (uint32_t)AGX_QUAD_DECODED;  // (read before the word is written: they may be one array)
        u64 bits = 0;
        if (why == AGX_QUAD_DECODED) {
            const float *pp = a.points + (u64)slot * (u64)(2 * nb);
            const uint8_t *luma = a.luma + (long long)(slot / a.quads_per_frame) * a.luma_frame_stride;
            // a coordinate that is not finite is outside (the project's rule, as for a quad's corners); :84-93
            const auto point = [&](int n, float &px, float &py) {
                px = pp[2 * n];
                py = pp[2 * n + 1];
                return f32_finite(px) && f32_finite(py);
            };
            why = (uint32_t)bit_code_lanes<16, 4>(luma, w, h, a.luma_row_stride, l, nb, a.threshold, a.max_invalid, false, point, bits);
            if (why != AGX_QUAD_DECODED) bits = 0;
        }
        if (l == 0) a.status[slot] = why;
        else if (l == 1) a.bits[slot] = bits;
    }
}

// ---- agx_best_tag_enqueue: best_tag (detector.rs:142-169) ------------------------------------------------------------------------
// The row's one scan for the four rotations with (distance << 16 | index) keys (best_tag_scan: the launcher admits at most 65535
// codes), then the rotations in the reference's order (pick_rotation).  LDS: a list of at most BT_LDS_CODES codes is staged once
// per workgroup (5120 bytes, k_decode_quads' table); a longer one is read where it lies -- every row reads all of it, from L2
// after the first.
template <bool LDS>
__global__ void __launch_bounds__(DS_THREADS, 4) k_best_tag(BestTagArgs t)
{
    const uint64_t *codes = t.codes;
    if constexpr (LDS) {
        __shared__ uint64_t lds_codes[BT_LDS_CODES];
        for (uint32_t i = threadIdx.x; i < t.n_codes && i < (uint32_t)BT_LDS_CODES; i += DS_THREADS) lds_codes[i] = t.codes[i];
        __syncthreads();
        codes = lds_codes;
    }
    const int l = (int)(threadIdx.x & 15u);
    const uint32_t step = gridDim.x * (DS_THREADS / 16);  // (the launcher: n_slots < 2^31, at most 2048 workgroups)
    for (uint32_t slot = blockIdx.x * (DS_THREADS / 16) + (threadIdx.x >> 4); slot < t.n_slots; slot += step) {
        if (slot_beyond_count(t.counts, slot, t.quads_per_frame)) continue;
        uint32_t why = t.status_in ? t.status_in[slot] : (uint32_t)AGX_QUAD_DECODED;  // (read before the word is written)
        int id = 0, rot = 0;
        if (why == AGX_QUAD_DECODED) {
            uint32_t ms[4];
            best_tag_scan(codes, (int)t.n_codes, t.bits[slot], t.edge, l, ms);
            if (!pick_rotation(ms, t.thres, id, rot)) why = AGX_QUAD_NO_MATCH;
        }
        const bool hit = why == AGX_QUAD_DECODED;
        if (l == 0) {
            t.status[slot] = why;
        } else if (l == 1) {
            t.ids[slot] = (uint32_t)id;
        } else if (l == 2) {
            t.rotations[slot] = (uint32_t)rot;
        } else if (l < 12 && t.tags) {  // lanes 3 .. 11: the nine words of the slot's agx_tag, k_decode_quads' record
            const uint8_t *pts = t.quads + (u64)slot * 4u * (u64)t.point_stride;
            reinterpret_cast<uint32_t *>(t.tags + slot)[l - 3] = tag_word(l - 3, hit, id, rot, pts, t.point_stride);
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

int launch_positions_homography(const DecodePositionsArgs &p, void *stream)
{
    const unsigned long long n_slots = (unsigned long long)(p.n_frames > 0 ? p.n_frames : 0) * p.quads_per_frame;
    if (!n_slots || n_slots >= (1ull << 31) || !p.quads || !p.points || !p.status || p.point_stride < 8 || (p.point_stride & 3) || p.edge < 1 ||
        p.edge > 8 || p.border < 0 || p.border > 16)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_positions_homography, dim3(ds_grid(n_slots)), dim3(DS_THREADS), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

int launch_tag_maps(const TagMapsArgs &p, void *stream)
{
    const unsigned long long n_slots = (unsigned long long)(p.n_frames > 0 ? p.n_frames : 0) * p.quads_per_frame;
    if (!n_slots || n_slots >= (1ull << 31) || !p.quads || !p.maps || !p.status || p.point_stride < 8 || (p.point_stride & 3) || p.side_bits < 1 ||
        p.side_bits > 40 || (p.model != AGX_TAG_MAP_AFFINE && p.model != AGX_TAG_MAP_HOMOGRAPHY))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tag_maps, dim3(ds_grid(n_slots)), dim3(DS_THREADS), 0, (hipStream_t)stream, p);
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
