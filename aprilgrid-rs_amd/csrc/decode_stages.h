// decode_stages.h -- host-visible interface of the decode's three stages as kernels of their own (decode_stages.hip):
// decode_positions (detector.rs:42-72), bit_code (:74-122) and best_tag (:142-169) with the crate's own arguments, on the
// slots k_decode_quads answers in one launch.  Internal to the library; the public boundary is include/aprilgrid_amd.h.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/aprilgrid_amd.h"

namespace agx {

constexpr int BT_LDS_CODES = 640;  // a code list up to this long is staged in LDS (k_decode_quads' table); a longer one is read from L2

// k_decode_positions (agx_decode_positions_enqueue).  All pointers are device pointers.
struct DecodePositionsArgs {
    const uint8_t *quads;          // point p of slot s: two floats at quads + (s * 4 + p) * point_stride; slot = f * quads_per_frame + q
    uint32_t point_stride;         // bytes: a multiple of 4, >= 8
    int n_frames;
    uint32_t quads_per_frame;
    const uint32_t *counts;        // [n_frames] or null, as DecodeQuadsArgs::counts
    const uint32_t *point_status;  // [slots * 4] or null: a quad with a word != 0 is AGX_QUAD_SKIPPED
    uint32_t W, H;                 // decode_positions' img_w, img_h: no pixel is read
    int border, edge;              // border_bits 0 .. 16, edge_bits 1 .. 8
    float margin;
    float *points;     // [slots][edge * edge][2]: x outer, y inner; written for AGX_QUAD_DECODED slots only
    uint32_t *status;  // [slots]: AGX_QUAD_DECODED, _OUTSIDE or _SKIPPED
};
// one row of 16 lanes per slot, grid-stride; n_frames * quads_per_frame < 2^31; hipError_t
int launch_decode_positions(const DecodePositionsArgs &p, void *stream);
// k_positions_homography (agx_decode_positions_enqueue_m at AGX_TAG_MAP_HOMOGRAPHY): the same arguments, the samples through
// tag_homography (image_util.rs:5-37); status also AGX_QUAD_DEGENERATE, and AGX_QUAD_OUTSIDE for a sample whose w is not > 0
int launch_positions_homography(const DecodePositionsArgs &p, void *stream);

// k_tag_maps (agx_tag_maps_enqueue): tag_affine / tag_homography themselves.  All pointers are device pointers.
struct TagMapsArgs {
    const uint8_t *quads;  // as DecodePositionsArgs
    uint32_t point_stride;
    int n_frames;
    uint32_t quads_per_frame;
    const uint32_t *counts;
    const uint32_t *point_status;
    int side_bits;  // 1 .. 40
    float margin;
    int model;         // AGX_TAG_MAP_*
    float *maps;       // [slots][9] row-major 3 x 3; written for AGX_QUAD_DECODED slots only
    uint32_t *status;  // [slots]: AGX_QUAD_DECODED, _OUTSIDE (a corner that is not finite), _SKIPPED or _DEGENERATE
};
int launch_tag_maps(const TagMapsArgs &p, void *stream);

// k_bit_code (agx_bit_code_enqueue).  All pointers are device pointers.
struct BitCodeArgs {
    const uint8_t *luma;  // to_luma8 of frame f at luma + f * luma_frame_stride, rows luma_row_stride bytes apart
    long long luma_frame_stride;
    int luma_row_stride;
    int W, H;
    int n_frames;
    const float *points;       // [slots][points_per_slot][2]
    uint32_t points_per_slot;  // 1 .. 64
    uint32_t quads_per_frame;
    const uint32_t *counts;     // [n_frames] or null
    const uint32_t *status_in;  // [slots] or null (may be `status`): a slot whose word is != 0 reads nothing and keeps the word
    int threshold;              // valid_brightness_threshold, 0 .. 255
    uint32_t max_invalid;       // max_invalid_bit
    uint64_t *bits;    // [slots]: bit_code's value, 0 unless AGX_QUAD_DECODED
    uint32_t *status;  // [slots]: AGX_QUAD_DECODED, _OUTSIDE, _LOW_CONTRAST, _AMBIGUOUS, or status_in's word
};
int launch_bit_code(const BitCodeArgs &b, void *stream);

// k_best_tag (agx_best_tag_enqueue).  All pointers are device pointers.
struct BestTagArgs {
    const uint64_t *bits;  // [n_slots]
    uint32_t n_slots;
    uint32_t quads_per_frame;   // with counts: slot s belongs to frame s / quads_per_frame
    const uint32_t *counts;     // or null: every slot
    const uint32_t *status_in;  // [n_slots] or null (may be `status`)
    uint32_t thres;             // 0 .. 255: a rotation matches at a distance below it
    const uint64_t *codes;
    uint32_t n_codes;  // 1 .. 65535
    int edge;          // 1 .. 8
    const uint8_t *quads;   // the corners the tags are made of (with `tags`), or null
    uint32_t point_stride;
    uint32_t *ids, *rotations;  // [n_slots]: 0 unless AGX_QUAD_DECODED
    uint32_t *status;           // [n_slots]: AGX_QUAD_DECODED, _NO_MATCH, or status_in's word
    agx_tag *tags;              // [n_slots] or null: k_decode_quads' record
};
int launch_best_tag(const BestTagArgs &t, void *stream);

}  // namespace agx
