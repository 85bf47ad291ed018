// tail_kernels.h -- host-visible interface of the device board search + tag decode (tail_kernels.hip).
// Internal to the library; the public boundary is include/aprilgrid_amd.h.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/aprilgrid_amd.h"
#include "chain_kernels.h"

namespace agx {

// Per-frame status word of the device tail (frame row [1]).
enum : uint32_t {
    TAIL_OK = 0u,
    TAIL_UNCERTAIN = 1u,  // an angle comparison fell inside the guard band of its threshold: only the host's own
                          // expression (libm's atan2f / cosf / sinf, as the reference) decides there -- the frame goes to the host tail
    TAIL_CAPACITY = 2u,   // more saddles / candidate quads / board cells / tags than the kernel's fixed lists hold: host tail
    TAIL_CHAIN = 4u       // the chain itself reported an overflow for the frame (no saddle list): reported as such
};

constexpr int TAIL_MAX_SADDLES = 1024;  // saddles of a frame the device tail takes (more: TAIL_CAPACITY)

struct TailArgs {
    // the chain's results of the batch (device): compact agx_saddle array + per-frame counters (n_out, out_offset, flags)
    const float *saddles;
    const FrameCounters *ctr;
    int n_frames;
    // u8 luma for the decode (to_luma8): rows luma_row_stride bytes apart, frames luma_frame_stride bytes apart
    const uint8_t *luma;
    long long luma_frame_stride;
    int luma_row_stride;
    int W, H;
    // TagDetector's family fields (src/detector.rs:17-23) and max_num_of_boards
    int edge, border, hamming, n_codes;
    const uint64_t *codes;  // device copy of the family's code list
    int max_boards;
    // results: tags[f][tag_stride] (at most tag_cap of them written: more is TAIL_CAPACITY), table[f] = {count, status,
    // ticks (100 MHz) the frame took, saddles | seeds << 16}
    agx_tag *tags;
    uint32_t *table;
    uint32_t tag_cap, tag_stride;
    // option "tail_debug_band" (tests of the hand-back path): a white-block angle within this many degrees of 60 / 120 is
    // reported undecided whatever the exact evaluation would say (0 = off: only the kernel's own guard band)
    float debug_band;
    int debug;  // AGX_TAIL_DEBUG >= 2 (and a build with -DAGX_TAIL_TIMERS): frame debug_frame's first wave prints where its time went (100 MHz ticks)
    int debug_frame;  // AGX_TAIL_DEBUG_FRAME (default 0)
};

// Enqueue the device tail of the batch on `stream`; hipError_t.
int launch_board_tail(const TailArgs &t, void *stream);
// agx_detect_batch_enqueue_to: the tail's rows and frame table (device memory, rows tag_stride apart) into the caller's layout,
// one wave per frame: d_tags[f][cap] (a frame's rows only), d_counts[f], d_status[f] (agx_status; AGX_ERR_STATE for a frame
// handed back to the host tail, which agx_detect_batch_fetch fills in); ctr = the chain's counters of the batch.  hipError_t.
int launch_publish_tags(const uint32_t *table, const agx_tag *tags, uint32_t tag_stride, const FrameCounters *ctr, int n_frames,
                        uint32_t cap, agx_tag *d_tags, uint32_t *d_counts, int *d_status, void *stream);
// agx_group_detect_enqueue: flags word of a packed frame table entry {count, offset, status, flags}
enum : uint32_t {
    PACK_HANDED_BACK = 1u,  // the device tail handed the frame back: count 0, AGX_ERR_STATE until the fetch has run the host tail
    PACK_UNCERTAIN = 2u,    // ... because of an angle inside its guard band (TAIL_UNCERTAIN)
    PACK_SLAB_FULL = 4u     // the frame's rows would cross the end of the slab: AGX_ERR_CAPACITY, the true count, no row
};
// The same inputs as launch_publish_tags, packed instead of laid out per frame: d_table[f] = {count, offset, status, flags}
// (16 bytes; status = the agx_status k_publish_tags reports), the rows of the AGX_OK frames back to back in frame order in
// d_slab[slab_records] -- offset = the exclusive prefix sum over the frames before f of the rows they hold (a frame that is not
// AGX_OK holds none).  A frame whose rows would end beyond slab_records is PACK_SLAB_FULL and still counts in the sum, so every
// frame behind it is too: the first overflow closes the slab, and a frame's offset depends only on the frames before it.
// d_table must be 16-byte aligned; n_frames <= 65535.  hipError_t.
int launch_pack_tags(const uint32_t *table, const agx_tag *tags, uint32_t tag_stride, const FrameCounters *ctr, int n_frames,
                     uint32_t cap, uint32_t *d_table, agx_tag *d_slab, uint32_t slab_records, void *stream);
// k_decode_quads (agx_decode_quads_enqueue): try_decode_quad (detector.rs:448-476) of caller-given quads on the frames' u8 luma.
// All pointers are device pointers.
struct DecodeQuadsArgs {
    const uint8_t *luma;  // to_luma8 of frame f at luma + f * luma_frame_stride, rows luma_row_stride bytes apart
    long long luma_frame_stride;
    int luma_row_stride;
    int W, H;
    int n_frames;
    int edge, border, hamming, n_codes;  // the family (src/detector.rs:17-23)
    const uint64_t *codes;               // its code list
    const uint8_t *quads;        // point p of slot s: two floats at quads + (s * 4 + p) * point_stride; slot = f * quads_per_frame + q
    uint32_t point_stride;       // bytes: a multiple of 4, >= 8
    uint32_t quads_per_frame;
    const uint32_t *counts;        // [n_frames] quads of frame f (capped at quads_per_frame), or null: quads_per_frame each
    const uint32_t *point_status;  // [slots * 4] AGX_POINT_* of every point, or null: a quad with a word != 0 is AGX_QUAD_SKIPPED
    agx_tag *tags;     // [slots]: {id, xy}; zeros unless AGX_QUAD_DECODED
    uint32_t *status;  // [slots]: AGX_QUAD_*
    uint64_t *bits;    // [slots] or null: bit_code's value (DECODED, NO_MATCH), else 0
};
// one row of 16 lanes per slot, grid-stride; n_frames * quads_per_frame < 2^31; hipError_t
int launch_decode_quads(const DecodeQuadsArgs &d, void *stream);
// k_find_boards (agx_find_boards_enqueue): one try_find_best_board (detector.rs:588-639) per frame over caller-given saddle
// slots -- k_board_tail's round up to its complete quad list, the quads out as slot numbers.  All pointers are device pointers.
struct FindBoardsArgs {
    const uint8_t *saddles;  // slot s: floats x, y, k, theta, phi at saddles + s * stride (k and phi are never read)
    uint32_t stride;         // bytes: a multiple of 4, >= 20
    int n_frames;
    uint32_t saddles_per_frame;   // frame f owns the slots from f * saddles_per_frame ...
    const uint32_t *counts;       // ... min(counts[f], saddles_per_frame) of them, or null: saddles_per_frame; or ...
    const uint32_t *frame_table;  // ... agx_frame_result[n_frames]: count slots from offset (status & 7: AGX_BOARD_INPUT, nothing read)
    const uint32_t *point_status;  // a word per slot (the batch's numbering), or null: only slots whose word is 0 enter the list
    uint32_t quads_per_frame;
    uint32_t *quads;      // [n_frames][quads_per_frame][4]: slot numbers WITHIN the frame; a frame's own rows only
    float *quad_points;   // [n_frames][quads_per_frame][4][2] or null: the corners' x, y
    uint32_t *n_quads;    // [n_frames]
    uint32_t *status;     // [n_frames]: AGX_BOARD_* (AGX_BOARD_PENDING: handed back, the host form answers)
    float debug_band;     // option "tail_debug_band", as TailArgs::debug_band
    int host_only;        // every frame is AGX_BOARD_PENDING and nothing is read (option "device_tail" 0, or refused)
};
// one workgroup per frame, k_board_tail's LDS; needs init_tail_kernels on the device; hipError_t
int launch_find_boards(const FindBoardsArgs &b, void *stream);
// k_grow_boards (agx_grow_boards_enqueue): per frame the boards of caller-given seed quads, Board::new (board.rs:26-48) at the
// caller's spacing_ratio, and the best of them out as k_find_boards writes its board.  The list and the results are
// FindBoardsArgs'; all pointers are device pointers.
struct GrowBoardsArgs : FindBoardsArgs {
    const uint32_t *seed_quads;   // [n_frames][seeds_per_frame][4]: slot numbers within the frame, init_quads' corner order
    uint32_t seeds_per_frame;     // > 0
    const uint32_t *seed_counts;  // [n_frames]: frame f has min(seed_counts[f], seeds_per_frame) seeds, or null: seeds_per_frame
    float spacing_ratio;          // finite, 1.0f + spacing_ratio > 0
    uint32_t stop_score;          // > 0: no seed is taken behind the first one that leaves the best score at or above it
    int flags;                    // AGX_GROW_FIX_MISSING
    uint32_t *seed_scores;        // [n_frames][seeds_per_frame] or null: the seeds' scores (0 behind the stop); FOUND / CAPACITY frames
    uint32_t *best_seed;          // [n_frames] or null: the chosen board's seed; FOUND / CAPACITY frames
};
// as launch_find_boards; n_frames * seeds_per_frame < 2^27; hipError_t
int launch_grow_boards(const GrowBoardsArgs &b, void *stream);
// k_init_quads (agx_init_quads_enqueue): per frame init_quads (detector.rs:543-586) of caller-given seed saddles -- or of
// try_find_best_board's own seeds (:601-616) -- over the same lists, the candidate quads of seed i behind those of seed i - 1.
// The list and quads / quad_points / n_quads / status are FindBoardsArgs'; all pointers are device pointers.
struct InitQuadsArgs : FindBoardsArgs {
    const uint32_t *seed_saddles;  // [n_frames][seeds_per_frame]: slot numbers within the frame, or null: the reference's seeds in pop order
    uint32_t seeds_per_frame;      // > 0; with seed_saddles null: at most this many of the reference's seeds
    const uint32_t *seed_counts;   // [n_frames]: frame f has min(seed_counts[f], seeds_per_frame) seeds, or null: seeds_per_frame
    uint32_t n_nearest;            // 2 .. 64: :550's 50
    uint32_t *seed_quad_counts;    // [n_frames][seeds_per_frame] or null: the quads of each seed (0 behind the frame's seeds); FOUND / NONE / CAPACITY frames
    uint32_t *seeds_out;           // [n_frames][seeds_per_frame] or null: the seeds taken (rows below n_seeds_out); FOUND / NONE / CAPACITY frames
    uint32_t *n_seeds_out;         // [n_frames] or null
};
// one workgroup per frame, an LDS layout of its own (100 656 bytes); n_frames * seeds_per_frame < 2^27; needs init_tail_kernels; hipError_t
int launch_init_quads(const InitQuadsArgs &b, void *stream);
// k_collect_tags (agx_collect_tags_enqueue): one round's bookkeeping of detect's loop (detector.rs:510-539) per frame -- the
// decoded quads of the round into the frame's tag table (detected_tags.insert, :520: a tag keeps the row of its first insertion and
// takes the corners of its last) and AGX_POINT_USED into the status words of their saddles (:521-536).  No pixels.  All pointers
// are device pointers; host_tail.cpp's collect_tags is the same round on the host.
struct CollectTagsArgs {
    int n_frames;
    uint32_t quads_per_frame;
    const uint32_t *quads;         // [n_frames][quads_per_frame][4]: slot numbers within the frame (k_find_boards' rows)
    const uint32_t *n_quads;       // [n_frames]
    const uint32_t *board_status;  // [n_frames]: AGX_BOARD_*
    const agx_tag *quad_tags;      // [n_frames * quads_per_frame] (k_decode_quads' rows)
    const uint32_t *quad_status;   // [n_frames * quads_per_frame]: AGX_QUAD_*
    uint32_t saddles_per_frame;    // frame f's words start at f * saddles_per_frame, saddles_per_frame of them; or ...
    const uint32_t *frame_table;   // ... agx_frame_result[n_frames]: `count` words from `offset`
    uint32_t *point_status;        // a word per slot, or null: nothing is marked
    uint32_t tags_per_frame;
    agx_tag *tags;         // [n_frames][tags_per_frame]: rows below the frame's count
    uint32_t *n_tags;      // [n_frames]
    uint32_t *tag_status;  // [n_frames]: AGX_TAGS_*
    int n_codes;           // the family's code count: a decoded id is below it
    int reset;             // != 0: every frame's table is empty (count 0, AGX_TAGS_OK) whatever the arrays hold
};
// one wave per frame; n_codes in 1 .. 640 (the LDS tables are indexed by id); hipError_t
int launch_collect_tags(const CollectTagsArgs &c, void *stream);
// k_snap_points (agx_snap_points_enqueue): per frame every caller point to the nearest listed saddle of the frame's list, and the
// rows whose points all snapped to pairwise distinct slots compacted in row order -- k_grow_boards' seed quads (4 points per row)
// or k_init_quads' seed saddles (1) as they stand.  The list is read as FindBoardsArgs' (x and y only).  All pointers are device
// pointers; host_tail.cpp's snap_points is the same on the host.
constexpr uint32_t SNAP_CHUNK = 1024;        // listed saddles staged in LDS at a time
constexpr uint32_t SNAP_ROWS_PER_WAVE = 4;   // rows one wave answers per pass: 16 lanes to a row, 4 to a point
struct SnapPointsArgs {
    const uint8_t *saddles;  // slot s: floats x, y at saddles + s * stride (k, theta and phi are never read)
    uint32_t stride;         // bytes: a multiple of 4, >= 20
    int n_frames;
    uint32_t saddles_per_frame;
    const uint32_t *counts;        // as FindBoardsArgs::counts
    const uint32_t *frame_table;   // as FindBoardsArgs::frame_table (status & 7: AGX_SNAP_INPUT, nothing read)
    const uint32_t *point_status;  // as FindBoardsArgs::point_status
    const uint8_t *points;         // point j of row r of frame f: two floats at points + (f * rows_per_frame + r) * row_stride + j * point_stride
    unsigned long long row_stride;  // bytes: a multiple of 4
    uint32_t point_stride;          // bytes: a multiple of 4, >= 8
    uint32_t rows_per_frame;        // > 0
    uint32_t points_per_row;        // 1 .. 4
    const uint32_t *row_counts;     // [n_frames]: frame f has min(row_counts[f], rows_per_frame) rows, or null: rows_per_frame
    float max_dist_sq;              // >= 0, +inf allowed: a point snaps if d2 <= max_dist_sq
    int flags;                      // AGX_SNAP_REVERSE
    uint32_t *slots;      // [n_frames][rows_per_frame][points_per_row]: the slot within the frame or AGX_SNAP_NONE, in stored order
    float *dist_sq;       // the same shape, or null: d2 to the nearest candidate, +inf where there is none
    uint32_t *rows;       // [n_frames][rows_per_frame][points_per_row]: the compacted rows
    uint32_t *n_rows;     // [n_frames]
    uint32_t *row_index;  // [n_frames][rows_per_frame] or null: the row a compacted row came from
    uint32_t *status;     // [n_frames]: AGX_SNAP_*
};
// one workgroup of four waves per frame; n_frames * rows_per_frame < 2^27; hipError_t
int launch_snap_points(const SnapPointsArgs &s, void *stream);
int init_tail_kernels();  // per-device kernel attributes (current device); hipError_t

}  // namespace agx
