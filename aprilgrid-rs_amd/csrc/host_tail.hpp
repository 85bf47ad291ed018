// host_tail.hpp -- the irregular tail of TagDetector::detect that stays on the host:
// board search (reference src/detector.rs:543-639, src/board.rs, src/saddle.rs:17-67) and tag
// decode (src/detector.rs:42-169,448-476, src/image_util.rs:39-70).
#pragma once
#include <array>
#include <functional>
#include <cstdint>
#include <vector>

#include "../../include/aprilgrid_amd.h"
#include "board_fit.h"
#include "board_pose.h"

namespace agx {

struct FamilyInfo {
    int edge, border, hamming;
    const uint64_t *codes;
    int n_codes;
};

// TagDetector::new's table, src/detector.rs:369-405.  Returns false for an unknown family.
bool family_info(int family, FamilyInfo &out);

using Quad = std::array<int, 4>;

// math_util.rs:15-33
float theta_distance_degree(float t0, float t1);
float angle_degree(float v0x, float v0y, float v1x, float v1y);
// test hook: angle_degree next to the bounded approximation the board search decides with outside
// its guard bands (has_approx 0: the approximation is not used for these operands); v = n x 4 floats
// (coarse / has_coarse, optional: the cheaper first-level approximation and where it is used)
void debug_angle_pairs(const float *v, size_t n, float *exact, float *approx, uint8_t *has_approx, float *coarse = nullptr,
                       uint8_t *has_coarse = nullptr);
// this process's atan2f against libm_f32.h's restatement of glibc's routine on n pseudo-random operand pairs + the special
// cases: the number of disagreements (the device tail is offered only where it is 0)
uint64_t libm_atan2f_mismatches(uint64_t n, uint64_t seed);
// test hook: the white-block angle as the reference evaluates it and as the device tail's binary64 evaluation does (t = n x (theta, v02x, v02y))
void debug_white_block_angles(const float *t, size_t n, float *reference, double *binary64);
// saddle.rs:17-67
bool is_valid_quad(const agx_saddle &s0, const agx_saddle &d0, const agx_saddle &s1, const agx_saddle &d1);

// Workers for the board search of ONE frame (option "tail_threads"; agx_detect_batch parallelises over
// frames instead).  run(n, f) calls f(task) for task = 0..n-1 on the workers and returns when all are done.
struct TailWorkers {
    virtual ~TailWorkers() {}
    virtual int size() const = 0;
    virtual void run(int n, const std::function<void(int)> &f) = 0;
};

// detector.rs:588-639: quads (saddle indices) of the best board, or false (None).  With workers, the
// seeds are taken in waves of size() in the reference's order and merged in that order, so the board
// chosen is the one the sequential loop chooses.
bool try_find_best_board(const std::vector<agx_saddle> &refined, std::vector<Quad> &quads, TailWorkers *workers = nullptr);

// The host form of agx_find_boards_enqueue / agx_find_board_tail: one try_find_best_board (detector.rs:588-639) over the slots
// of one frame (floats x, y, k, theta, phi every `stride` bytes) that point_status admits (null: all; else a word per slot, 0 =
// listed).  AGX_BOARD_INPUT (a listed x, y or theta that is not finite), AGX_BOARD_NONE or AGX_BOARD_FOUND with the quads as SLOT
// numbers, four per quad, in all_tag_indexes' order.
int find_board_in_slots(const void *slots, size_t stride, uint32_t n_slots, const uint32_t *point_status, std::vector<uint32_t> &quads);

// Boards from the caller's seed quads: try_find_best_board's loop (:613-629) over `seeds` (indices into `listed`, taken as they
// are: Board::new does not test them) instead of init_quads' quads, with Board::new (board.rs:26-48) at spacing_ratio.  The
// board is the first seed whose score is strictly above every earlier one (:622); with stop_score > 0 the loop ends behind the
// first seed that leaves the best score at or above it (the seeds behind it: score 0).  try_fix_missing only with fix_missing.
// AGX_BOARD_NONE (no seed, or an empty list) or AGX_BOARD_FOUND with the quads in all_tag_indexes' order.
int grow_boards(const std::vector<agx_saddle> &listed, const std::vector<Quad> &seeds, float spacing_ratio, uint32_t stop_score, bool fix_missing,
                std::vector<Quad> &quads, std::vector<uint32_t> &seed_scores, uint32_t &best_seed);
// The host form of agx_grow_boards_enqueue / agx_grow_board_tail over the slots of one frame, as find_board_in_slots: seed_quads
// [n_seeds][4] and the quads are SLOT numbers.  AGX_BOARD_INPUT (a listed x, y or theta that is not finite; else a seed naming a
// slot at or beyond n_slots or one that is not listed -- every seed is looked at first), AGX_BOARD_NONE, AGX_BOARD_FOUND.
int grow_boards_in_slots(const void *slots, size_t stride, uint32_t n_slots, const uint32_t *point_status, const uint32_t *seed_quads,
                         uint32_t n_seeds, float spacing_ratio, uint32_t stop_score, int flags, std::vector<uint32_t> &quads,
                         std::vector<uint32_t> &seed_scores, uint32_t &best_seed);
// The host form of agx_init_quads_enqueue / agx_init_quads_tail over the slots of one frame, as find_board_in_slots: init_quads
// (detector.rs:543-586) with n_nearest (2 .. 64) in place of :550's 50 for the first min(n_seeds, max_seeds) of seed_saddles (SLOT
// numbers) or, with seed_saddles null, for try_find_best_board's own seeds (:601-616), the first max_seeds in pop order.  quads:
// SLOT numbers, four per quad, seed after seed in init_quads' order; seed_quad_counts [max_seeds] (0 behind the seeds taken) and
// seeds_out (the seeds taken) are filled unless the answer is AGX_BOARD_INPUT (as grow_boards_in_slots'; every seed is looked at
// first).  AGX_BOARD_NONE (an empty list, no seed, no quad) or AGX_BOARD_FOUND else.
int init_quads_in_slots(const void *slots, size_t stride, uint32_t n_slots, const uint32_t *point_status, const uint32_t *seed_saddles,
                        uint32_t n_seeds, uint32_t max_seeds, uint32_t n_nearest, std::vector<uint32_t> &quads,
                        std::vector<uint32_t> &seed_quad_counts, std::vector<uint32_t> &seeds_out);

// (tag_affine, image_util.rs:39-70, is decode_math.h's: the decode kernels run the same definition)
// detector.rs:124-140, 142-169
uint64_t rotate_bits(uint64_t bits, int edge_bits);
bool best_tag(uint64_t bits, int thres, const uint64_t *codes, int n_codes, int edge_bits, int &idx, int &rot);

// The stages decode_quad below is made of, with the crate's own arguments (agx_decode_positions_tail / agx_bit_code_tail;
// k_decode_positions and k_bit_code are the device forms):
// decode_positions, detector.rs:42-72: AGX_QUAD_OUTSIDE (None), or AGX_QUAD_DECODED and the edge * edge points (x, y) in pts, x
// outer and y inner.  The corners are finite (the callers' rule) and the source square is not degenerate.
int decode_positions(uint32_t w, uint32_t h, const float quad_xy[8], int border, int edge, float margin, float *pts);
// the same with tag_homography (image_util.rs:5-37) in tag_affine's place (agx_decode_positions_tail_m; k_positions_homography is
// the device form): also AGX_QUAD_DEGENERATE (no map), and AGX_QUAD_OUTSIDE for a sample whose w is not > 0 or not finite
int decode_positions_homography(uint32_t w, uint32_t h, const float quad_xy[8], int border, int edge, float margin, float *pts);
// bit_code, detector.rs:74-122, over n <= 64 points: AGX_QUAD_DECODED and the bits (first point = most significant of the n), or
// AGX_QUAD_OUTSIDE / _LOW_CONTRAST / _AMBIGUOUS in the reference's order, bits 0
int bit_code(const uint8_t *luma8, uint32_t w, uint32_t h, size_t stride, const float *pts, int n, int valid_brightness_threshold,
             uint32_t max_invalid_bit, uint64_t &bits);

// try_decode_quad, detector.rs:448-476, of one quad (x, y of its four corners) on the u8 luma plane: AGX_QUAD_DECODED with the
// code's index and the corners after rotate_left(rotation); reverse() (:467-470), or the reason for None (AGX_QUAD_OUTSIDE,
// _LOW_CONTRAST, _AMBIGUOUS, _NO_MATCH); bits = bit_code's value before any rotation (DECODED and NO_MATCH; else 0).
// tag_id and corners are written only for AGX_QUAD_DECODED.
int decode_quad(const FamilyInfo &fam, const uint8_t *luma8, uint32_t w, uint32_t h, size_t stride, const float quad_xy[8],
                int &tag_id, float corners[8], uint64_t &bits);

// detector.rs:510-539: board search + decode over a saddle list and the u8 luma plane.
// Tags in first-insertion order; a repeated id replaces the earlier corners.
void detect_tail(const FamilyInfo &fam, int max_num_of_boards, std::vector<agx_saddle> refined,
                 const uint8_t *luma8, int width, int height, size_t row_stride, std::vector<agx_tag> &tags,
                 TailWorkers *workers = nullptr);

// The same for a pool thread of agx_detect_batch: the list is copied into the calling thread's scratch, the tags are
// returned in it (valid until the thread's next tail) -- no allocation once the thread has seen a frame of that size.
const std::vector<agx_tag> &detect_tail_scratch(const FamilyInfo &fam, int max_num_of_boards, const agx_saddle *saddles, size_t n_saddles,
                                                const uint8_t *luma8, int width, int height, size_t row_stride);

// image 0.25.9 to_luma8 (call site detector.rs:507)
int luma8(const void *pixels, int width, int height, size_t row_stride, int format, uint8_t *out);

// The k / phi filter of refined_saddle_points (detector.rs:432-445) over n records and their status words, in place: the words
// that are AGX_POINT_REFINED and whose record fails become AGX_POINT_FILTERED (agx_filter_saddles_tail; k_filter_saddles is
// the device form)
void filter_saddles(const agx_params &params, const agx_saddle *records, uint32_t *status, uint32_t n);

// One round of detect's loop behind its board search and decode (detector.rs:510-539) for one frame: the round's decoded quads
// into the tag table (:520; a tag keeps the row of its first insertion and takes the corners of its last) and AGX_POINT_USED into
// the words of their saddles (:521-536; point_status may be null).  *n_tags / *tag_status (AGX_TAGS_*) in and out; a status that
// is not AGX_TAGS_OK is sticky.  n_codes = the family's code count.  (agx_collect_tags_tail; k_collect_tags is the device form)
void collect_tags(int n_codes, uint32_t n_quads, const uint32_t *quads, uint32_t board_status, const agx_tag *quad_tags,
                  const uint32_t *quad_status, uint32_t n_slots, uint32_t *point_status, uint32_t tag_cap, agx_tag *tags,
                  uint32_t *n_tags, uint32_t *tag_status);

// Caller points to the nearest listed saddle of one frame's slots (agx_snap_points_tail; k_snap_points is the device form): row r
// of n_rows has points_per_row (1 .. 4) points, point j two floats at points + r * row_stride + j * point_stride, read back to
// front under AGX_SNAP_REVERSE.  d2 = dx*dx + dy*dy in binary32 (squared_euclidean's fold); the nearest is the smallest d2 below
// +inf, at equal d2 the lowest slot; it is taken if d2 <= max_dist_sq.  out_slots / dist_sq (may be null) [n_rows][points_per_row]
// in the order read; rows / row_index (may be null): the rows whose points all snapped to pairwise distinct slots, compacted.
// -> AGX_SNAP_INPUT (a listed x or y that is not finite: only *n_rows_out = 0 is written) or AGX_SNAP_OK.
uint32_t snap_points(const void *slots, size_t stride, uint32_t n_slots, const uint32_t *point_status, const void *points, size_t row_stride,
                     size_t point_stride, uint32_t n_rows, uint32_t points_per_row, float max_dist_sq, int flags, uint32_t *out_slots,
                     float *dist_sq, uint32_t *rows, uint32_t *n_rows_out, uint32_t *row_index);

// The board-to-image homography through one frame's tag table, its outlier rounds and the predicted corners of the layout's tags
// (agx_board_fit_tail; k_board_fit is the device form, board_fit_math.h the arithmetic and the order of summation of both,
// board_rounds.h the rounds).  b is the kernel's record with host pointers, of which frame 0 is read and written (n_frames is 1;
// a null tag_status is AGX_TAGS_OK).  -> AGX_FIT_*, which is not stored; for AGX_FIT_FEW, _SINGULAR and _INPUT only
// n_inliers[0] = n_pred[0] = 0 is written.
uint32_t board_fit(const BoardFitArgs &b);

// The board's pose under the lens model `lens` (AGX_LENS_*, checked by the caller) likewise (agx_board_pose_tail; k_board_pose is
// the device form, board_pose_math.h the arithmetic).  b.camera is the caller's.  iter_sums [iterations + 1] or null: the sum of
// |e|^2 of every iterate of the last round, NaN for an iterate that was not reached (agx_debug_board_pose_sums).
uint32_t board_pose(const BoardPoseArgs &b, int lens, double *iter_sums);
// board_pose_math.h's pose_atan of r [n] as this compiler gives it (agx_debug_pose_atan), and its pose_project of n camera-frame
// points xyz [n][3] under the identity pose moved to each point's Z (agx_debug_pose_project): uv [n][2], NaN where Z is not > 0.
void pose_atan_host(const double *r, uint32_t n, double *out);
void pose_project_host(int lens, const agx_camera &cam, const double *xyz, uint32_t n, double *uv);

}  // namespace agx
