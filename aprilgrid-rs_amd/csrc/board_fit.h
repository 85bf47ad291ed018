// board_fit.h -- host-visible interface of k_board_fit (board_fit.hip): the board-to-image homography through every frame's tag
// table, its outlier rounds and the predicted corners of the layout's tags (agx_board_fit_enqueue).  The arithmetic is
// board_fit_math.h's, the rounds are board_rounds.h's; host_tail.cpp's board_fit is the same on the host.  Internal to the
// library; the public boundary is include/aprilgrid_amd.h.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/aprilgrid_amd.h"

namespace agx {

constexpr int FIT_FRAMES_PER_WG = 2;  // one wave per frame; two frames' staged rows fit the 64 KiB of static LDS

// All pointers are device pointers for the kernel; the host form (board_fit) reads frame 0 of a record of host pointers.
struct BoardFitArgs {
    int n_frames;
    const agx_tag *tags;         // [n_frames][tags_per_frame]
    uint32_t tags_per_frame;     // > 0
    const uint32_t *n_tags;      // [n_frames]
    const uint32_t *tag_status;  // [n_frames] or null: a word that is not AGX_TAGS_OK makes the frame AGX_FIT_INPUT
    uint32_t cols, rows, first_id;  // rows * cols in 1 .. 4096
    float spacing_ratio;            // finite, > -1
    int img_w, img_h;               // > 0
    float max_err_sq;               // >= 0
    uint32_t max_drop, min_tags;    // min_tags >= 1
    int flags;                      // AGX_FIT_PREDICT_MISSING
    double *h;             // [n_frames][9]
    float *err_sq;         // [n_frames][tags_per_frame]
    uint32_t *row_status;  // [n_frames][tags_per_frame]: AGX_FIT_ROW_*
    uint32_t *n_inliers;   // [n_frames]
    float *rms;            // [n_frames]
    agx_tag *pred;         // [n_frames][rows * cols]
    uint32_t *n_pred;      // [n_frames]
    uint32_t *status;      // [n_frames]: AGX_FIT_*
};
// The rule that the record breaks, or null: every entry point's check and the launch's.  device: the kernel's record (n_frames and
// tags_per_frame > 0, tag_status may be null); else the host form's, whose tags, err_sq and row_status may be null while
// n_tags[0] == 0.  Arrays 4-byte aligned, h 8-byte; n_frames * tags_per_frame < 2^27.
const char *board_fit_args_bad(const BoardFitArgs &b, bool device);
// one wave per frame, FIT_FRAMES_PER_WG frames per workgroup; hipError_t
int launch_board_fit(const BoardFitArgs &b, void *stream);

}  // namespace agx
