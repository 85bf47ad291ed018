// board_pose.h -- host-visible interface of k_board_pose (board_pose.hip): the board's pose under a lens model through every
// frame's tag table, its outlier rounds and the predicted corners of the layout's tags (agx_board_pose_enqueue).  The arithmetic
// is board_pose_math.h's, the rounds are board_rounds.h's; host_tail.cpp's board_pose is the same on the host.  Internal to the
// library; the public boundary is include/aprilgrid_amd.h.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/aprilgrid_amd.h"

namespace agx {

constexpr int POSE_FRAMES_PER_WG = 2;  // one wave per frame; two frames' staged rows fit the 64 KiB of static LDS

// All pointers are device pointers for the kernel; the host form (board_pose) reads frame 0 of a record of host pointers.
struct BoardPoseArgs {
    int n_frames;
    const agx_tag *tags;         // [n_frames][tags_per_frame]
    uint32_t tags_per_frame;     // > 0
    const uint32_t *n_tags;      // [n_frames]
    const uint32_t *tag_status;  // [n_frames] or null: a word that is not AGX_TAGS_OK makes the frame AGX_FIT_INPUT
    uint32_t cols, rows, first_id;  // rows * cols in 1 .. 4096
    float spacing_ratio;            // finite, > -1
    double tag_size;                // finite, > 0
    agx_camera camera;              // every field finite, fx and fy > 0; under AGX_LENS_EQUIDISTANT fx fy cx cy k1 k2 k3 k4 0,
                                    // under AGX_LENS_DOUBLE_SPHERE fx fy cx cy xi alpha 0 0 0 (the launch puts w2 into the ninth)
    float max_err_sq;               // >= 0
    uint32_t max_drop, min_tags;    // min_tags >= 1
    uint32_t iterations;            // 0 .. 64
    int flags;                      // AGX_FIT_PREDICT_MISSING
    double *pose;          // [n_frames][12]: R row major, then t
    float *err_sq;         // [n_frames][tags_per_frame]
    uint32_t *row_status;  // [n_frames][tags_per_frame]: AGX_FIT_ROW_*
    uint32_t *n_inliers;   // [n_frames]
    float *rms;            // [n_frames]
    uint32_t *best_iter;   // [n_frames]
    agx_tag *pred;         // [n_frames][rows * cols]
    uint32_t *n_pred;      // [n_frames]
    uint32_t *status;      // [n_frames]: AGX_FIT_*
};
// The rule that the record breaks under the lens model `lens`, or null: board_fit_args_bad's rules with pose and best_iter for h,
// and pose_args_ok (board_pose_math.h) for the camera (the caller's, before pose_camera()), tag_size and iterations.
const char *board_pose_args_bad(const BoardPoseArgs &b, int lens, bool device);
// one wave per frame, POSE_FRAMES_PER_WG frames per workgroup; lens: AGX_LENS_*, which picks the kernel's
// instantiation; b.camera is the caller's; hipError_t
int launch_board_pose(const BoardPoseArgs &b, int lens, void *stream);

}  // namespace agx
