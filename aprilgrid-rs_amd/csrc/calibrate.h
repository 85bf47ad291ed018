// calibrate.h -- host-visible interface of k_calib_blocks and k_calib_solve (calibrate.hip): the camera's nine doubles and every
// usable frame's pose from a batch of tag tables, their poses, inlier masks and statuses (agx_calibrate_enqueue).  The arithmetic
// is calib_math.h's; calibrate_host.cpp's calibrate_host is the same on the host.  Internal to the library; the public boundary
// is include/aprilgrid_amd.h.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/aprilgrid_amd.h"

namespace agx {

constexpr int CALIB_FRAMES_PER_WG = 2;  // one wave per frame; two frames' staged rows fit the 64 KiB of static LDS

// All pointers are device pointers for the kernels, host pointers for the host form.
struct CalibArgs {
    int n_frames;                // 1 .. 65535
    const agx_tag *tags;         // [n_frames][tags_per_frame]
    uint32_t tags_per_frame;     // > 0
    const uint32_t *n_tags;      // [n_frames]
    const uint32_t *tag_status;  // [n_frames] or null: a word that is not AGX_TAGS_OK makes the frame unusable
    uint32_t cols, rows, first_id;  // rows * cols in 1 .. 4096
    float spacing_ratio;            // finite, > -1
    double tag_size;                // finite, > 0
    agx_camera camera;              // the seed: agx_board_pose_enqueue_m's rules under the lens model
    uint32_t fixed_mask;            // bit i holds camera double i
    double damping;                 // finite, >= 0
    uint32_t iterations;            // 0 .. 64
    uint32_t min_tags, min_frames;  // >= 1
    int flags;                      // AGX_CALIB_ACCEPT_LOOSE
    const double *pose_in;       // [n_frames][12]: agx_board_pose_enqueue_m's d_pose
    const uint32_t *row_status;  // [n_frames][tags_per_frame]: its d_row_status
    const uint32_t *fit_status;  // [n_frames]: its d_status
    double *camera_out;          // [9]
    double *pose;                // [n_frames][12], may be pose_in
    float *frame_cost;           // [n_frames]
    uint32_t *frame_n;           // [n_frames]
    agx_calib_report *report;
};

// the kernels' workspace, device memory of calib_work_bytes(n_frames) bytes (8-byte aligned), carved by calib_work()
struct CalibCtl;
struct CalibWork {
    CalibCtl *ctl;
    double *blocks;     // [n_frames][CALIB_BLOCK]
    double *pose_cur;   // [n_frames][12]: the current iterate's poses
    double *pose_best;  // [n_frames][12]: the best iterate's
    double *cost_best;  // [n_frames]: the frames' |e|^2 at the best iterate
    uint32_t *corners;  // [n_frames]: 4 x the frame's inlier rows, 0 for an unusable frame
    uint32_t *list;     // [n_frames]: the usable frames in frame order
};
size_t calib_work_bytes(int n_frames);
CalibWork calib_work(void *base, int n_frames);

// The rule that the record breaks under the lens model `lens`, or null.
const char *calib_args_bad(const CalibArgs &a, int lens);
// 2 (iterations + 1) + 1 launches on the stream, nothing returns to the host; hipError_t
int launch_calibrate(const CalibArgs &a, int lens, void *work, void *stream);
// the host form: the same bytes into host arrays
void calibrate_host(const CalibArgs &a, int lens);
// the closed-form seed (agx_calibrate_seed_tail) and the parameter Jacobian of n camera-frame points (agx_debug_calib_param_jacobian)
uint32_t calibrate_seed_host(const double *h, const uint32_t *fit_status, uint32_t n, int img_w, int img_h, double *camera_out);
void calib_param_jacobian_host(int lens, const agx_camera &camera, const double *xyz, uint32_t n, double *out);

}  // namespace agx
