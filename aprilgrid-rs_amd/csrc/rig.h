// rig.h -- host-visible interface of k_rig_blocks, k_rig_instants and k_rig_solve (rig.hip): the extrinsics of a rig of cameras
// and every usable instant's board pose from synchronised tag tables (agx_rig_calibrate_enqueue).  The arithmetic is rig_math.h's;
// rig_host.cpp's rig_calibrate_host is the same on the host.  Internal to the library; the public boundary is
// include/aprilgrid_amd.h.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/aprilgrid_amd.h"

namespace agx {

constexpr int RIG_FRAMES_PER_WG = 2;    // k_rig_blocks: one wave per frame; two frames' staged rows fit the static LDS
constexpr int RIG_INSTANTS_PER_WG = 4;  // k_rig_instants: one wave per instant

// All pointers are device pointers for the kernels, host pointers for the host form.  Frame f = c n_instants + s.
struct RigArgs {
    int n_cams, n_instants;      // 2 .. 8;  n_cams n_instants in 1 .. 65535
    const agx_tag *tags;         // [frames][tags_per_frame]
    uint32_t tags_per_frame;     // > 0
    const uint32_t *n_tags;      // [frames]
    const uint32_t *tag_status;  // [frames] or null
    uint32_t cols, rows, first_id;
    float spacing_ratio;
    double tag_size;
    int lens[8];                 // per camera
    agx_camera camera[8];        // per camera, the caller's nine (agx_board_pose_enqueue_m's rules)
    double damping;
    uint32_t iterations;
    uint32_t min_tags, min_cams, min_instants;
    int flags;                   // AGX_CALIB_ACCEPT_LOOSE
    const double *pose_in;       // [frames][12]
    const uint32_t *row_status;  // [frames][tags_per_frame]
    const uint32_t *fit_status;  // [frames]
    const double *ext_in;        // [n_cams][12], may be ext
    double *ext;                 // [n_cams][12]
    double *rig_pose;            // [n_instants][12]
    float *frame_cost;           // [frames]
    uint32_t *frame_n;           // [frames]
    uint32_t *cam_n;             // [n_cams]
    agx_rig_report *report;
};

// the kernels' workspace, device memory of rig_work_bytes() bytes (8-byte aligned), carved by rig_work()
struct RigCtl;
struct RigWork {
    RigCtl *ctl;
    double *frames;     // [frames][RIG_FRAME]: the frames' sums
    double *instants;   // [n_instants][rig_block_len(n_cams)]: the instants' contributions and back-substitution rows
    double *t_cur;      // [n_instants][12]: the current iterate's T_s
    double *t_best;     // [n_instants][12]: the best iterate's
    double *cost_best;  // [frames]: the frames' |e|^2 at the best iterate
    uint32_t *corners;  // [frames]: 4 x the frame's inlier rows, 0 for a frame that does not count
    uint32_t *inst_ok;  // [n_instants]: the instant is usable
    uint32_t *list;     // [n_instants]: the usable instants in instant order
};
size_t rig_work_bytes(int n_cams, int n_instants);
RigWork rig_work(void *base, int n_cams, int n_instants);

// The rule that the record breaks, or null.  host: the seed extrinsics are readable and must be finite.
const char *rig_args_bad(const RigArgs &a, bool host);
// 3 (iterations + 1) launches on the stream, nothing returns to the host; hipError_t
int launch_rig_calibrate(const RigArgs &a, void *work, void *stream);
// the host form: the same bytes into host arrays
void rig_calibrate_host(const RigArgs &a);
// the closed-form seed (agx_rig_seed_tail) and the residual's derivative for tests (agx_debug_rig_jacobian)
void rig_seed_host(int n_cams, int n_instants, const double *pose, const uint32_t *fit_status, const uint32_t *frame_n, double *ext_out, uint32_t *cam_status);
void rig_jacobian_host(int lens, const agx_camera &camera, const double *extrinsic, const double *rig_pose, const double *xy, uint32_t n, double *out);

}  // namespace agx
