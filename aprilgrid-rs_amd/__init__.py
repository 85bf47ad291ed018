"""aprilgrid-rs_amd -- MI355X-native AprilGrid saddle/tag detection path.

Host-side mirror of the Rust crate `aprilgrid` 0.8.0 (`aprilgrid::detector::TagDetector`,
`aprilgrid::TagFamily`, `DetectorParams`, `Saddle`) over the C ABI of
include/aprilgrid_amd.h.  All compute happens in libaprilgrid_amd.so (hand-written HIP for
gfx950 plus the C++ host tail); importing this package fails loudly if that library has not
been built -- there is no CPU fallback.
"""
from .detector import (DetectorGroup, DetectorParams, Saddle, TagDetector, TagFamily, AgxError, SADDLE_DTYPE, CLUSTER_DTYPE,
                       blur_weights, build_library, decode_quads_tail, find_board_tail, grow_board_tail, init_quads_tail, snap_points, library_path,
                       refine_constants, filter_saddles, collect_tags, decode_positions, bit_code, best_tag, tag_maps, board_fit, board_pose, Camera,
                       rectify_map, remap, decimate, rectified_points, render_boards, board_pose_looking_at, pose_rows,
                       calibrate, calibrate_seed, calib_report, calib_param_jacobian,
                       rig_calibrate, rig_seed, rig_report, rig_jacobian)

__all__ = ["DetectorGroup", "DetectorParams", "Saddle", "TagDetector", "TagFamily", "AgxError", "SADDLE_DTYPE", "CLUSTER_DTYPE",
           "blur_weights", "build_library", "decode_quads_tail", "find_board_tail", "grow_board_tail", "init_quads_tail", "snap_points", "library_path", "refine_constants",
           "filter_saddles", "collect_tags", "decode_positions", "bit_code", "best_tag", "tag_maps", "board_fit", "board_pose", "Camera",
           "rectify_map", "remap", "decimate", "rectified_points", "render_boards", "board_pose_looking_at", "pose_rows",
           "calibrate", "calibrate_seed", "calib_report", "calib_param_jacobian",
           "rig_calibrate", "rig_seed", "rig_report", "rig_jacobian"]
