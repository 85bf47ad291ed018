"""ctypes declarations of include/aprilgrid_amd.h (one-to-one)."""
import ctypes as C
import os
import subprocess

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG_DIR, "libaprilgrid_amd.so")

AGX_OK = 0
AGX_ERR_ARG, AGX_ERR_FORMAT, AGX_ERR_CAPACITY, AGX_ERR_HIP = -1, -2, -3, -4
AGX_ERR_NO_DEVICE, AGX_ERR_FAMILY, AGX_ERR_STATE, AGX_ERR_NOMEM = -5, -6, -7, -8
AGX_L8, AGX_L16, AGX_RGB8, AGX_LF32 = 0, 1, 2, 3
AGX_LA8, AGX_RGBA8, AGX_BGR8, AGX_BGRA8, AGX_RGB8P, AGX_LA16, AGX_RGB16, AGX_RGBA16 = 4, 5, 6, 7, 8, 9, 10, 11
# agx_format -> (bytes between adjacent pixels of a row, rows per frame as a multiple of the height, numpy dtype of a channel)
FORMAT_LAYOUT = {AGX_L8: (1, 1, "u1"), AGX_L16: (2, 1, "u2"), AGX_RGB8: (3, 1, "u1"), AGX_LF32: (4, 1, "f4"),
                 AGX_LA8: (2, 1, "u1"), AGX_RGBA8: (4, 1, "u1"), AGX_BGR8: (3, 1, "u1"), AGX_BGRA8: (4, 1, "u1"),
                 AGX_RGB8P: (1, 3, "u1"), AGX_LA16: (4, 1, "u2"), AGX_RGB16: (6, 1, "u2"), AGX_RGBA16: (8, 1, "u2")}
AGX_GATHER_RCCL, AGX_GATHER_PEER = 0, 1
# rochade_refine of caller-given points (src/detector.rs:194-361): the status of a point, and which plane is refined on
AGX_POINT_REFINED, AGX_POINT_OUTSIDE, AGX_POINT_NOT_SADDLE, AGX_POINT_MOVED = 0, 1, 2, 3
AGX_REFINE_BLURRED, AGX_REFINE_PLANE = 0, 1
# try_decode_quad of caller-given quads (src/detector.rs:448-476): what became of a quad
AGX_QUAD_DECODED, AGX_QUAD_OUTSIDE, AGX_QUAD_LOW_CONTRAST, AGX_QUAD_AMBIGUOUS, AGX_QUAD_NO_MATCH, AGX_QUAD_SKIPPED = 0, 1, 2, 3, 4, 5
# the sampling model of decode_positions (src/image_util.rs:39-70 tag_affine, :5-37 tag_homography); the homography's refusal
AGX_TAG_MAP_AFFINE, AGX_TAG_MAP_HOMOGRAPHY = 0, 1
AGX_QUAD_DEGENERATE = 6
# try_find_best_board of caller-given saddle lists (src/detector.rs:588-639): what became of a frame
AGX_BOARD_FOUND, AGX_BOARD_NONE, AGX_BOARD_CAPACITY, AGX_BOARD_INPUT, AGX_BOARD_PENDING = 0, 1, 2, 3, 4
AGX_GROW_FIX_MISSING = 1  # agx_grow_boards_enqueue / agx_grow_board_tail: flags
# caller points snapped to the nearest listed saddle (agx_snap_points_enqueue / _tail): flag, per-frame status, "did not snap"
AGX_SNAP_REVERSE = 1
AGX_SNAP_OK, AGX_SNAP_INPUT = 0, 1
AGX_SNAP_NONE = 0xFFFFFFFF
# cluster centres of caller-given response planes (src/detector.rs:414-429): what became of a frame; INEXACT is a flag OR'd in
AGX_CLUSTERS_OK, AGX_CLUSTERS_CAPACITY, AGX_CLUSTERS_BORDER, AGX_CLUSTERS_OVERFLOW, AGX_CLUSTERS_INEXACT = 0, 1, 2, 3, 0x100
AGX_POINT_FILTERED = 4  # the k / phi filter (src/detector.rs:432-445) removed a refined point
# the rounds of max_num_of_boards (src/detector.rs:510-539): a saddle of a quad an earlier round decoded; a frame's tag table
AGX_POINT_USED = 5
AGX_TAGS_OK, AGX_TAGS_CAPACITY, AGX_TAGS_INPUT, AGX_TAGS_PENDING = 0, 1, 2, 3
# the board's homography from a tag table (agx_board_fit_enqueue / _tail): flag, what became of a frame, what became of a row
AGX_FIT_PREDICT_MISSING = 1
AGX_FIT_OK, AGX_FIT_LOOSE, AGX_FIT_FEW, AGX_FIT_SINGULAR, AGX_FIT_INPUT = 0, 1, 2, 3, 4
AGX_FIT_ROW_INLIER, AGX_FIT_ROW_OUTLIER, AGX_FIT_ROW_OFF_BOARD = 0, 1, 2
# the lens model of agx_board_pose_enqueue_m / _tail_m: pinhole + radial-tangential, pinhole-equidistant (fisheye), double sphere
AGX_LENS_RADTAN, AGX_LENS_EQUIDISTANT, AGX_LENS_DOUBLE_SPHERE = 0, 1, 2
# agx_calibrate_enqueue / _tail: the call's status, its flag; agx_calib_report as a numpy dtype
AGX_CALIB_OK, AGX_CALIB_FEW, AGX_CALIB_SINGULAR = 0, 1, 2
AGX_CALIB_ACCEPT_LOOSE = 1
CALIB_REPORT_DTYPE = [("status", "u4"), ("best_iter", "u4"), ("iterations_run", "u4"), ("n_frames_used", "u4"), ("n_corners", "u4"),
                      ("reserved", "u4"), ("rms", "f8"), ("cost", "f8", (65,))]
# agx_rig_calibrate_enqueue / _tail: the call's status; agx_rig_seed_tail's word per camera; agx_rig_report as a numpy dtype
AGX_RIG_OK, AGX_RIG_FEW, AGX_RIG_SINGULAR = 0, 1, 2
AGX_RIG_CAM_ATTACHED, AGX_RIG_CAM_DETACHED = 0, 1
RIG_REPORT_DTYPE = [("status", "u4"), ("best_iter", "u4"), ("iterations_run", "u4"), ("n_instants_used", "u4"), ("n_frames_used", "u4"),
                    ("n_corners", "u4"), ("n_cams_free", "u4"), ("reserved", "u4"), ("rms", "f8"), ("cost", "f8", (65,))]
AGX_MAP_NONE = -2 ** 31  # both words of a rectification map's entry without a source pixel (agx_rectify_map_enqueue / _tail)
# agx_render_boards_enqueue / _tail: what became of a frame; the flag under which the destination's pixels are the background
AGX_RENDER_OK, AGX_RENDER_EMPTY, AGX_RENDER_INPUT = 0, 1, 2
AGX_RENDER_KEEP_BACKGROUND = 1
AGX_DBG_BLUR, AGX_DBG_RESP, AGX_DBG_MIN, AGX_DBG_CENTERS, AGX_DBG_REFINED = 0, 1, 2, 3, 4
AGX_N_KERNELS = 5


class Params(C.Structure):
    _fields_ = [("tag_spacing_ratio", C.c_float), ("min_saddle_angle", C.c_float),
                ("max_saddle_angle", C.c_float), ("max_num_of_boards", C.c_uint8)]


class SaddleC(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("k", C.c_float), ("theta", C.c_float),
                ("phi", C.c_float)]


class PointC(C.Structure):  # agx_point: one (f32, f32) of initial_corners
    _fields_ = [("x", C.c_float), ("y", C.c_float)]


POINT_DTYPE = [("x", "f4"), ("y", "f4")]  # numpy dtype of agx_point


class TagC(C.Structure):
    _fields_ = [("id", C.c_uint32), ("xy", C.c_float * 8)]


class RenderParams(C.Structure):  # agx_render_params: six 32-bit fields, handed over as const void *
    _fields_ = [("black", C.c_uint32), ("white", C.c_uint32), ("background", C.c_uint32), ("page_margin", C.c_float),
                ("supersample", C.c_uint32), ("flags", C.c_uint32)]


# every symbol include/aprilgrid_amd.h declares: name -> (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "agx_abi_version": (C.c_int, []),
    "agx_status_string": (C.c_char_p, [C.c_int]),
    "agx_last_error": (C.c_char_p, [_P]),
    "agx_family_from_str": (C.c_int, [C.c_char_p, C.POINTER(C.c_int)]),
    "agx_default_params": (None, [C.POINTER(Params)]),
    "agx_detector_create": (C.c_int, [C.c_int, C.POINTER(Params), C.c_int, C.POINTER(_P)]),
    "agx_detector_destroy": (None, [_P]),
    "agx_detector_family_info": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                           C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_int)]),
    "agx_detector_set_limits": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32]),
    "agx_detector_set_stream": (C.c_int, [_P, _P, C.c_int]),
    "agx_detector_sync": (C.c_int, [_P]),
    "agx_detector_set_option": (C.c_int, [_P, C.c_char_p, C.c_int]),
    "agx_detector_get_option": (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_int)]),
    "agx_detector_set_blur_sigma": (C.c_int, [_P, C.c_float]),
    "agx_detector_get_blur_sigma": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "agx_detector_set_half_size_patch": (C.c_int, [_P, C.c_int]),
    "agx_detector_get_half_size_patch": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "agx_refined_saddle_points": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_size_t, C.c_int, _P, C.c_uint32,
                                            C.POINTER(C.c_uint32)]),
    "agx_detect": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_size_t, C.c_int, _P, C.c_uint32,
                             C.POINTER(C.c_uint32)]),
    "agx_detect_planes": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_size_t, C.c_int, C.c_int, _P, C.c_uint32, C.POINTER(C.c_uint32)]),
    "agx_saddles_batch_enqueue": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int]),
    "agx_saddles_batch_fetch": (C.c_int, [_P, _P, C.c_uint32, _P, _P]),
    "agx_saddles_batch_enqueue_to": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int,
                                               _P, C.c_uint32, _P]),
    "agx_host_parallelism": (C.c_int, []),
    "agx_debug_cgroup_cpu_quota": (C.c_int, [C.c_char_p, C.c_char_p]),
    "agx_detect_batch": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, _P, C.c_uint32,
                                   _P, _P, C.c_int]),
    "agx_detect_batch_enqueue": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_uint32]),
    "agx_detect_batch_enqueue_to": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, _P, C.c_uint32,
                                              _P, _P]),
    "agx_detect_batch_fetch": (C.c_int, [_P, _P, _P, _P, C.c_int]),
    "agx_refine_points_enqueue": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, _P, C.c_uint32,
                                            _P, _P, _P]),
    "agx_refine_points_fetch": (C.c_int, [_P, _P, _P]),
    "agx_refine_points_enqueue_h": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, _P, C.c_uint32,
                                              _P, _P, _P, C.c_int]),
    "agx_rochade_refine": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, _P, C.c_uint32, _P, _P,
                                     C.POINTER(C.c_uint32)]),
    "agx_rochade_refine_h": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, _P, C.c_uint32, _P, _P,
                                       C.POINTER(C.c_uint32), C.c_int]),
    "agx_refine_windows_enqueue": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, _P, C.c_size_t, C.c_uint32,
                                             _P, _P, _P, _P, C.c_int, C.c_int]),
    "agx_decimate_enqueue": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, _P, C.c_size_t, C.c_size_t]),
    "agx_decimate_tail": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, _P, C.c_size_t, C.c_size_t]),
    "agx_decode_quads_enqueue": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, _P, C.c_size_t, C.c_uint32,
                                           _P, _P, _P, _P, _P]),
    "agx_decode_quads_fetch": (C.c_int, [_P, _P, _P, _P]),
    "agx_decode_quads": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_size_t, C.c_int, _P, C.c_uint32, _P, _P, _P, C.POINTER(C.c_uint32)]),
    "agx_decode_quads_tail": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_size_t, _P, C.c_uint32, _P, _P, _P, C.POINTER(C.c_uint32)]),
    "agx_decode_positions_enqueue": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_uint32, _P, _P, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_float,
                                               _P, _P]),
    "agx_decode_positions_tail": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_float, _P, _P]),
    "agx_decode_positions_enqueue_m": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_uint32, _P, _P, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_float,
                                                 _P, _P, C.c_int]),
    "agx_decode_positions_tail_m": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_float, _P, _P, C.c_int]),
    "agx_tag_maps_enqueue": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_uint32, _P, _P, C.c_int, C.c_float, C.c_int, _P, _P]),
    "agx_tag_maps_tail": (C.c_int, [_P, C.c_uint32, C.c_int, C.c_float, C.c_int, _P, _P]),
    "agx_bit_code_enqueue": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, _P, C.c_uint32, C.c_uint32, _P, _P,
                                       C.c_int, C.c_uint32, _P, _P]),
    "agx_bit_code_tail": (C.c_int, [_P, C.c_int, C.c_int, C.c_size_t, _P, C.c_uint32, C.c_uint32, _P, C.c_int, C.c_uint32, _P, _P]),
    "agx_best_tag_enqueue": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, _P, C.c_int, _P, C.c_uint32, C.c_int, _P, C.c_size_t, _P, _P, _P, _P]),
    "agx_best_tag_tail": (C.c_int, [_P, C.c_uint32, _P, C.c_int, C.c_int, _P, C.c_uint32, C.c_int, _P, _P, _P, _P, _P]),
    "agx_find_boards_enqueue": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_uint32, _P, _P, _P, C.c_uint32, _P, _P, _P, _P]),
    "agx_find_boards_fetch": (C.c_int, [_P, _P, _P, _P, _P, C.c_int]),
    "agx_find_board": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "agx_find_board_tail": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "agx_init_quads_enqueue": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_uint32, _P, _P, _P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, _P, _P, _P,
                                         _P, _P, _P, _P]),
    "agx_init_quads_fetch": (C.c_int, [_P, C.c_int]),
    "agx_init_quads_tail": (C.c_int, [_P, C.c_uint32, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, C.c_uint32, C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_uint32), _P, _P, C.POINTER(C.c_uint32)]),
    "agx_grow_boards_enqueue": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_uint32, _P, _P, _P, _P, C.c_uint32, _P, C.c_float, C.c_uint32, C.c_int,
                                          C.c_uint32, _P, _P, _P, _P, _P, _P]),
    "agx_grow_boards_fetch": (C.c_int, [_P, C.c_int]),
    "agx_grow_board_tail": (C.c_int, [_P, C.c_uint32, _P, _P, C.c_uint32, C.c_float, C.c_uint32, C.c_int, _P, C.c_uint32, C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_uint32), _P, C.POINTER(C.c_uint32)]),
    "agx_snap_points_enqueue": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_uint32, _P, _P, _P, _P, C.c_size_t, C.c_size_t, C.c_uint32, C.c_uint32, _P,
                                          C.c_float, C.c_int, _P, _P, _P, _P, _P, _P]),
    "agx_snap_points_tail": (C.c_int, [_P, C.c_uint32, _P, _P, C.c_size_t, C.c_size_t, C.c_uint32, C.c_uint32, C.c_float, C.c_int, _P, _P, _P,
                                       C.POINTER(C.c_uint32), _P, C.POINTER(C.c_uint32)]),
    "agx_planes_enqueue": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_float, _P, _P, C.c_size_t,
                                     C.c_size_t]),
    "agx_gaussian_blur_f32": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_float, _P]),
    "agx_hessian_response": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_size_t, C.c_int, _P]),
    "agx_clusters_enqueue": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_uint32, _P, _P, _P, _P]),
    "agx_clusters_fetch": (C.c_int, [_P, _P, _P, _P, _P]),
    "agx_cluster_centers": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_size_t, _P, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "agx_filter_saddles_enqueue": (C.c_int, [_P, _P, _P, C.c_int, C.c_uint32, _P]),
    "agx_filter_saddles_tail": (C.c_int, [C.POINTER(Params), _P, _P, C.c_uint32]),
    "agx_collect_tags_enqueue": (C.c_int, [_P, C.c_int, C.c_uint32, _P, _P, _P, _P, _P, C.c_uint32, _P, _P, C.c_uint32, _P, _P, _P, C.c_int]),
    "agx_collect_tags_tail": (C.c_int, [C.c_int, C.c_uint32, _P, C.c_uint32, _P, _P, C.c_uint32, _P, C.c_uint32, _P, _P, _P]),
    "agx_board_fit_enqueue": (C.c_int, [_P, C.c_int, _P, C.c_uint32, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_int, C.c_int,
                                        C.c_float, C.c_uint32, C.c_uint32, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "agx_board_fit_tail": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_int, C.c_int,
                                     C.c_float, C.c_uint32, C.c_uint32, C.c_int, _P, _P, _P, C.POINTER(C.c_uint32), C.POINTER(C.c_float), _P,
                                     C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "agx_board_pose_enqueue": (C.c_int, [_P, C.c_int, _P, C.c_uint32, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_double,
                                         C.POINTER(C.c_double), C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _P, _P, _P, _P, _P, _P,
                                         _P, _P, _P]),
    "agx_board_pose_tail": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_double,
                                      C.POINTER(C.c_double), C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _P, _P, _P,
                                      C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_uint32), _P, C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_uint32)]),
    "agx_debug_board_pose_sums": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_double,
                                            C.POINTER(C.c_double), C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_uint32), _P]),
    "agx_board_pose_enqueue_m": (C.c_int, [_P, C.c_int, _P, C.c_uint32, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_double, C.c_int,
                                           C.POINTER(C.c_double), C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _P, _P, _P, _P, _P, _P,
                                           _P, _P, _P]),
    "agx_board_pose_tail_m": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_double, C.c_int,
                                        C.POINTER(C.c_double), C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _P, _P, _P,
                                        C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_uint32), _P, C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint32)]),
    "agx_debug_board_pose_sums_m": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_double,
                                              C.c_int, C.POINTER(C.c_double), C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                              C.POINTER(C.c_uint32), _P]),
    "agx_debug_pose_atan": (C.c_int, [_P, C.c_uint32, _P]),
    "agx_debug_pose_project": (C.c_int, [C.c_int, C.POINTER(C.c_double), _P, C.c_uint32, _P]),
    "agx_calibrate_enqueue": (C.c_int, [_P, C.c_int, _P, C.c_uint32, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_double, C.c_int,
                                        C.POINTER(C.c_double), C.c_uint32, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _P, _P, _P, _P, _P,
                                        _P, _P, _P]),
    "agx_calibrate_tail": (C.c_int, [C.c_int, _P, C.c_uint32, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_double, C.c_int,
                                     C.POINTER(C.c_double), C.c_uint32, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _P, _P, _P, _P, _P, _P,
                                     _P, _P]),
    "agx_calibrate_seed_tail": (C.c_int, [_P, _P, C.c_uint32, C.c_int, C.c_int, _P, C.POINTER(C.c_uint32)]),
    "agx_debug_calib_param_jacobian": (C.c_int, [C.c_int, C.POINTER(C.c_double), _P, C.c_uint32, _P]),
    "agx_rig_calibrate_enqueue": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_uint32, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_double,
                                            C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                            _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "agx_rig_calibrate_tail": (C.c_int, [C.c_int, C.c_int, _P, C.c_uint32, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_double,
                                         C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                         _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "agx_rig_seed_tail": (C.c_int, [C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    "agx_debug_rig_jacobian": (C.c_int, [C.c_int, C.POINTER(C.c_double), _P, _P, _P, C.c_uint32, _P]),
    "agx_rectify_map_enqueue": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t]),
    "agx_rectify_map_tail": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t]),
    "agx_remap_enqueue": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, _P, C.c_size_t, C.c_int, C.c_int, _P,
                                    C.c_size_t, C.c_size_t, C.c_uint32]),
    "agx_remap_tail": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, _P, C.c_size_t, C.c_int, C.c_int, _P, C.c_size_t,
                                 C.c_size_t, C.c_uint32]),
    "agx_rectified_points_enqueue": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.c_size_t, C.c_uint32, _P, C.c_size_t]),
    "agx_rectified_points_tail": (C.c_int, [C.c_int, _P, _P, _P, _P, C.c_size_t, C.c_uint32, _P, C.c_size_t]),
    "agx_render_boards_enqueue": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_uint32, C.c_uint32,
                                            C.c_uint32, C.c_float, C.c_double, C.c_int, _P, _P, _P, _P, _P, _P, _P]),
    "agx_render_boards_tail": (C.c_int, [C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float,
                                         C.c_double, C.c_int, _P, _P, _P, _P, _P, _P, _P]),
    "agx_group_create": (C.c_int, [C.c_int, C.POINTER(Params), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(_P)]),
    "agx_group_destroy": (None, [_P]),
    "agx_group_size": (C.c_int, [_P]),
    "agx_group_detector": (_P, [_P, C.c_int]),
    "agx_group_saddles_enqueue": (C.c_int, [_P, C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int,
                                            C.c_uint32]),
    "agx_group_saddles_fetch": (C.c_int, [_P, _P, C.c_uint32, _P, _P]),
    "agx_group_detect_enqueue": (C.c_int, [_P, C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int,
                                           C.c_uint32, C.c_uint32]),
    "agx_group_detect_fetch": (C.c_int, [_P, _P, _P, _P, C.c_int]),
    "agx_group_last_error": (C.c_char_p, [_P]),
    "agx_detect_from_saddles": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_int, C.c_int, C.c_size_t, _P, C.c_uint32,
                                          C.POINTER(C.c_uint32)]),
    "agx_detect_tail": (C.c_int, [C.c_int, C.POINTER(Params), _P, C.c_uint32, _P, C.c_int, C.c_int, C.c_size_t, _P,
                                  C.c_uint32, C.POINTER(C.c_uint32)]),
    "agx_detect_tail_threads": (C.c_int, [C.c_int, C.POINTER(Params), _P, C.c_uint32, _P, C.c_int, C.c_int, C.c_size_t, _P,
                                          C.c_uint32, C.POINTER(C.c_uint32), C.c_int]),
    "agx_luma8": (C.c_int, [_P, C.c_int, C.c_int, C.c_size_t, C.c_int, _P]),
    "agx_debug_angle_pairs": (C.c_int, [_P, C.c_size_t, _P, _P, _P]),
    "agx_debug_angle_pairs_coarse": (C.c_int, [_P, C.c_size_t, _P, _P]),
    "agx_debug_libm_atan2f_check": (C.c_int, [C.c_uint64, C.c_uint64, _P]),
    "agx_debug_white_block_angles": (C.c_int, [_P, C.c_size_t, _P, _P]),
    "agx_profile_enable": (C.c_int, [_P, C.c_int]),
    "agx_profile_reset": (C.c_int, [_P]),
    "agx_profile_read": (C.c_int, [_P, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "agx_debug_fetch": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "agx_detector_constants": (C.c_int, [_P, _P, _P, _P]),
    "agx_debug_blur_weights": (C.c_int, [C.c_float, _P, C.c_int, C.POINTER(C.c_int)]),
    "agx_debug_refine_constants": (C.c_int, [C.c_int, _P, _P, C.c_int, C.POINTER(C.c_int)]),
}


def build_library(force=False):
    """Compile libaprilgrid_amd.so in-tree with hipcc for gfx950 (make -C <package dir>)."""
    cmd = ["make", "-C", _PKG_DIR, "-s"] + (["-B"] if force else [])
    subprocess.check_call(cmd)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "aprilgrid-rs_amd: %s is missing. Build it with `make -C %s` (hipcc, gfx950) or "
                "__graft_entry__.build(). There is no CPU fallback." % (LIB_PATH, _PKG_DIR))
        # One HIP runtime per process: torch bundles its own libamdhip64 / libhsa-runtime64.  If
        # this library pulled in /opt/rocm's copy first and torch loaded its own afterwards, the
        # second runtime would find "no ROCm-capable device".  Import torch first when it is
        # installed so that libamdhip64.so.7 resolves to the copy already in the process.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        # AGX_LIBRARY: another build of the same library (kernel A/B measurements on one GPU box)
        l = C.CDLL(os.environ.get("AGX_LIBRARY") or LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            f = getattr(l, name)  # AttributeError if the library does not export it
            f.restype = res
            f.argtypes = args
        _lib = l
    return _lib
