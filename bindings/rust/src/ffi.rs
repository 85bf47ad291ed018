//! include/aprilgrid_amd.h, declaration for declaration.  Nothing here is written twice by hand without a check:
//! tests/test_rust_binding.py (CPU suite of the repository) parses this file and the header and compares every function's
//! name, argument count and argument / return widths, every `#[repr(C)]` struct's fields, and every constant.
#![allow(non_camel_case_types, dead_code)]
use std::os::raw::{c_char, c_double, c_float, c_int, c_void};

/// `agx_detector` / `agx_group`: opaque handles.
#[repr(C)]
pub struct agx_detector {
    _private: [u8; 0],
}
#[repr(C)]
pub struct agx_group {
    _private: [u8; 0],
}

/// `agx_params` = DetectorParams (reference src/detector.rs:25-30).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct agx_params {
    pub tag_spacing_ratio: c_float,
    pub min_saddle_angle: c_float,
    pub max_saddle_angle: c_float,
    pub max_num_of_boards: u8,
}
/// `agx_saddle` = Saddle (reference src/saddle.rs:3-9), 5 x f32.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct agx_saddle {
    pub x: c_float,
    pub y: c_float,
    pub k: c_float,
    pub theta: c_float,
    pub phi: c_float,
}
/// `agx_tag`: one entry of detect()'s map (reference src/detector.rs:520): id and four corners.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct agx_tag {
    pub id: u32,
    pub xy: [c_float; 8],
}
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct agx_frame_result {
    pub count: u32,
    pub offset: u32,
    pub status: u32,
    pub n_clusters: u32,
}
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct agx_cluster_info {
    pub first_index: u32,
    pub size: u32,
    pub cx: c_float,
    pub cy: c_float,
}

/// `agx_point`: one `(f32, f32)` of rochade_refine's `initial_corners` (reference src/detector.rs:194-361).  The header passes
/// arrays of them as `const void *`; tests/test_refine_points_cpu.py holds this layout to the header's.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct agx_point {
    pub x: c_float,
    pub y: c_float,
}

pub const AGX_ABI_VERSION: c_int = 1;
pub const AGX_N_KERNELS: c_int = 5;

// enum agx_status
pub const AGX_OK: c_int = 0;
pub const AGX_ERR_ARG: c_int = -1;
pub const AGX_ERR_FORMAT: c_int = -2;
pub const AGX_ERR_CAPACITY: c_int = -3;
pub const AGX_ERR_HIP: c_int = -4;
pub const AGX_ERR_NO_DEVICE: c_int = -5;
pub const AGX_ERR_FAMILY: c_int = -6;
pub const AGX_ERR_STATE: c_int = -7;
pub const AGX_ERR_NOMEM: c_int = -8;
// enum agx_family: the order of `enum TagFamily` (reference src/tag_families.rs:5-13)
pub const AGX_T16H5: c_int = 0;
pub const AGX_T25H7: c_int = 1;
pub const AGX_T25H9: c_int = 2;
pub const AGX_T36H11: c_int = 3;
pub const AGX_T36H11B1: c_int = 4;
// enum agx_format
pub const AGX_L8: c_int = 0;
pub const AGX_L16: c_int = 1;
pub const AGX_RGB8: c_int = 2;
pub const AGX_LF32: c_int = 3;
pub const AGX_LA8: c_int = 4;
pub const AGX_RGBA8: c_int = 5;
pub const AGX_BGR8: c_int = 6;
pub const AGX_BGRA8: c_int = 7;
pub const AGX_RGB8P: c_int = 8;
pub const AGX_LA16: c_int = 9;
pub const AGX_RGB16: c_int = 10;
pub const AGX_RGBA16: c_int = 11;
// per-frame status bits of the device frame table
pub const AGX_FRAME_CANDIDATE_OVERFLOW: c_int = 1;
pub const AGX_FRAME_CLUSTER_OVERFLOW: c_int = 2;
pub const AGX_FRAME_SADDLE_OVERFLOW: c_int = 4;
pub const AGX_FRAME_CENTROID_INEXACT: c_int = 8;
pub const AGX_FRAME_GENERIC_PATH: c_int = 16;
pub const AGX_FRAME_DENSE_THRESHOLD: c_int = 32;
pub const AGX_FRAME_LARGE_RESULT: c_int = 64;
// transports of a detector group
pub const AGX_GATHER_RCCL: c_int = 0;
pub const AGX_GATHER_PEER: c_int = 1;
// rochade_refine of caller-given points: a point's status, and the plane it is refined on
pub const AGX_POINT_REFINED: c_int = 0;
pub const AGX_POINT_OUTSIDE: c_int = 1;
pub const AGX_POINT_NOT_SADDLE: c_int = 2;
pub const AGX_POINT_MOVED: c_int = 3;
pub const AGX_REFINE_BLURRED: c_int = 0;
pub const AGX_REFINE_PLANE: c_int = 1;
// try_decode_quad of caller-given quads (reference src/detector.rs:448-476): what became of a quad
pub const AGX_QUAD_DECODED: c_int = 0;
pub const AGX_QUAD_OUTSIDE: c_int = 1;
pub const AGX_QUAD_LOW_CONTRAST: c_int = 2;
pub const AGX_QUAD_AMBIGUOUS: c_int = 3;
pub const AGX_QUAD_NO_MATCH: c_int = 4;
pub const AGX_QUAD_SKIPPED: c_int = 5;
pub const AGX_QUAD_DEGENERATE: c_int = 6;
// the sampling model of decode_positions (reference src/image_util.rs:39-70 tag_affine, :5-37 tag_homography)
pub const AGX_TAG_MAP_AFFINE: c_int = 0;
pub const AGX_TAG_MAP_HOMOGRAPHY: c_int = 1;
// try_find_best_board of caller-given saddle lists (reference src/detector.rs:588-639): what became of a frame
pub const AGX_BOARD_FOUND: c_int = 0;
pub const AGX_BOARD_NONE: c_int = 1;
pub const AGX_BOARD_CAPACITY: c_int = 2;
pub const AGX_BOARD_INPUT: c_int = 3;
pub const AGX_BOARD_PENDING: c_int = 4;
// agx_grow_boards_enqueue / agx_grow_board_tail: flags
pub const AGX_GROW_FIX_MISSING: c_int = 1;
// agx_snap_points_enqueue / agx_snap_points_tail: flag, what became of a frame, and the slot of a point that did not snap
pub const AGX_SNAP_REVERSE: c_int = 1;
pub const AGX_SNAP_OK: c_int = 0;
pub const AGX_SNAP_INPUT: c_int = 1;
pub const AGX_SNAP_NONE: u32 = 0xFFFF_FFFF;
// cluster centres of caller-given response planes (reference src/detector.rs:414-429): what became of a frame
pub const AGX_CLUSTERS_OK: c_int = 0;
pub const AGX_CLUSTERS_CAPACITY: c_int = 1;
pub const AGX_CLUSTERS_BORDER: c_int = 2;
pub const AGX_CLUSTERS_OVERFLOW: c_int = 3;
pub const AGX_CLUSTERS_INEXACT: c_int = 256;
// the k / phi filter (reference src/detector.rs:432-445): the status of a refined point it removes
pub const AGX_POINT_FILTERED: c_int = 4;
// the rounds of max_num_of_boards (reference src/detector.rs:510-539): a saddle of a quad an earlier round decoded, and what
// became of a frame's tag table
pub const AGX_POINT_USED: c_int = 5;
pub const AGX_TAGS_OK: c_int = 0;
pub const AGX_TAGS_CAPACITY: c_int = 1;
pub const AGX_TAGS_INPUT: c_int = 2;
pub const AGX_TAGS_PENDING: c_int = 3;
// agx_board_fit_enqueue / agx_board_fit_tail: flag, what became of a frame, what became of a row
pub const AGX_FIT_PREDICT_MISSING: c_int = 1;
pub const AGX_FIT_OK: c_int = 0;
pub const AGX_FIT_LOOSE: c_int = 1;
pub const AGX_FIT_FEW: c_int = 2;
pub const AGX_FIT_SINGULAR: c_int = 3;
pub const AGX_FIT_INPUT: c_int = 4;
pub const AGX_FIT_ROW_INLIER: c_int = 0;
pub const AGX_FIT_ROW_OUTLIER: c_int = 1;
pub const AGX_FIT_ROW_OFF_BOARD: c_int = 2;
pub const AGX_LENS_RADTAN: c_int = 0;
pub const AGX_LENS_EQUIDISTANT: c_int = 1;
pub const AGX_LENS_DOUBLE_SPHERE: c_int = 2;
// agx_calibrate_enqueue / _tail: the call's status, its flag
pub const AGX_CALIB_OK: c_int = 0;
pub const AGX_CALIB_FEW: c_int = 1;
pub const AGX_CALIB_SINGULAR: c_int = 2;
pub const AGX_CALIB_ACCEPT_LOOSE: c_int = 1;
// agx_rig_calibrate_enqueue / _tail: the call's status; agx_rig_seed_tail's word per camera
pub const AGX_RIG_OK: c_int = 0;
pub const AGX_RIG_FEW: c_int = 1;
pub const AGX_RIG_SINGULAR: c_int = 2;
pub const AGX_RIG_CAM_ATTACHED: c_int = 0;
pub const AGX_RIG_CAM_DETACHED: c_int = 1;
pub const AGX_RENDER_OK: c_int = 0;
pub const AGX_RENDER_EMPTY: c_int = 1;
pub const AGX_RENDER_INPUT: c_int = 2;
pub const AGX_RENDER_KEEP_BACKGROUND: c_int = 1;
/// `params` of `agx_render_boards_enqueue` / `_tail` (the header's `struct agx_render_params`; the prototypes take it as `const void *`)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct agx_render_params {
    pub black: u32,
    pub white: u32,
    pub background: u32,
    pub page_margin: c_float,
    pub supersample: u32,
    pub flags: u32,
}
/// both words of a rectification map's entry that has no source pixel (the header's `#define AGX_MAP_NONE`, INT32_MIN)
pub const AGX_MAP_NONE: i32 = i32::MIN;
// agx_debug_fetch items
pub const AGX_DBG_BLUR: c_int = 0;
pub const AGX_DBG_RESP: c_int = 1;
pub const AGX_DBG_MIN: c_int = 2;
pub const AGX_DBG_CENTERS: c_int = 3;
pub const AGX_DBG_REFINED: c_int = 4;
pub const AGX_DBG_COUNTERS: c_int = 5;
pub const AGX_DBG_RESP_RECOMPUTED: c_int = 6;
pub const AGX_DBG_VERIFY_STATS: c_int = 7;
pub const AGX_DBG_REDZONES: c_int = 8;
pub const AGX_DBG_LUMA8: c_int = 9;
pub const AGX_DBG_WAVE_TIMES: c_int = 10;
pub const AGX_DBG_TAIL_TABLE_ADDR: c_int = 11;

extern "C" {
    pub fn agx_abi_version() -> c_int;
    pub fn agx_status_string(status: c_int) -> *const c_char;
    pub fn agx_last_error(det: *const agx_detector) -> *const c_char;
    pub fn agx_family_from_str(name: *const c_char, family_out: *mut c_int) -> c_int;
    pub fn agx_default_params(out: *mut agx_params);

    pub fn agx_detector_create(family: c_int, params: *const agx_params, device: c_int, out: *mut *mut agx_detector) -> c_int;
    pub fn agx_detector_destroy(det: *mut agx_detector);
    pub fn agx_detector_family_info(det: *const agx_detector, edge_bits: *mut c_int, border_bits: *mut c_int,
                                    hamming_distance: *mut c_int, codes: *mut *const u64, n_codes: *mut c_int) -> c_int;
    pub fn agx_detector_set_limits(det: *mut agx_detector, max_candidates: u32, max_clusters: u32, max_saddles: u32) -> c_int;
    pub fn agx_detector_set_option(det: *mut agx_detector, name: *const c_char, value: c_int) -> c_int;
    pub fn agx_detector_get_option(det: *const agx_detector, name: *const c_char, value: *mut c_int) -> c_int;
    pub fn agx_detector_set_blur_sigma(det: *mut agx_detector, sigma: c_float) -> c_int;
    pub fn agx_detector_get_blur_sigma(det: *const agx_detector, sigma: *mut c_float) -> c_int;
    pub fn agx_detector_set_half_size_patch(det: *mut agx_detector, half_size_patch: c_int) -> c_int;
    pub fn agx_detector_get_half_size_patch(det: *const agx_detector, half_size_patch: *mut c_int) -> c_int;
    pub fn agx_detector_set_stream(det: *mut agx_detector, hip_stream: *mut c_void, external: c_int) -> c_int;
    pub fn agx_detector_sync(det: *mut agx_detector) -> c_int;
    pub fn agx_detector_constants(det: *const agx_detector, blur_w7: *mut c_float, cone25: *mut c_float, pmat150: *mut c_float) -> c_int;

    pub fn agx_refined_saddle_points(det: *mut agx_detector, pixels: *const c_void, width: c_int, height: c_int,
                                     row_stride_bytes: usize, format: c_int, out: *mut agx_saddle, cap: u32, n_out: *mut u32) -> c_int;
    pub fn agx_detect(det: *mut agx_detector, pixels: *const c_void, width: c_int, height: c_int, row_stride_bytes: usize,
                      format: c_int, out: *mut agx_tag, cap: u32, n_out: *mut u32) -> c_int;
    pub fn agx_detect_planes(det: *mut agx_detector, luma32f: *const c_float, stride32f_bytes: usize, luma8: *const u8,
                             stride8_bytes: usize, width: c_int, height: c_int, out: *mut agx_tag, cap: u32, n_out: *mut u32) -> c_int;
    pub fn agx_detect_batch(det: *mut agx_detector, frames: *const c_void, d_frames: *const c_void, n_frames: c_int, width: c_int,
                            height: c_int, row_stride_bytes: usize, frame_stride_bytes: usize, format: c_int, out: *mut agx_tag,
                            cap_per_frame: u32, counts: *mut u32, frame_status: *mut c_int, n_threads: c_int) -> c_int;
    pub fn agx_detect_batch_enqueue(det: *mut agx_detector, d_frames: *const c_void, n_frames: c_int, width: c_int, height: c_int,
                                    row_stride_bytes: usize, frame_stride_bytes: usize, format: c_int, cap_per_frame: u32) -> c_int;
    pub fn agx_detect_batch_enqueue_to(det: *mut agx_detector, d_frames: *const c_void, n_frames: c_int, width: c_int, height: c_int,
                                       row_stride_bytes: usize, frame_stride_bytes: usize, format: c_int, d_tags: *mut agx_tag,
                                       cap_per_frame: u32, d_counts: *mut u32, d_status: *mut c_int) -> c_int;
    pub fn agx_detect_batch_fetch(det: *mut agx_detector, out: *mut agx_tag, counts: *mut u32, frame_status: *mut c_int,
                                  n_threads: c_int) -> c_int;
    pub fn agx_host_parallelism() -> c_int;
    pub fn agx_luma8(pixels: *const c_void, width: c_int, height: c_int, row_stride_bytes: usize, format: c_int, out: *mut u8) -> c_int;

    pub fn agx_saddles_batch_enqueue(det: *mut agx_detector, d_frames: *const c_void, n_frames: c_int, width: c_int, height: c_int,
                                     row_stride_bytes: usize, frame_stride_bytes: usize, format: c_int) -> c_int;
    pub fn agx_saddles_batch_enqueue_to(det: *mut agx_detector, d_frames: *const c_void, n_frames: c_int, width: c_int, height: c_int,
                                        row_stride_bytes: usize, frame_stride_bytes: usize, format: c_int, d_saddles: *mut c_void,
                                        saddle_capacity: u32, d_frame_table: *mut c_void) -> c_int;
    pub fn agx_saddles_batch_fetch(det: *mut agx_detector, out: *mut agx_saddle, cap_per_frame: u32, counts: *mut u32,
                                   frame_status: *mut c_int) -> c_int;

    pub fn agx_refine_points_enqueue(det: *mut agx_detector, d_frames: *const c_void, n_frames: c_int, width: c_int, height: c_int,
                                     row_stride_bytes: usize, frame_stride_bytes: usize, format: c_int, image: c_int,
                                     d_points: *const c_void, points_per_frame: u32, d_counts: *const u32, d_out: *mut agx_saddle,
                                     d_status: *mut u32) -> c_int;
    pub fn agx_refine_points_fetch(det: *mut agx_detector, out: *mut agx_saddle, status: *mut u32) -> c_int;
    pub fn agx_refine_points_enqueue_h(det: *mut agx_detector, d_frames: *const c_void, n_frames: c_int, width: c_int, height: c_int,
                                       row_stride_bytes: usize, frame_stride_bytes: usize, format: c_int, image: c_int,
                                       d_points: *const c_void, points_per_frame: u32, d_counts: *const u32, d_out: *mut agx_saddle,
                                       d_status: *mut u32, half_size_patch: c_int) -> c_int;
    pub fn agx_rochade_refine(det: *mut agx_detector, pixels: *const c_void, width: c_int, height: c_int, row_stride_bytes: usize,
                              format: c_int, image: c_int, points: *const c_void, n_points: u32, out: *mut agx_saddle,
                              status: *mut u32, n_refined: *mut u32) -> c_int;
    pub fn agx_rochade_refine_h(det: *mut agx_detector, pixels: *const c_void, width: c_int, height: c_int, row_stride_bytes: usize,
                                format: c_int, image: c_int, points: *const c_void, n_points: u32, out: *mut agx_saddle,
                                status: *mut u32, n_refined: *mut u32, half_size_patch: c_int) -> c_int;

    pub fn agx_decode_quads_enqueue(det: *mut agx_detector, d_frames: *const c_void, n_frames: c_int, width: c_int, height: c_int,
                                    row_stride_bytes: usize, frame_stride_bytes: usize, format: c_int, d_quads: *const c_void,
                                    point_stride_bytes: usize, quads_per_frame: u32, d_counts: *const u32, d_point_status: *const u32,
                                    d_tags: *mut agx_tag, d_status: *mut u32, d_bits: *mut u64) -> c_int;
    pub fn agx_decode_quads_fetch(det: *mut agx_detector, out: *mut agx_tag, status: *mut u32, bits: *mut u64) -> c_int;
    pub fn agx_decode_quads(det: *mut agx_detector, pixels: *const c_void, width: c_int, height: c_int, row_stride_bytes: usize,
                            format: c_int, quads: *const c_void, n_quads: u32, out: *mut agx_tag, status: *mut u32, bits: *mut u64,
                            n_decoded: *mut u32) -> c_int;
    pub fn agx_decode_quads_tail(family: c_int, luma8: *const u8, width: c_int, height: c_int, row_stride_bytes: usize,
                                 quads: *const c_void, n_quads: u32, out: *mut agx_tag, status: *mut u32, bits: *mut u64,
                                 n_decoded: *mut u32) -> c_int;

    // the decode in three stages: decode_positions, bit_code, best_tag (reference src/detector.rs:42-72, :74-122, :142-169)
    pub fn agx_decode_positions_enqueue(det: *mut agx_detector, d_quads: *const c_void, point_stride_bytes: usize, n_frames: c_int,
                                        quads_per_frame: u32, d_counts: *const u32, d_point_status: *const u32, img_w: u32, img_h: u32,
                                        border_bits: c_int, edge_bits: c_int, margin: c_float, d_points: *mut c_float,
                                        d_status: *mut u32) -> c_int;
    pub fn agx_decode_positions_tail(quads: *const c_void, n_quads: u32, img_w: u32, img_h: u32, border_bits: c_int, edge_bits: c_int,
                                     margin: c_float, points: *mut c_float, status: *mut u32) -> c_int;
    // the sampling model opened (reference src/image_util.rs:5-37 tag_homography, :39-70 tag_affine)
    pub fn agx_decode_positions_enqueue_m(det: *mut agx_detector, d_quads: *const c_void, point_stride_bytes: usize, n_frames: c_int,
                                          quads_per_frame: u32, d_counts: *const u32, d_point_status: *const u32, img_w: u32, img_h: u32,
                                          border_bits: c_int, edge_bits: c_int, margin: c_float, d_points: *mut c_float,
                                          d_status: *mut u32, model: c_int) -> c_int;
    pub fn agx_decode_positions_tail_m(quads: *const c_void, n_quads: u32, img_w: u32, img_h: u32, border_bits: c_int, edge_bits: c_int,
                                       margin: c_float, points: *mut c_float, status: *mut u32, model: c_int) -> c_int;
    pub fn agx_tag_maps_enqueue(det: *mut agx_detector, d_quads: *const c_void, point_stride_bytes: usize, n_frames: c_int,
                                quads_per_frame: u32, d_counts: *const u32, d_point_status: *const u32, side_bits: c_int,
                                margin: c_float, model: c_int, d_maps: *mut c_float, d_status: *mut u32) -> c_int;
    pub fn agx_tag_maps_tail(quads: *const c_void, n_quads: u32, side_bits: c_int, margin: c_float, model: c_int, maps: *mut c_float,
                             status: *mut u32) -> c_int;
    pub fn agx_bit_code_enqueue(det: *mut agx_detector, d_frames: *const c_void, n_frames: c_int, width: c_int, height: c_int,
                                row_stride_bytes: usize, frame_stride_bytes: usize, format: c_int, d_points: *const c_float,
                                points_per_slot: u32, quads_per_frame: u32, d_counts: *const u32, d_status_in: *const u32,
                                valid_brightness_threshold: c_int, max_invalid_bit: u32, d_bits: *mut u64, d_status: *mut u32) -> c_int;
    pub fn agx_bit_code_tail(luma8: *const u8, width: c_int, height: c_int, row_stride_bytes: usize, points: *const c_float,
                             points_per_slot: u32, n_slots: u32, status_in: *const u32, valid_brightness_threshold: c_int,
                             max_invalid_bit: u32, bits: *mut u64, status: *mut u32) -> c_int;
    pub fn agx_best_tag_enqueue(det: *mut agx_detector, d_bits: *const u64, n_slots: u32, quads_per_frame: u32, d_counts: *const u32,
                                d_status_in: *const u32, thres: c_int, d_codes: *const u64, n_codes: u32, edge_bits: c_int,
                                d_quads: *const c_void, point_stride_bytes: usize, d_ids: *mut u32, d_rotations: *mut u32,
                                d_status: *mut u32, d_tags: *mut agx_tag) -> c_int;
    pub fn agx_best_tag_tail(bits: *const u64, n_slots: u32, status_in: *const u32, thres: c_int, family: c_int, codes: *const u64,
                             n_codes: u32, edge_bits: c_int, quads: *const c_void, ids: *mut u32, rotations: *mut u32, status: *mut u32,
                             tags: *mut agx_tag) -> c_int;

    pub fn agx_find_boards_enqueue(det: *mut agx_detector, d_saddles: *const c_void, saddle_stride_bytes: usize, n_frames: c_int,
                                   saddles_per_frame: u32, d_counts: *const u32, d_frame_table: *const c_void, d_point_status: *const u32,
                                   quads_per_frame: u32, d_quads: *mut u32, d_quad_points: *mut c_float, d_n_quads: *mut u32,
                                   d_status: *mut u32) -> c_int;
    pub fn agx_find_boards_fetch(det: *mut agx_detector, quads: *mut u32, quad_points: *mut c_float, n_quads: *mut u32, status: *mut u32,
                                 n_threads: c_int) -> c_int;
    pub fn agx_find_board(det: *mut agx_detector, saddles: *const agx_saddle, n_saddles: u32, quads: *mut u32, cap: u32,
                          n_quads: *mut u32, status: *mut u32) -> c_int;
    pub fn agx_find_board_tail(saddles: *const agx_saddle, n_saddles: u32, quads: *mut u32, cap: u32, n_quads: *mut u32,
                               status: *mut u32) -> c_int;

    pub fn agx_init_quads_enqueue(det: *mut agx_detector, d_saddles: *const c_void, saddle_stride_bytes: usize, n_frames: c_int,
                                  saddles_per_frame: u32, d_counts: *const u32, d_frame_table: *const c_void, d_point_status: *const u32,
                                  d_seed_saddles: *const u32, seeds_per_frame: u32, d_seed_counts: *const u32, n_nearest: u32,
                                  quads_per_frame: u32, d_quads: *mut u32, d_quad_points: *mut c_float, d_n_quads: *mut u32,
                                  d_status: *mut u32, d_seed_quad_counts: *mut u32, d_seeds_out: *mut u32, d_n_seeds_out: *mut u32) -> c_int;
    pub fn agx_init_quads_fetch(det: *mut agx_detector, n_threads: c_int) -> c_int;
    pub fn agx_init_quads_tail(saddles: *const agx_saddle, n_saddles: u32, point_status: *const u32, seed_saddles: *const u32, n_seeds: u32,
                               max_seeds: u32, n_nearest: u32, quads: *mut u32, cap: u32, n_quads: *mut u32, status: *mut u32,
                               seed_quad_counts: *mut u32, seeds_out: *mut u32, n_seeds_out: *mut u32) -> c_int;

    pub fn agx_grow_boards_enqueue(det: *mut agx_detector, d_saddles: *const c_void, saddle_stride_bytes: usize, n_frames: c_int,
                                   saddles_per_frame: u32, d_counts: *const u32, d_frame_table: *const c_void, d_point_status: *const u32,
                                   d_seed_quads: *const u32, seeds_per_frame: u32, d_seed_counts: *const u32, spacing_ratio: c_float,
                                   stop_score: u32, flags: c_int, quads_per_frame: u32, d_quads: *mut u32, d_quad_points: *mut c_float,
                                   d_n_quads: *mut u32, d_status: *mut u32, d_seed_scores: *mut u32, d_best_seed: *mut u32) -> c_int;
    pub fn agx_grow_boards_fetch(det: *mut agx_detector, n_threads: c_int) -> c_int;
    pub fn agx_grow_board_tail(saddles: *const agx_saddle, n_saddles: u32, point_status: *const u32, seed_quads: *const u32, n_seeds: u32,
                               spacing_ratio: c_float, stop_score: u32, flags: c_int, quads: *mut u32, cap: u32, n_quads: *mut u32,
                               status: *mut u32, seed_scores: *mut u32, best_seed: *mut u32) -> c_int;

    pub fn agx_snap_points_enqueue(det: *mut agx_detector, d_saddles: *const c_void, saddle_stride_bytes: usize, n_frames: c_int,
                                   saddles_per_frame: u32, d_counts: *const u32, d_frame_table: *const c_void, d_point_status: *const u32,
                                   d_points: *const c_void, row_stride_bytes: usize, point_stride_bytes: usize, rows_per_frame: u32,
                                   points_per_row: u32, d_row_counts: *const u32, max_dist_sq: c_float, flags: c_int, d_slots: *mut u32,
                                   d_dist_sq: *mut c_float, d_rows: *mut u32, d_n_rows: *mut u32, d_row_index: *mut u32,
                                   d_status: *mut u32) -> c_int;
    pub fn agx_snap_points_tail(saddles: *const agx_saddle, n_saddles: u32, point_status: *const u32, points: *const c_void,
                                row_stride_bytes: usize, point_stride_bytes: usize, n_rows: u32, points_per_row: u32, max_dist_sq: c_float,
                                flags: c_int, slots: *mut u32, dist_sq: *mut c_float, rows: *mut u32, n_rows_out: *mut u32,
                                row_index: *mut u32, status: *mut u32) -> c_int;

    pub fn agx_planes_enqueue(det: *mut agx_detector, d_frames: *const c_void, n_frames: c_int, width: c_int, height: c_int,
                              row_stride_bytes: usize, frame_stride_bytes: usize, format: c_int, sigma: c_float, d_blur: *mut c_float,
                              d_response: *mut c_float, out_row_stride_bytes: usize, out_frame_stride_bytes: usize) -> c_int;
    pub fn agx_gaussian_blur_f32(det: *mut agx_detector, pixels: *const c_void, width: c_int, height: c_int, row_stride_bytes: usize,
                                 format: c_int, sigma: c_float, out: *mut c_float) -> c_int;
    pub fn agx_hessian_response(det: *mut agx_detector, pixels: *const c_void, width: c_int, height: c_int, row_stride_bytes: usize,
                                format: c_int, out: *mut c_float) -> c_int;
    pub fn agx_clusters_enqueue(det: *mut agx_detector, d_response: *const c_float, n_frames: c_int, width: c_int, height: c_int,
                                row_stride_bytes: usize, frame_stride_bytes: usize, clusters_per_frame: u32, d_clusters: *mut agx_cluster_info,
                                d_points: *mut c_void, d_counts: *mut u32, d_status: *mut u32) -> c_int;
    pub fn agx_clusters_fetch(det: *mut agx_detector, clusters: *mut agx_cluster_info, points: *mut c_void, counts: *mut u32,
                              status: *mut u32) -> c_int;
    pub fn agx_cluster_centers(det: *mut agx_detector, response: *const c_float, width: c_int, height: c_int, row_stride_bytes: usize,
                               out: *mut agx_cluster_info, cap: u32, n_out: *mut u32, status: *mut u32) -> c_int;
    pub fn agx_filter_saddles_enqueue(det: *mut agx_detector, d_records: *const agx_saddle, d_status: *mut u32, n_frames: c_int,
                                      points_per_frame: u32, d_counts: *const u32) -> c_int;
    pub fn agx_filter_saddles_tail(params: *const agx_params, records: *const agx_saddle, status: *mut u32, n: u32) -> c_int;
    pub fn agx_collect_tags_enqueue(det: *mut agx_detector, n_frames: c_int, quads_per_frame: u32, d_quads: *const u32,
                                    d_n_quads: *const u32, d_board_status: *const u32, d_quad_tags: *const agx_tag,
                                    d_quad_status: *const u32, saddles_per_frame: u32, d_frame_table: *const c_void,
                                    d_point_status: *mut u32, tags_per_frame: u32, d_tags: *mut agx_tag, d_n_tags: *mut u32,
                                    d_tag_status: *mut u32, reset: c_int) -> c_int;
    pub fn agx_collect_tags_tail(family: c_int, n_quads: u32, quads: *const u32, board_status: u32, quad_tags: *const agx_tag,
                                 quad_status: *const u32, n_slots: u32, point_status: *mut u32, tag_cap: u32, tags: *mut agx_tag,
                                 n_tags: *mut u32, tag_status: *mut u32) -> c_int;

    pub fn agx_board_fit_enqueue(det: *mut agx_detector, n_frames: c_int, d_tags: *const agx_tag, tags_per_frame: u32, d_n_tags: *const u32,
                                 d_tag_status: *const u32, cols: u32, rows: u32, first_id: u32, spacing_ratio: c_float, img_w: c_int,
                                 img_h: c_int, max_err_sq: c_float, max_drop: u32, min_tags: u32, flags: c_int, d_h: *mut c_double,
                                 d_err_sq: *mut c_float, d_row_status: *mut u32, d_n_inliers: *mut u32, d_rms: *mut c_float,
                                 d_pred: *mut agx_tag, d_n_pred: *mut u32, d_status: *mut u32) -> c_int;
    pub fn agx_board_fit_tail(tags: *const agx_tag, tags_per_frame: u32, n_tags: u32, tag_status: u32, cols: u32, rows: u32, first_id: u32,
                              spacing_ratio: c_float, img_w: c_int, img_h: c_int, max_err_sq: c_float, max_drop: u32, min_tags: u32,
                              flags: c_int, h: *mut c_double, err_sq: *mut c_float, row_status: *mut u32, n_inliers: *mut u32,
                              rms: *mut c_float, pred: *mut agx_tag, n_pred: *mut u32, status: *mut u32) -> c_int;
    // camera: the nine doubles of an agx_camera (fx, fy, cx, cy, k1, k2, p1, p2, k3), host memory
    pub fn agx_board_pose_enqueue(det: *mut agx_detector, n_frames: c_int, d_tags: *const agx_tag, tags_per_frame: u32, d_n_tags: *const u32,
                                  d_tag_status: *const u32, cols: u32, rows: u32, first_id: u32, spacing_ratio: c_float, tag_size: c_double,
                                  camera: *const c_double, max_err_sq: c_float, max_drop: u32, min_tags: u32, iterations: u32, flags: c_int,
                                  d_pose: *mut c_double, d_err_sq: *mut c_float, d_row_status: *mut u32, d_n_inliers: *mut u32,
                                  d_rms: *mut c_float, d_best_iter: *mut u32, d_pred: *mut agx_tag, d_n_pred: *mut u32,
                                  d_status: *mut u32) -> c_int;
    pub fn agx_board_pose_tail(tags: *const agx_tag, tags_per_frame: u32, n_tags: u32, tag_status: u32, cols: u32, rows: u32, first_id: u32,
                               spacing_ratio: c_float, tag_size: c_double, camera: *const c_double, max_err_sq: c_float, max_drop: u32,
                               min_tags: u32, iterations: u32, flags: c_int, pose: *mut c_double, err_sq: *mut c_float,
                               row_status: *mut u32, n_inliers: *mut u32, rms: *mut c_float, best_iter: *mut u32, pred: *mut agx_tag,
                               n_pred: *mut u32, status: *mut u32) -> c_int;
    pub fn agx_debug_board_pose_sums(tags: *const agx_tag, tags_per_frame: u32, n_tags: u32, tag_status: u32, cols: u32, rows: u32,
                                     first_id: u32, spacing_ratio: c_float, tag_size: c_double, camera: *const c_double,
                                     max_err_sq: c_float, max_drop: u32, min_tags: u32, iterations: u32, flags: c_int,
                                     status: *mut u32, iter_sums: *mut c_double) -> c_int;
    // lens_model: AGX_LENS_*; under AGX_LENS_EQUIDISTANT camera is fx, fy, cx, cy, k1, k2, k3, k4, 0; under
    // AGX_LENS_DOUBLE_SPHERE fx, fy, cx, cy, xi, alpha, 0, 0, 0
    pub fn agx_board_pose_enqueue_m(det: *mut agx_detector, n_frames: c_int, d_tags: *const agx_tag, tags_per_frame: u32, d_n_tags: *const u32,
                                    d_tag_status: *const u32, cols: u32, rows: u32, first_id: u32, spacing_ratio: c_float, tag_size: c_double,
                                    lens_model: c_int, camera: *const c_double, max_err_sq: c_float, max_drop: u32, min_tags: u32,
                                    iterations: u32, flags: c_int, d_pose: *mut c_double, d_err_sq: *mut c_float, d_row_status: *mut u32,
                                    d_n_inliers: *mut u32, d_rms: *mut c_float, d_best_iter: *mut u32, d_pred: *mut agx_tag,
                                    d_n_pred: *mut u32, d_status: *mut u32) -> c_int;
    pub fn agx_board_pose_tail_m(tags: *const agx_tag, tags_per_frame: u32, n_tags: u32, tag_status: u32, cols: u32, rows: u32, first_id: u32,
                                 spacing_ratio: c_float, tag_size: c_double, lens_model: c_int, camera: *const c_double, max_err_sq: c_float,
                                 max_drop: u32, min_tags: u32, iterations: u32, flags: c_int, pose: *mut c_double, err_sq: *mut c_float,
                                 row_status: *mut u32, n_inliers: *mut u32, rms: *mut c_float, best_iter: *mut u32, pred: *mut agx_tag,
                                 n_pred: *mut u32, status: *mut u32) -> c_int;
    pub fn agx_debug_board_pose_sums_m(tags: *const agx_tag, tags_per_frame: u32, n_tags: u32, tag_status: u32, cols: u32, rows: u32,
                                       first_id: u32, spacing_ratio: c_float, tag_size: c_double, lens_model: c_int, camera: *const c_double,
                                       max_err_sq: c_float, max_drop: u32, min_tags: u32, iterations: u32, flags: c_int,
                                       status: *mut u32, iter_sums: *mut c_double) -> c_int;
    pub fn agx_debug_pose_atan(r: *const c_double, n: u32, out: *mut c_double) -> c_int;
    pub fn agx_debug_pose_project(lens_model: c_int, camera: *const c_double, xyz: *const c_double, n: u32, uv: *mut c_double) -> c_int;
    // the camera from the batch; d_report / report: one agx_calib_report (lib.rs: CalibReport), 8-byte aligned
    pub fn agx_calibrate_enqueue(det: *mut agx_detector, n_frames: c_int, d_tags: *const agx_tag, tags_per_frame: u32, d_n_tags: *const u32,
                                 d_tag_status: *const u32, cols: u32, rows: u32, first_id: u32, spacing_ratio: c_float, tag_size: c_double,
                                 lens_model: c_int, camera: *const c_double, fixed_mask: u32, damping: c_double, iterations: u32, min_tags: u32,
                                 min_frames: u32, flags: c_int, d_pose_in: *const c_double, d_row_status: *const u32, d_fit_status: *const u32,
                                 d_camera: *mut c_double, d_pose: *mut c_double, d_frame_cost: *mut c_float, d_frame_n: *mut u32,
                                 d_report: *mut c_void) -> c_int;
    pub fn agx_calibrate_tail(n_frames: c_int, tags: *const agx_tag, tags_per_frame: u32, n_tags: *const u32, tag_status: *const u32, cols: u32,
                              rows: u32, first_id: u32, spacing_ratio: c_float, tag_size: c_double, lens_model: c_int, camera: *const c_double,
                              fixed_mask: u32, damping: c_double, iterations: u32, min_tags: u32, min_frames: u32, flags: c_int,
                              pose_in: *const c_double, row_status: *const u32, fit_status: *const u32, camera_out: *mut c_double,
                              pose: *mut c_double, frame_cost: *mut c_float, frame_n: *mut u32, report: *mut c_void) -> c_int;
    pub fn agx_calibrate_seed_tail(h: *const c_double, fit_status: *const u32, n: u32, img_w: c_int, img_h: c_int, camera_out: *mut c_double,
                                   status: *mut u32) -> c_int;
    pub fn agx_debug_calib_param_jacobian(lens_model: c_int, camera: *const c_double, xyz: *const c_double, n: u32, out: *mut c_double) -> c_int;
    // the rig from the batch; d_report / report: one agx_rig_report (lib.rs: RigReport), 8-byte aligned
    pub fn agx_rig_calibrate_enqueue(det: *mut agx_detector, n_cams: c_int, n_instants: c_int, d_tags: *const agx_tag, tags_per_frame: u32,
                                     d_n_tags: *const u32, d_tag_status: *const u32, cols: u32, rows: u32, first_id: u32, spacing_ratio: c_float,
                                     tag_size: c_double, lens_models: *const c_int, cameras: *const c_double, damping: c_double, iterations: u32,
                                     min_tags: u32, min_cams: u32, min_instants: u32, flags: c_int, d_pose_in: *const c_double,
                                     d_row_status: *const u32, d_fit_status: *const u32, d_extrinsics_in: *const c_double,
                                     d_extrinsics: *mut c_double, d_rig_pose: *mut c_double, d_frame_cost: *mut c_float, d_frame_n: *mut u32,
                                     d_cam_n: *mut u32, d_report: *mut c_void) -> c_int;
    pub fn agx_rig_calibrate_tail(n_cams: c_int, n_instants: c_int, tags: *const agx_tag, tags_per_frame: u32, n_tags: *const u32,
                                  tag_status: *const u32, cols: u32, rows: u32, first_id: u32, spacing_ratio: c_float, tag_size: c_double,
                                  lens_models: *const c_int, cameras: *const c_double, damping: c_double, iterations: u32, min_tags: u32,
                                  min_cams: u32, min_instants: u32, flags: c_int, pose_in: *const c_double, row_status: *const u32,
                                  fit_status: *const u32, extrinsics_in: *const c_double, extrinsics: *mut c_double, rig_pose: *mut c_double,
                                  frame_cost: *mut c_float, frame_n: *mut u32, cam_n: *mut u32, report: *mut c_void) -> c_int;
    pub fn agx_rig_seed_tail(n_cams: c_int, n_instants: c_int, pose: *const c_double, fit_status: *const u32, frame_n: *const u32,
                             extrinsics_out: *mut c_double, cam_status: *mut u32) -> c_int;
    pub fn agx_debug_rig_jacobian(lens_model: c_int, camera: *const c_double, extrinsic: *const c_double, rig_pose: *const c_double,
                                  XY: *const c_double, n: u32, out: *mut c_double) -> c_int;
    // rectified batches: the map (two 32-bit words per destination pixel in 1/32 source px, or AGX_MAP_NONE), the remap, points back
    pub fn agx_rectify_map_enqueue(det: *mut agx_detector, lens_model: c_int, camera: *const c_double, new_camera: *const c_double,
                                   rotation: *const c_double, src_width: c_int, src_height: c_int, dst_width: c_int, dst_height: c_int,
                                   d_map: *mut c_int, map_row_stride_bytes: usize) -> c_int;
    pub fn agx_rectify_map_tail(lens_model: c_int, camera: *const c_double, new_camera: *const c_double, rotation: *const c_double,
                                src_width: c_int, src_height: c_int, dst_width: c_int, dst_height: c_int, map: *mut c_int,
                                map_row_stride_bytes: usize) -> c_int;
    pub fn agx_remap_enqueue(det: *mut agx_detector, d_src: *const c_void, n_frames: c_int, src_width: c_int, src_height: c_int,
                             src_row_stride_bytes: usize, src_frame_stride_bytes: usize, format: c_int, d_map: *const c_int,
                             map_row_stride_bytes: usize, dst_width: c_int, dst_height: c_int, d_dst: *mut c_void,
                             dst_row_stride_bytes: usize, dst_frame_stride_bytes: usize, border: u32) -> c_int;
    pub fn agx_remap_tail(src: *const c_void, n_frames: c_int, src_width: c_int, src_height: c_int, src_row_stride_bytes: usize,
                          src_frame_stride_bytes: usize, format: c_int, map: *const c_int, map_row_stride_bytes: usize, dst_width: c_int,
                          dst_height: c_int, dst: *mut c_void, dst_row_stride_bytes: usize, dst_frame_stride_bytes: usize, border: u32) -> c_int;
    pub fn agx_rectified_points_enqueue(det: *mut agx_detector, lens_model: c_int, camera: *const c_double, new_camera: *const c_double,
                                        rotation: *const c_double, d_points: *const c_void, point_stride_bytes: usize, n_points: u32,
                                        d_out: *mut c_void, out_stride_bytes: usize) -> c_int;
    pub fn agx_rectified_points_tail(lens_model: c_int, camera: *const c_double, new_camera: *const c_double, rotation: *const c_double,
                                     points: *const c_void, point_stride_bytes: usize, n_points: u32, out: *mut c_void,
                                     out_stride_bytes: usize) -> c_int;
    // the board through pose and lens model; params: an agx_render_params (six 32-bit fields: black, white, background as u32,
    // page_margin as f32, supersample and flags as u32), handed over as const void *
    pub fn agx_render_boards_enqueue(det: *mut agx_detector, n_frames: c_int, width: c_int, height: c_int, row_stride_bytes: usize,
                                     frame_stride_bytes: usize, format: c_int, family: c_int, cols: u32, rows: u32, first_id: u32,
                                     spacing_ratio: c_float, tag_size: c_double, lens_model: c_int, camera: *const c_double,
                                     d_poses: *const c_double, params: *const c_void, d_frames: *mut c_void, d_truth: *mut agx_tag,
                                     d_n_truth: *mut u32, d_status: *mut u32) -> c_int;
    pub fn agx_render_boards_tail(width: c_int, height: c_int, row_stride_bytes: usize, format: c_int, family: c_int, cols: u32, rows: u32,
                                  first_id: u32, spacing_ratio: c_float, tag_size: c_double, lens_model: c_int, camera: *const c_double,
                                  pose: *const c_double, params: *const c_void, frame: *mut c_void, truth: *mut agx_tag, n_truth: *mut u32,
                                  status: *mut u32) -> c_int;
    // coarse to fine: the batch averaged down by `factor`, and rochade_refine on the blur of the full frames with every point's blur
    // window computed from the input (no blur plane); its `factor` takes a point of the decimated frame to full resolution
    pub fn agx_decimate_enqueue(det: *mut agx_detector, d_src: *const c_void, n_frames: c_int, width: c_int, height: c_int,
                                row_stride_bytes: usize, frame_stride_bytes: usize, format: c_int, factor: c_int, d_dst: *mut c_void,
                                dst_row_stride_bytes: usize, dst_frame_stride_bytes: usize) -> c_int;
    pub fn agx_decimate_tail(src: *const c_void, n_frames: c_int, width: c_int, height: c_int, row_stride_bytes: usize,
                             frame_stride_bytes: usize, format: c_int, factor: c_int, dst: *mut c_void, dst_row_stride_bytes: usize,
                             dst_frame_stride_bytes: usize) -> c_int;
    pub fn agx_refine_windows_enqueue(det: *mut agx_detector, d_frames: *const c_void, n_frames: c_int, width: c_int, height: c_int,
                                      row_stride_bytes: usize, frame_stride_bytes: usize, format: c_int, d_points: *const c_void,
                                      point_stride_bytes: usize, points_per_frame: u32, d_counts: *const u32, d_status_in: *const u32,
                                      d_out: *mut agx_saddle, d_status: *mut u32, factor: c_int, half_size_patch: c_int) -> c_int;
    pub fn agx_debug_blur_weights(sigma: c_float, weights: *mut c_float, cap: c_int, radius: *mut c_int) -> c_int;
    pub fn agx_debug_refine_constants(half_size_patch: c_int, cone: *mut c_float, pmat: *mut c_float, cap_points: c_int,
                                      n_points: *mut c_int) -> c_int;

    pub fn agx_detect_from_saddles(det: *const agx_detector, saddles: *const agx_saddle, n_saddles: u32, luma8: *const u8, width: c_int,
                                   height: c_int, row_stride_bytes: usize, out: *mut agx_tag, cap: u32, n_out: *mut u32) -> c_int;
    pub fn agx_detect_tail(family: c_int, params: *const agx_params, saddles: *const agx_saddle, n_saddles: u32, luma8: *const u8,
                           width: c_int, height: c_int, row_stride_bytes: usize, out: *mut agx_tag, cap: u32, n_out: *mut u32) -> c_int;
    pub fn agx_detect_tail_threads(family: c_int, params: *const agx_params, saddles: *const agx_saddle, n_saddles: u32,
                                   luma8: *const u8, width: c_int, height: c_int, row_stride_bytes: usize, out: *mut agx_tag, cap: u32,
                                   n_out: *mut u32, n_threads: c_int) -> c_int;

    pub fn agx_group_create(family: c_int, params: *const agx_params, devices: *const c_int, n_devices: c_int, transport: c_int,
                            out: *mut *mut agx_group) -> c_int;
    pub fn agx_group_destroy(group: *mut agx_group);
    pub fn agx_group_size(group: *const agx_group) -> c_int;
    pub fn agx_group_detector(group: *mut agx_group, rank: c_int) -> *mut agx_detector;
    pub fn agx_group_saddles_enqueue(group: *mut agx_group, d_frames: *const *const c_void, frames_per_rank: c_int, width: c_int,
                                     height: c_int, row_stride_bytes: usize, frame_stride_bytes: usize, format: c_int,
                                     records_per_frame: u32) -> c_int;
    pub fn agx_group_saddles_fetch(group: *mut agx_group, out: *mut agx_saddle, cap_per_frame: u32, counts: *mut u32,
                                   frame_status: *mut c_int) -> c_int;
    pub fn agx_group_detect_enqueue(group: *mut agx_group, d_frames: *const *const c_void, frames_per_rank: c_int, width: c_int,
                                    height: c_int, row_stride_bytes: usize, frame_stride_bytes: usize, format: c_int,
                                    cap_per_frame: u32, tags_per_frame: u32) -> c_int;
    pub fn agx_group_detect_fetch(group: *mut agx_group, out: *mut agx_tag, counts: *mut u32, frame_status: *mut c_int,
                                  n_threads: c_int) -> c_int;
    pub fn agx_group_last_error(group: *const agx_group) -> *const c_char;

    pub fn agx_profile_enable(det: *mut agx_detector, on: c_int) -> c_int;
    pub fn agx_profile_reset(det: *mut agx_detector) -> c_int;
    pub fn agx_profile_read(det: *mut agx_detector, names: *mut *const c_char, ms_total: *mut c_double, launches: *mut u64) -> c_int;
    pub fn agx_debug_fetch(det: *mut agx_detector, frame: c_int, what: c_int, host_out: *mut c_void, cap_bytes: usize,
                           n_items: *mut usize) -> c_int;
    pub fn agx_debug_angle_pairs(vectors: *const c_float, n: usize, exact: *mut c_float, approx: *mut c_float, has_approx: *mut u8) -> c_int;
    pub fn agx_debug_angle_pairs_coarse(vectors: *const c_float, n: usize, coarse: *mut c_float, has_coarse: *mut u8) -> c_int;
    pub fn agx_debug_libm_atan2f_check(n: u64, seed: u64, mismatches: *mut u64) -> c_int;
    pub fn agx_debug_white_block_angles(triples: *const c_float, n: usize, reference: *mut c_float, binary64: *mut c_double) -> c_int;
    pub fn agx_debug_cgroup_cpu_quota(cgroup_root: *const c_char, proc_self_cgroup: *const c_char) -> c_int;
}
