// rectify.h -- host-visible interface of rectify.hip: the rectification map of a camera (k_rectify_map), the remap of a batch of
// L8 / L16 frames through a map (k_remap), rectified points back to the sensor (k_rectified_points), and the three host forms.  The
// arithmetic is rectify_math.h's for both.  Internal to the library; the public boundary is include/aprilgrid_amd.h.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/aprilgrid_amd.h"
#include "rectify_math.h"

namespace agx {

constexpr int REMAP_PX = 4;                // adjacent destination pixels per lane: one dword (L8) or two (L16) per store
constexpr int REMAP_FRAMES_PER_GROUP = 16; // frames a workgroup applies its map entries to

struct RectifyMapArgs {
    int lens;  // AGX_LENS_*
    RectifyGeom g;
    int src_w, src_h, dst_w, dst_h;  // 1 .. RECT_MAX_SIDE
    int32_t *map;                    // [dst_h][dst_w][2], 8-byte aligned
    size_t map_stride;               // bytes, a multiple of 8, >= 8 dst_w
};

struct RemapArgs {
    const void *src;  // [n_frames] frames of src_h rows
    int n_frames, src_w, src_h;
    size_t src_row_stride, src_frame_stride;  // bytes; src_row_stride * src_h < 2^31
    int format;                               // AGX_L8 or AGX_L16
    const int32_t *map;
    size_t map_stride;
    int dst_w, dst_h;
    void *dst;
    size_t dst_row_stride, dst_frame_stride;  // bytes; dst_row_stride * dst_h < 2^31
    uint32_t border;
};

struct RectifiedPointsArgs {
    int lens;
    RectifyGeom g;
    const void *points;  // point i: two floats at points + i * stride
    size_t stride;       // bytes, a multiple of 4, >= 8
    uint32_t n;
    void *out;  // may be points
    size_t out_stride;
};

// what every form refuses (null: nothing) -- the text of the AGX_ERR_ARG
const char *rectify_map_args_bad(const RectifyMapArgs &a);
const char *remap_args_bad(const RemapArgs &a);
const char *rectified_points_args_bad(const RectifiedPointsArgs &a);

// device pointers; hipError_t.  Arguments as checked by the functions above.
int launch_rectify_map(const RectifyMapArgs &a, void *stream);
int launch_remap(const RemapArgs &a, void *stream);
int launch_rectified_points(const RectifiedPointsArgs &a, void *stream);

// the same on host memory
void rectify_map_host(const RectifyMapArgs &a);
void remap_host(const RemapArgs &a);
void rectified_points_host(const RectifiedPointsArgs &a);

}  // namespace agx
