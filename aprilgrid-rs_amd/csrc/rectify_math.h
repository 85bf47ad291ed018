// rectify_math.h -- a rectified (ideal pinhole) pixel to the sensor pixel it comes from, the rectification map's entry, and the
// remap's fixed-point blend: one definition each for the kernels (rectify.hip) and the host forms (rectify.hip: rectify_map_host,
// remap_host, rectified_points_host).  The reference has no such function.
//
// A rectified point (x, y) of the pinhole `new_camera` = fx' fy' cx' cy', THE ORDER OF OPERATIONS, binary64, no contraction:
//   dx = (x - cx') / fx',  dy = (y - cy') / fy';   X = R0 dx + R1 dy + R2,  Y = R3 dx + R4 dy + R5,  Z = R6 dx + R7 dy + R8
//   (left to right; R row major, rectified frame -> camera frame; no rotation is the identity matrix through the same statements);
//   (u, v) = board_pose_math.h's pose_project<LENS> of the point (X, Y) under the identity pose moved to Z -- the call behind
//   agx_debug_pose_project, not restated here.  No projection: Z not > 0 (under AGX_LENS_DOUBLE_SPHERE: (X, Y, Z) outside the
//   model's valid cone, which reaches past Z = 0), or u or v not finite.
// rectified_points rounds (u, v) to binary32, (NaN, NaN) without a projection.  The map's entry at the integer position (i, j) is
//   mx = floor(u 32 + 1/2),  my = floor(v 32 + 1/2)  in binary64, kept if 0 <= mx <= 32 (src_w - 1) and 0 <= my <= 32 (src_h - 1);
//   else, and without a projection, both words are RECT_NONE (AGX_MAP_NONE).
// The remap has no floating-point operation.  An entry outside the source (AGX_MAP_NONE among them) gives `border`; else
//   x0 = mx >> 5, ax = mx & 31, x1 = min(x0 + 1, src_w - 1), the same in y,
//   value = ((32 - ax)(32 - ay) p00 + ax (32 - ay) p10 + (32 - ax) ay p01 + ax ay p11 + 512) >> 10   in uint32
//   (65535 x 1024 + 512 < 2^32).  Both forms go through remap_tap and remap_blend: byte equality is a matter of indices only.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/aprilgrid_amd.h"
#include "board_pose_math.h"

namespace agx {

constexpr int32_t RECT_NONE = AGX_MAP_NONE;
constexpr int RECT_MAX_SIDE = 16384;  // of the source and the target of a map, of the target of a remap

struct RectifyGeom {
    agx_camera cam;
    double nfx, nfy, ncx, ncy;  // new_camera
    double R[9];                // row major, rectified frame -> camera frame
};

// false: the point has no projection (u, v untouched or not finite)
template <int LENS>
AGX_HD bool rectify_point(const RectifyGeom &g, double x, double y, double &u, double &v)
{
    const double dx = (x - g.ncx) / g.nfx, dy = (y - g.ncy) / g.nfy;
    const double X = g.R[0] * dx + g.R[1] * dy + g.R[2];
    const double Y = g.R[3] * dx + g.R[4] * dy + g.R[5];
    const double Z = g.R[6] * dx + g.R[7] * dy + g.R[8];
    const Pose p = {{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, {0.0, 0.0, Z}};
    PosePointOf<LENS> q;
    if (!pose_project<LENS>(g.cam, p, X, Y, q)) return false;
    u = q.u;
    v = q.v;
    return f64_finite(u) && f64_finite(v);
}

// the map's entry from a projection
AGX_HD void rectify_entry(bool ok, double u, double v, int src_w, int src_h, int32_t &mx, int32_t &my)
{
    mx = my = RECT_NONE;
    if (!ok) return;
    const double qx = __builtin_floor(u * 32.0 + 0.5), qy = __builtin_floor(v * 32.0 + 0.5);
    if (!(qx >= 0.0 && qx <= (double)(32 * (src_w - 1)) && qy >= 0.0 && qy <= (double)(32 * (src_h - 1)))) return;
    mx = (int32_t)qx;
    my = (int32_t)qy;
}

// rectified_points' answer for one point
template <int LENS>
AGX_HD void rectify_point_f32(const RectifyGeom &g, float x, float y, float &u, float &v)
{
    double ud, vd;
    if (rectify_point<LENS>(g, (double)x, (double)y, ud, vd)) {
        u = (float)ud;
        v = (float)vd;
    } else {
        u = v = f32_from_bits(0x7fc00000u);
    }
}

// what one map entry means for every frame of a batch: the byte offsets of its two source rows at x0, the step to x1, the weights.
// An entry outside the source reads pixel (0, 0) and is not used (ok false).
struct RemapTap {
    uint32_t off0, off1;  // bytes from the frame's first pixel to (x0, y0) and (x0, y1); a frame is below 2^31 bytes
    uint32_t xstep;       // bytes from x0 to x1: the pixel's size, or 0 on the last column
    uint32_t ax, ay;      // 0 .. 31
    bool ok;
};

AGX_HD RemapTap remap_tap(int32_t mx, int32_t my, int src_w, int src_h, uint32_t row_stride, uint32_t px_bytes)
{
    RemapTap t;
    t.ok = mx >= 0 && my >= 0 && mx <= 32 * (src_w - 1) && my <= 32 * (src_h - 1);
    const uint32_t ux = t.ok ? (uint32_t)mx : 0u, uy = t.ok ? (uint32_t)my : 0u;
    const uint32_t x0 = ux >> 5, y0 = uy >> 5;
    const uint32_t y1 = y0 + 1u < (uint32_t)src_h ? y0 + 1u : y0;
    t.ax = ux & 31u;
    t.ay = uy & 31u;
    t.xstep = x0 + 1u < (uint32_t)src_w ? px_bytes : 0u;
    t.off0 = y0 * row_stride + x0 * px_bytes;
    t.off1 = y1 * row_stride + x0 * px_bytes;
    return t;
}

// T = uint8_t (AGX_L8) or uint16_t (AGX_L16); frame -> the frame's first pixel
template <typename T>
AGX_HD uint32_t remap_blend(const unsigned char *frame, const RemapTap &t, uint32_t border)
{
    const uint32_t p00 = *reinterpret_cast<const T *>(frame + t.off0), p10 = *reinterpret_cast<const T *>(frame + t.off0 + t.xstep);
    const uint32_t p01 = *reinterpret_cast<const T *>(frame + t.off1), p11 = *reinterpret_cast<const T *>(frame + t.off1 + t.xstep);
    const uint32_t bx = 32u - t.ax, by = 32u - t.ay;
    const uint32_t v = (bx * by * p00 + t.ax * by * p10 + bx * t.ay * p01 + t.ax * t.ay * p11 + 512u) >> 10;
    return t.ok ? v : border;
}

// what both forms refuse in the rectification's own arguments (agx_board_pose_enqueue_m's rules on the lens model and the camera;
// new_camera finite with fx' and fy' > 0; rotation null or finite); fills g
inline bool rectify_geom(int lens, const double *camera, const double *new_camera, const double *rotation, RectifyGeom &g)
{
    if (!camera || !new_camera) return false;
    const double *c = camera;
    g.cam = agx_camera{c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8]};
    if (!pose_args_ok(lens, g.cam, 1.0, 0)) return false;
    g.cam = pose_camera(lens, g.cam);  // (the double-sphere model's w2: once per call, for the kernel and the host form)
    for (int i = 0; i < 4; ++i)
        if (!f64_finite(new_camera[i])) return false;
    if (!(new_camera[0] > 0.0) || !(new_camera[1] > 0.0)) return false;
    g.nfx = new_camera[0];
    g.nfy = new_camera[1];
    g.ncx = new_camera[2];
    g.ncy = new_camera[3];
    for (int i = 0; i < 9; ++i) {
        g.R[i] = rotation ? rotation[i] : (i % 4 == 0 ? 1.0 : 0.0);
        if (!f64_finite(g.R[i])) return false;
    }
    return true;
}

}  // namespace agx
