// render.h -- host-visible interface of render.hip: the printed board through a pose and a lens model into a batch of L8 / L16
// frames, with the projected tag corners as ground truth (k_render_boards), and the host form.  The arithmetic is render_math.h's
// for both.  Internal to the library; the public boundary is include/aprilgrid_amd.h.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/aprilgrid_amd.h"
#include "render_math.h"

namespace agx {

constexpr int RENDER_PX = 4;  // adjacent pixels of a row per lane: one dword (L8) or two (L16) per store

struct RenderArgs {
    int lens;  // AGX_LENS_*
    RenderGeom g;
    int n_frames, width, height;  // sides 1 .. RENDER_MAX_SIDE
    size_t row_stride, frame_stride;  // bytes; row_stride * height < 2^31
    int format;                       // AGX_L8 or AGX_L16
    int family;                       // agx_family: its code table is read at first_id .. first_id + rows cols - 1
    const double *poses;              // [n_frames][12]: R row major, then t
    void *frames;
    agx_tag *truth;     // [n_frames][rows cols]
    uint32_t *n_truth;  // [n_frames]
    uint32_t *status;   // [n_frames] AGX_RENDER_*
};

// the family's cell layout and the length of its code table; false: no such family
bool render_family(int family, int &edge, int &border, uint32_t &n_codes);

// what every form refuses (null: nothing) -- the text of the AGX_ERR_ARG.  p: the caller's parameters, as given
const char *render_args_bad(const RenderArgs &a, const agx_camera &camera, const agx_render_params &p, bool device);

// device pointers; hipError_t.  Arguments as checked by render_args_bad.
int launch_render_boards(const RenderArgs &a, void *stream);

// the same on host memory
void render_boards_host(const RenderArgs &a);

}  // namespace agx
