// decimate.h -- host-visible interface of decimate.hip: a batch of L8 / L16 frames averaged down by an integer factor (k_decimate)
// and the host form.  The arithmetic is decimate_math.h's for both.  Internal to the library; the public boundary is
// include/aprilgrid_amd.h.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/aprilgrid_amd.h"
#include "decimate_math.h"

namespace agx {

constexpr int DECIMATE_PX = 4;  // adjacent output pixels per lane: one dword (L8) or two (L16) per store

struct DecimateArgs {
    const void *src;  // [n_frames] frames of src_w x src_h
    int n_frames, src_w, src_h;
    size_t src_row_stride, src_frame_stride;  // bytes
    int format;                               // AGX_L8 or AGX_L16
    int factor;                               // DECIMATE_MIN_FACTOR .. DECIMATE_MAX_FACTOR
    void *dst;                                // [n_frames] frames of (src_w / factor) x (src_h / factor)
    size_t dst_row_stride, dst_frame_stride;  // bytes
};

inline int decimate_out_w(const DecimateArgs &a) { return a.src_w / a.factor; }
inline int decimate_out_h(const DecimateArgs &a) { return a.src_h / a.factor; }

// what both forms refuse (null: nothing) -- the text of the AGX_ERR_ARG; the format is the caller's to check first
const char *decimate_args_bad(const DecimateArgs &a);

// device pointers; hipError_t.  Arguments as checked by decimate_args_bad.
int launch_decimate(const DecimateArgs &a, void *stream);

// the same on host memory
void decimate_host(const DecimateArgs &a);

}  // namespace agx
