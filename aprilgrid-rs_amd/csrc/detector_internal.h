// detector_internal.h -- library-internal accessors of a detector handle (not part of the ABI).
#pragma once
#include "../../include/aprilgrid_amd.h"

extern "C" {
// hipStream_t the detector's kernels are enqueued on (its own stream, or the caller's after
// agx_detector_set_stream) and its device ordinal.
void *agx_internal_stream(agx_detector *det);
int agx_internal_device(const agx_detector *det);
// agx_detect_batch: the detector's worker pool (created on first use, resized when n_threads
// changes), its family table (agx::FamilyInfo), max_num_of_boards and a device staging buffer of
// at least `bytes` (grown on demand).
void *agx_internal_pool(agx_detector *det, int n_threads);
const void *agx_internal_family(const agx_detector *det);
int agx_internal_max_boards(const agx_detector *det);
void *agx_internal_stage(agx_detector *det, size_t bytes);
// Wait for whatever is enqueued and forget it (an error path between enqueue and fetch).
void agx_internal_abandon_batch(agx_detector *det);
#define AGX_UPLOAD_STREAMS 3
int agx_internal_upload_streams(agx_detector *det, void **streams /* [AGX_UPLOAD_STREAMS] */);  // hipError_t
// u8 luma of a chunk of L16 / RGB8 device frames, computed on the device and copied to pinned host
// memory behind the detector's stream ([n_frames][H][W] at *h_out once the stream has been waited for);
// the staging is a ring of n_slots chunks of chunk_capacity_frames
int agx_internal_chunk_luma8(agx_detector *det, const void *d_frames, int n_frames, int width, int height, size_t row_stride,
                             size_t frame_stride, int format, int slot, int n_slots, size_t chunk_capacity_frames,
                             const uint8_t **h_out, const uint8_t **d_out);  // (h_out null: no copy to the host; d_out: where it is on the device)
// the last batch's compact list in the detector's pinned host mirror (valid until the next enqueue) + per-frame
// counts / offsets / status; waits for the device
int agx_internal_fetch_compact(agx_detector *det, const agx_saddle **records, uint32_t *counts, uint32_t *offsets, int *status);
// option "device_tail": board search + decode of the enqueued batch on the device (tail_kernels.hip); the results in mapped
// pinned host memory after agx_internal_fetch_tail: tags[f * *tag_cap ..] (the rows' stride, >= the cap that was enqueued), table[4 f] = count, table[4 f + 1] = agx::TAIL_* status (+ 2: the frame's 100 MHz ticks, + 3: saddles | seeds << 16)
int agx_internal_device_tail(agx_detector *det);
int agx_internal_tail_prepare(agx_detector *det);  // one-time set-up on the handle's device (code list, kernel attributes): all or nothing
int agx_internal_tail_debug(const agx_detector *det);  // AGX_TAIL_DEBUG as read when the handle was created
// to_device != 0 (agx_detect_batch_enqueue_to): tags and table go to a pair of device buffers instead, read by
// agx_internal_publish_tags and agx_internal_device_tail_table
int agx_internal_enqueue_tail(agx_detector *det, const void *d_luma, size_t luma_row_stride, size_t luma_frame_stride, uint32_t tag_cap,
                              int to_device);
int agx_internal_fetch_tail(agx_detector *det, const agx_tag **tags, const uint32_t **table, uint32_t *tag_cap);
void agx_internal_tail_stats(agx_detector *det, int frames, int fallbacks, int uncertain);
// agx_detect_batch_enqueue_to: the device tail's results of the batch (device buffers) into the caller's layout, behind the
// tail on the detector's stream (tail_kernels.hip, k_publish_tags); the device address of the tail's frame table [n][4]
int agx_internal_publish_tags(agx_detector *det, uint32_t cap_per_frame, agx_tag *d_tags, uint32_t *d_counts, int *d_status);
const uint32_t *agx_internal_device_tail_table(agx_detector *det);
// agx_detect_batch_fetch: pinned host memory of at least `bytes` for the u8 luma of the frames the host tail takes (grown on
// demand, guarded like every side buffer)
uint8_t *agx_internal_fetch_luma(agx_detector *det, size_t bytes);
}
namespace agx {
// agx_format: bytes between horizontally adjacent pixels (0: not a format), the rows a frame of `height` spans (the planar
// layout: three planes), the layouts the front-end kernel converts (k_front_luma) and which of those have 16-bit channels
inline int format_px_bytes(int f)
{
    switch (f) {
    case AGX_L8: case AGX_RGB8P: return 1;
    case AGX_L16: case AGX_LA8: return 2;
    case AGX_RGB8: case AGX_BGR8: return 3;
    case AGX_LF32: case AGX_RGBA8: case AGX_BGRA8: case AGX_LA16: return 4;
    case AGX_RGB16: return 6;
    case AGX_RGBA16: return 8;
    default: return 0;
    }
}
inline size_t format_rows(int f, int height) { return (size_t)height * (f == AGX_RGB8P ? 3u : 1u); }
inline bool format_front(int f) { return f >= AGX_LA8 && f <= AGX_RGBA16; }
inline bool format_16bit(int f) { return f == AGX_L16 || f == AGX_LA16 || f == AGX_RGB16 || f == AGX_RGBA16; }
void destroy_worker_pool(void *pool);
void *create_worker_pool(int n_threads);
struct TailWorkers;  // host_tail.hpp
TailWorkers *create_tail_workers(int n_threads);  // nullptr for n_threads <= 1
void destroy_tail_workers(TailWorkers *w);

// agx_detect_batch_enqueue / _enqueue_to: what agx_detect_batch_fetch needs of the batch in flight.  Any enqueue of the chain
// (either pair, agx_detect_batch, agx_detect) resets it: one batch in flight per handle, the last one enqueued.
struct DetectPending {
    int kind = 0;              // 0 none, 1 results to host arrays (agx_detect_batch_enqueue), 2 to the caller's device arrays
    bool device_tail = false;  // the device tail runs behind the chain; else the fetch runs the host tail on every frame
    int n_frames = 0, width = 0, height = 0;
    uint32_t cap = 0;
    const uint8_t *d_luma = nullptr;  // the batch's u8 luma on the device: the L8 frames themselves or the k_luma8 planes
    size_t luma_row = 0, luma_frame = 0;
    agx_tag *d_tags = nullptr;  // kind 2: [n_frames][cap]
    uint32_t *d_counts = nullptr;
    int *d_status = nullptr;
};
int detect_enqueue_impl(agx_detector *det, const void *d_frames, int n_frames, int width, int height, size_t row_stride_bytes,
                        size_t frame_stride_bytes, int format, uint32_t cap_per_frame, bool to_device, agx_tag *d_tags,
                        uint32_t *d_counts, int *d_status);
int detect_fetch_impl(agx_detector *det, agx_tag *out, uint32_t *counts, int *frame_status, int n_threads);
}
extern "C" agx::DetectPending *agx_internal_detect_pending(agx_detector *det);
