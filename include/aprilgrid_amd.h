/*
 * aprilgrid_amd.h -- C ABI of the MI355X-native AprilGrid saddle/tag detection path.
 *
 * This is the drop-in boundary for the Rust crate `aprilgrid` 0.8.0: every entry point
 * below names the reference item (file:line under the crate root) it replaces, and a Rust
 * shim binds them 1:1.  Plain pointers and sizes only -- no C++, torch or
 * HIP types cross this line (a HIP stream is passed as an opaque void*).
 *
 * Conventions
 *   - every function returns AGX_OK (0) or a negative agx_status; nothing unwinds across
 *     the boundary: every entry point catches (std::bad_alloc, a failed std::thread ->
 *     AGX_ERR_NOMEM; tests/test_abi_cpu.py forces both) (the reference's panics -- detector.rs:500 "Only support u8c1 and u8c3",
 *     the height()-1 underflow at detector.rs:174 -- become AGX_ERR_FORMAT / AGX_ERR_ARG);
 *   - the caller owns every buffer it passes; results are copied into caller memory;
 *   - "nothing found" is AGX_OK with a zero count (reference: empty Vec / HashMap);
 *   - a detector handle owns one device, one stream and its scratch planes: it is NOT
 *     re-entrant.  The reference's `&self` methods are callable from many threads; a shim
 *     keeps that property by pooling handles (one per calling thread);
 *   - results never come from a CPU fallback: if the HIP runtime or a gfx950 device is
 *     missing, agx_detector_create fails with AGX_ERR_NO_DEVICE.
 */
#ifndef APRILGRID_AMD_H
#define APRILGRID_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AGX_ABI_VERSION 1

typedef enum agx_status {
    AGX_OK = 0,
    AGX_ERR_ARG = -1,       /* null pointer, zero size, w or h < 2, bad stride            */
    AGX_ERR_FORMAT = -2,    /* pixel format / channel count the reference panics on; agx_detect /
                               agx_luma8 on AGX_LF32 (no u8 luma to derive: agx_detect_planes)     */
    AGX_ERR_CAPACITY = -3,  /* an output or internal list overflowed; nothing is truncated
                               silently -- raise the capacity (agx_detector_set_limits)    */
    AGX_ERR_HIP = -4,       /* a HIP runtime call failed; see agx_last_error              */
    AGX_ERR_NO_DEVICE = -5, /* no usable gfx950 device                                    */
    AGX_ERR_FAMILY = -6,    /* unknown tag family (TagFamily::from_str Err)               */
    AGX_ERR_STATE = -7,     /* call sequence error (e.g. fetch before enqueue); an unexpected internal error */
    AGX_ERR_NOMEM = -8      /* a host allocation or the creation of a worker thread failed: the WHOLE call
                               failed, no per-frame result of it is valid                  */
} agx_status;

/* tag_families::TagFamily -- src/tag_families.rs:5-13 */
typedef enum agx_family {
    AGX_T16H5 = 0,
    AGX_T25H7 = 1,
    AGX_T25H9 = 2,
    AGX_T36H11 = 3,
    AGX_T36H11B1 = 4 /* 1-bit border */
} agx_family;

/* The three DynamicImage variants the reference's tests, benches and detect_kornia feed the
 * path (src/detector.rs:409,507,478-503): ImageLuma8, ImageLuma16, ImageRgb8 (HWC) -- their luma
 * conversion (image crate to_luma32f) is fused into the blur kernel -- and, for every other
 * variant, the caller's own img.to_luma32f() plane (AGX_LF32).
 * AGX_LA8 .. AGX_RGBA16: the other integer variants (ImageLumaA8, ImageRgba8, ImageLumaA16, ImageRgb16, ImageRgba16) and the
 * layouts GPU producers hand over (BGR / BGRA of OpenCV-style decoders, channel-first planes of tensor image decoders).  A
 * front-end kernel writes the frame's integer luma plane -- alpha is ignored; colour is (2126 R + 7152 G + 722 B) / 10000 in
 * unsigned 32-bit arithmetic, the image crate's to_luma8 (8-bit) / its 16-bit counterpart -- and the L8 / L16 chain runs on
 * that plane: to_luma32f of an integer colour image is that integer luma / 255 (/ 65535).  to_luma8 of the 16-bit ones is
 * (luma16 + 128) / 257, as for AGX_L16.  Every entry point that takes a format takes them, batches and single frames alike.
 * The f32 colour variants (Rgb32F, Rgba32F) stay with agx_detect_planes: nothing in this project records their arithmetic. */
typedef enum agx_format {
    AGX_L8 = 0,   /* 1 byte / pixel                                    */
    AGX_L16 = 1,  /* 2 bytes / pixel, native endian                    */
    AGX_RGB8 = 2, /* 3 bytes / pixel, interleaved R,G,B (kornia Image<u8,3>) */
    AGX_LF32 = 3, /* 4 bytes / pixel: row-major f32 luma in [0,1] = DynamicImage::to_luma32f
                     (src/detector.rs:409) as the caller computed it; taken as is */
    AGX_LA8 = 4,   /* 2 bytes / pixel: L,A                              */
    AGX_RGBA8 = 5, /* 4 bytes / pixel: R,G,B,A                          */
    AGX_BGR8 = 6,  /* 3 bytes / pixel: B,G,R                            */
    AGX_BGRA8 = 7, /* 4 bytes / pixel: B,G,R,A                          */
    AGX_RGB8P = 8, /* 1 byte / pixel in three planes R,G,B: plane c of a frame starts c * height * row_stride_bytes behind
                      the frame's start (a frame spans 3 * height rows; channel-first [N,3,H,W] tensors) */
    AGX_LA16 = 9,  /* 4 bytes / pixel: L,A as u16; the 16-bit layouts are native endian and 2-byte aligned, as AGX_L16 */
    AGX_RGB16 = 10, /* 6 bytes / pixel: R,G,B as u16                    */
    AGX_RGBA16 = 11 /* 8 bytes / pixel: R,G,B,A as u16                  */
} agx_format;

/* detector::DetectorParams -- src/detector.rs:25-41 */
typedef struct agx_params {
    float tag_spacing_ratio; /* kept for layout parity; unused by the reference too (:621) */
    float min_saddle_angle;
    float max_saddle_angle;
    uint8_t max_num_of_boards;
} agx_params;

/* saddle::Saddle -- src/saddle.rs:3-9 ; repr(C) {p.0, p.1, k, theta, phi}, 20 bytes */
typedef struct agx_saddle {
    float x, y, k, theta, phi;
} agx_saddle;

/* one entry of detect()'s HashMap<u32, [(f32,f32);4]> -- src/detector.rs:505,520 */
typedef struct agx_tag {
    uint32_t id;
    float xy[8]; /* 4 corners (x,y), in the order the reference returns (:467-470) */
} agx_tag;

typedef struct agx_detector agx_detector; /* opaque; mirrors detector::TagDetector */

/* TagFamily::from_str -- src/tag_families.rs:15-28.  Accepts "t36h11"/"T36H11" etc. */
int agx_family_from_str(const char *name, int *family_out);

/* DetectorParams::default_params -- src/detector.rs:33-40 : (0.3, 30, 60, 2) */
void agx_default_params(agx_params *out);

/* TagDetector::new(tag_family, optional_detector_params) -- src/detector.rs:364-406.
 * params may be NULL (== None).  device = HIP device ordinal.  The constants the
 * reference recomputes on every call (blur weights image_util.rs:111-124, cone kernel and
 * pseudo-inverse detector.rs:208-254) are computed once here. */
int agx_detector_create(int family, const agx_params *params, int device, agx_detector **out);
void agx_detector_destroy(agx_detector *det);

/* Family facts of TagDetector::new's table (edge, border, hamming_distance, code_list). */
int agx_detector_family_info(const agx_detector *det, int *edge_bits, int *border_bits,
                             int *hamming_distance, const uint64_t **codes, int *n_codes);

/* Internal list capacities per frame (0 = keep default).  Defaults scale with the frame:
 * candidates W*H/2, clusters W*H/8, saddles W*H/64 (lists of up to 16384 saddles are ordered in
 * LDS, longer ones -- pure-noise frames of several megapixels -- in global memory).
 * Overflow of any of them
 * is reported as AGX_ERR_CAPACITY for that frame, never truncated.  An explicit limit is taken as given, however small (the
 * floors of the defaults, 4096 / 1024 / 256, apply to the defaults only).  What each limit must cover for a frame to succeed
 * (a limit equal to the count changes nothing; one below voids that frame and no other -- tests/test_gpu_list_limits.py):
 *   max_saddles     the frame's saddles after the k / phi filter; one short: AGX_FRAME_SADDLE_OVERFLOW alone
 *   max_clusters    the frame's flood seeds -- candidate pixels that may start a cluster, at least one per cluster and a few per
 *                   cent more (AGX_DBG_COUNTERS word 1) -- on every path: the seed list shares this limit with the cluster list
 *                   behind it and is the longer of the two; one short: AGX_FRAME_CANDIDATE_OVERFLOW (the seed appends' bit)
 *   max_candidates  the pixels below the frame's threshold, only where the generic kernels cluster the frame ("force_generic",
 *                   or a component beyond the flood windows: AGX_FRAME_GENERIC_PATH); one short: AGX_FRAME_CANDIDATE_OVERFLOW */
int agx_detector_set_limits(agx_detector *det, uint32_t max_candidates, uint32_t max_clusters,
                            uint32_t max_saddles);

/* Tuning / test switches (integers by name):
 *   "force_generic"        1 = cluster every frame with the generic union-find kernels instead
 *                          of the windowed flood fill (results are identical; test hook)
 *   "k1_rows_per_segment"  rows one wave of the blur kernel walks (0 = automatic)
 *   "sparse_path"          how a batch's sparse stages (verify, clusters, refinement, emission) are launched: 0 = by batch size
 *                          (default), 1 = three batch-wide launches, 2 = one 1024-thread workgroup per frame for all of it,
 *                          3 = the verify launch, then one workgroup per frame for the rest (what batches that fill the chip
 *                          take by themselves).  Results are identical on every path (tests/test_gpu_sparse_paths.py).  At a
 *                          chain half_size_patch other than 2 (agx_detector_set_half_size_patch; 2 under "chain_refine_general")
 *                          the values 2 and 3 stay accepted, but such a batch runs as launches of its own whatever the option says,
 *                          and "last_sparse_path" reads 1
 *   "chain_refine_general" 1 = the chain at half_size_patch 2 refines by the kernel of the other sizes (k_refine_clusters, behind
 *                          flood stages that only cluster) instead of inside the flood stages; byte-identical lists.  Default 0;
 *                          the counterpart of "refine_general_kernel", for tests and measurements
 *   "store_response"       1 = the blur kernel also stores the Hessian response it evaluates in
 *                          registers (parity tests: agx_debug_fetch AGX_DBG_RESP); slower
 *   "profile_stride"       with agx_profile_enable(det, 1): time the blur kernel of every n-th batch
 *                          only (an event pair costs the stream two ~5 us gaps around the kernel)
 *   "profile_kernel"       with agx_profile_enable(det, 1): which of the AGX_N_KERNELS launches is timed (0 = the blur
 *                          kernel, the default).  One kernel at a time keeps its neighbours back to back on the
 *                          stream, so the figure is the kernel's own duration; level 2 (all at once) opens a gap
 *                          in front of every kernel
 *   "reload_tuning_env"    (any value) the AGX_* measurement overrides of the environment (AGX_K1_ROWS, AGX_SPARSE_PATH, ...:
 *                          README.md "Tuning switches") are read once per process and kept; this forgets them, so that a
 *                          tool which changes its environment between runs of one process sees the change
 *   "tail_threads"         n > 1: agx_detect / agx_detect_planes / agx_detect_from_saddles search the boards of
 *                          ONE frame on n host threads (the up-to-30 seed saddles of try_find_best_board,
 *                          detector.rs:611-625, in waves of n, merged in the reference's order: same result;
 *                          latency of a single detect, at the price of host cores).  Default 1, like the
 *                          reference; agx_detect_batch parallelises over frames instead
 *   "device_tail"          agx_detect_batch's board search + decode (detector.rs:510-539) on the device, behind the chain
 *                          (csrc/tail_kernels.hip), instead of on the pool of host threads.  -1 (default): for calls of at least four
 *                          frames per host thread (below that the host tail is the faster one), where this process's atan2f is
 *                          glibc's own routine -- the kernel evaluates angle_degree (math_util.rs:31-33) by that routine,
 *                          restated --, else off; 1: on for every call, AGX_ERR_STATE where libm differs; 0: off.
 *                          The tags are the host tail's bit for bit either way: a frame the kernel cannot decide (an angle
 *                          within 1e-4 degrees of the white-block thresholds, saddle.rs:26-38) or hold (more than 1024 saddles,
 *                          128 board cells ...) is handed to the host tail.  Read back: "last_device_tail_frames",
 *                          "last_device_tail_fallbacks", "last_device_tail_uncertain" of the last agx_detect_batch call
 *   "tail_debug_band"      test hook of the hand-back path: n > 0 makes the device tail treat a white-block angle within n / 1000
 *                          degrees of 60 / 120 as undecided (the kernel's own band is 1e-4 degrees, which the suite's frames never
 *                          hit), so that a known share of frames takes the host tail; results unchanged
 *                          (tests/test_gpu_device_tail.py).  0 (default) = off
 *   "debug_ablation"       measurement switches of the kernels (tools/): bits 1 .. 1024 remove parts of the blur kernel's
 *                          work -- timing experiments, results are INVALID; bits 128 / 2048 / 8192 / 16384 collect
 *                          statistics and phase times (AGX_DBG_VERIFY_STATS), 4096 the start and end of every wave of
 *                          the sparse kernels (AGX_DBG_WAVE_TIMES), 32768 selects the blur kernel's former ascending
 *                          segment order, 65536 its former refresh interval, 131072 / 262144 stage and phase times of the
 *                          workgroup-per-frame kernel (tools/sparse_frame_phases.py, tools/flood_phases.py): results unchanged
 *                          (tests/test_gpu_parity.py) */
int agx_detector_set_option(agx_detector *det, const char *name, int value);
/* Read an option back; additionally the tiling the blur kernel used for the last enqueued batch:
 * "k1_rows_per_segment" (effective value), "k1_segments", "k1_strips", "k1_strip_columns", and
 * "last_sparse_path": how the last batch's sparse stages ran: 1 = the three launches, 2 = one workgroup per frame for all
 * of it, 3 = the verify launch, then a workgroup per frame (the values of option "sparse_path"); and
 * "last_chain_refine": 0 = the last chain batch refined inside the flood stages (half_size_patch 2), 1 = it ran the deferred
 * refinement, k_refine_clusters (agx_detector_set_half_size_patch); and, with agx_profile_enable(det, 2),
 * "last_clusters_front_us" / "last_clusters_emit_us": the device time of k_plane_front's two launches and of k_emit_clusters of the
 * last agx_clusters_enqueue batch, and "last_response_front_us": that of k_response_front's two launches of the last chain batch
 * at a sigma other than 1.5 -- each as of the last fetch, agx_detector_sync or agx_profile_read behind that batch (microseconds;
 * tools/bench_clusters.py). */
int agx_detector_get_option(const agx_detector *det, const char *name, int *value);

/* The sigma of the chain's blur (src/detector.rs:410 hard-codes 1.5f, the default here).  Per-handle state; it applies from the
 * next enqueue on to every entry that runs the chain on this handle: agx_refined_saddle_points, agx_detect, agx_detect_planes,
 * agx_saddles_batch_enqueue[_to], agx_detect_batch, agx_detect_batch_enqueue[_to], agx_refine_points_enqueue with
 * AGX_REFINE_BLURRED, and a group's ranks through agx_group_detector(group, r).  sigma as agx_planes_enqueue's when positive:
 * finite, > 0, ceilf(2 sigma) in 1 .. 16; anything else, 0 included, is AGX_ERR_ARG and the stored value stays (so does a NULL
 * det or a NULL sigma).  With the stored value bit-equal to 1.5f the chain starts with its fused seven-tap blur kernel, as it
 * always did; at any other value with k_gauss_blur (the taps of agx_debug_blur_weights(sigma)) and k_response_front, which
 * hand the same products to the unchanged sparse stages: results are the reference's with `1.5` replaced by sigma, bit for
 * bit (tests/test_gpu_sigma.py).  Read-only option "last_chain_front": 0 = the last chain batch ran the fused kernel, 1 = the
 * any-sigma front. */
int agx_detector_set_blur_sigma(agx_detector *det, float sigma);
int agx_detector_get_blur_sigma(const agx_detector *det, float *sigma);

/* rochade_refine's half_size_patch inside the chain (src/detector.rs:430 hard-codes 2, the default here): the patch that goes
 * with the blur.  Per-handle state; it applies from the next enqueue on to the entries agx_detector_set_blur_sigma lists --
 * agx_refined_saddle_points, agx_detect, agx_detect_planes, agx_saddles_batch_enqueue[_to], agx_detect_batch,
 * agx_detect_batch_enqueue[_to], and a group's ranks through agx_group_detector(group, r) -- EXCEPT the refine-points entries:
 * agx_refine_points_enqueue and agx_rochade_refine keep refining at 2 whatever this value is, and their _h forms keep taking
 * their own argument.  Anything outside 1 .. 4 is AGX_ERR_ARG and the stored value stays (so does a NULL det or a NULL out
 * pointer); a batch in flight is never touched.  At 2 the chain is what it always was: the flood stages refine the clusters they
 * find.  At 1, 3 and 4 (and at 2 under option "chain_refine_general") the flood stages only cluster, and k_refine_clusters --
 * sixteen lanes to a cluster, the arithmetic of agx_refine_points_enqueue_h -- refines every frame's cluster table on its blur
 * plane before the unchanged emission: results are the reference's with `2` replaced (and `1.5` by the handle's sigma), x, y and k
 * bit for bit (tests/test_gpu_patch.py).  A cluster whose (4h+1) x (4h+1) window leaves the frame gives no saddle, as in the
 * reference.  HIP graphs: the first such batch uploads the kernel's constants, so a captured batch needs one eager batch at a
 * half that takes this path first (as it does for the workspace).  Read-only option "last_chain_refine": 0 / 1. */
int agx_detector_set_half_size_patch(agx_detector *det, int half_size_patch);
int agx_detector_get_half_size_patch(const agx_detector *det, int *half_size_patch);

/* Stream selection.  external != 0: launch on the caller's stream `hip_stream` (hipStream_t as
 * void*; NULL is HIP's legacy default stream) so that the chain is stream-ordered behind the
 * producer of the frames and in front of consumers of the results (e.g. an RCCL gather), and
 * events the caller records bracket the kernels.  external == 0: back to the detector's own
 * non-blocking stream (hip_stream ignored). */
int agx_detector_set_stream(agx_detector *det, void *hip_stream, int external);

/* ---- single frame, host memory in / host memory out ---------------------------------- */

/* TagDetector::refined_saddle_points(&self, img) -> Vec<Saddle> -- src/detector.rs:408-446.
 * pixels: host pointer, row_stride_bytes between rows.  Writes min(*n_out, cap) saddles in
 * the reference's order (clusters by ascending first pixel, raster order); returns
 * AGX_ERR_CAPACITY (with *n_out = required) if cap is too small. */
int agx_refined_saddle_points(agx_detector *det, const void *pixels, int width, int height,
                              size_t row_stride_bytes, int format, agx_saddle *out, uint32_t cap,
                              uint32_t *n_out);

/* TagDetector::detect(&self, img) -> HashMap<u32,[(f32,f32);4]> -- src/detector.rs:505-540,
 * and detect_kornia (:478-503) through format = AGX_L8 / AGX_RGB8.  One entry per distinct
 * id (a later quad with the same id replaces the earlier one, as HashMap::insert). */
int agx_detect(agx_detector *det, const void *pixels, int width, int height,
               size_t row_stride_bytes, int format, agx_tag *out, uint32_t cap, uint32_t *n_out);

/* detect() for ANY DynamicImage variant: the caller hands over the two planes the reference
 * derives from the image itself -- img.to_luma32f() for the saddle chain (src/detector.rs:409) and
 * img.to_luma8() for the code decode (:507, :518) -- so the result does not depend on this
 * library restating the image crate's conversions for that variant. */
int agx_detect_planes(agx_detector *det, const float *luma32f, size_t stride32f_bytes, const uint8_t *luma8,
                      size_t stride8_bytes, int width, int height, agx_tag *out, uint32_t cap, uint32_t *n_out);

/* ---- batches of equally sized frames resident in device memory (HBM) ------------------ */

/* Enqueue the whole saddle chain (luma -> blur -> Hessian response -> min/threshold ->
 * clustering -> rochade_refine -> k/phi filter) for n_frames frames on the detector's
 * stream and return without waiting.  d_frames: DEVICE pointer; frame i starts at
 * d_frames + i*frame_stride_bytes.  Any row stride that covers a row is accepted (16-bit pixels
 * 2-byte aligned); rows and frames aligned to 4 bytes with width % 4 == 0 take the fast path.
 * HIP graphs: the call may be made while the detector's stream is being captured (after one eager
 * batch of the same geometry, so that the workspace exists); every captured batch then clears its
 * own counters, so a graph of any number of batches replays correctly any number of times. */
int agx_saddles_batch_enqueue(agx_detector *det, const void *d_frames, int n_frames, int width,
                              int height, size_t row_stride_bytes, size_t frame_stride_bytes,
                              int format);

/* Wait for the enqueued batch and copy the results out.  out: n_frames * cap_per_frame
 * saddles (frame i at out + i*cap_per_frame); counts[i] = saddles of frame i;
 * frame_status[i] (may be NULL) = AGX_OK or AGX_ERR_CAPACITY.  Returns the first non-OK
 * frame status, else AGX_OK. */
int agx_saddles_batch_fetch(agx_detector *det, agx_saddle *out, uint32_t cap_per_frame,
                            uint32_t *counts, int *frame_status);

/* Same chain, results left in CALLER-OWNED DEVICE memory (nothing is copied to the host), so
 * that they can be consumed or gathered on the device (RCCL):
 *   d_saddles      room for saddle_capacity agx_saddle records; the frames' lists are packed
 *                  back to back in completion order (each list itself in reference order);
 *   d_frame_table  n_frames agx_frame_result entries: where frame i's list starts, its length
 *                  and its status flags (0 = ok; AGX_FRAME_* bits otherwise).
 * A frame whose list does not fit (or whose internal lists overflowed) gets a non-zero
 * status and no records -- never a truncated list. */
typedef struct agx_frame_result {
    uint32_t count;   /* saddles of this frame                     */
    uint32_t offset;  /* index of its first record in d_saddles    */
    uint32_t status;  /* 0 or a combination of AGX_FRAME_* bits    */
    uint32_t n_clusters;
} agx_frame_result;
/* Which overflow sets which bit (agx_detector_set_limits says what each limit must cover):
 *   CANDIDATE_OVERFLOW  the generic path's candidate list beyond max_candidates -- and the flood seed list beyond max_clusters,
 *                       on every sparse path and under "force_generic" alike (a seed is a candidate pixel; the seed appends
 *                       of k_verify_seeds and k_sparse_frame raise this bit, not CLUSTER_OVERFLOW)
 *   CLUSTER_OVERFLOW    the cluster list (flood clusters, the generic path's roots) beyond max_clusters -- reachable only where
 *                       the seed list fitted
 *   SADDLE_OVERFLOW     the frame's saddle list beyond max_saddles, or beyond what is left of a caller-owned slab
 *                       (agx_saddles_batch_enqueue_to: saddle_capacity), and nothing else */
enum {
    AGX_FRAME_CANDIDATE_OVERFLOW = 1,
    AGX_FRAME_CLUSTER_OVERFLOW = 2,
    AGX_FRAME_SADDLE_OVERFLOW = 4,
    AGX_FRAME_CENTROID_INEXACT = 8, /* informational: a cluster's coordinate sum reached 2^24 */
    AGX_FRAME_GENERIC_PATH = 16,    /* informational: clustered by the generic kernels         */
    AGX_FRAME_DENSE_THRESHOLD = 32, /* (unused) */
    AGX_FRAME_LARGE_RESULT = 64     /* informational: more than 1024 refined candidates, emitted by the large-list path */
};
int agx_saddles_batch_enqueue_to(agx_detector *det, const void *d_frames, int n_frames, int width,
                                 int height, size_t row_stride_bytes, size_t frame_stride_bytes,
                                 int format, void *d_saddles, uint32_t saddle_capacity,
                                 void *d_frame_table);

/* Block until everything enqueued on the detector's stream has finished. */
int agx_detector_sync(agx_detector *det);

/* How many host threads this process can keep busy: the smaller of its CPU affinity mask and its
 * cgroup CPU quota (cpu.max / cpu.cfs_quota_us; a container given 16 CPUs of a 256-thread host reports
 * 16), at least 1.  The default thread count of agx_detect_batch: threads beyond a quota make every
 * thread of the process -- the one driving the device included -- sit out the rest of each scheduler
 * period.  (The reference never spawns a thread, src/detector.rs:505; batches are this library's.) */
int agx_host_parallelism(void);
/* Test hook: the CPU-quota half of that rule on a given cgroup mount point and stand-in for /proc/self/cgroup (v2 cpu.max
 * and v1 cpu.cfs_quota_us / cpu.cfs_period_us of the process's cgroup and every ancestor, the smallest, rounded up to whole
 * CPUs); 0 = no quota found.  Nothing is cached. */
int agx_debug_cgroup_cpu_quota(const char *cgroup_root, const char *proc_self_cgroup);

/* TagDetector::detect (src/detector.rs:505-540) over a batch of equally sized frames in HOST memory
 * (frame i at frames + i*frame_stride_bytes; every agx_format but AGX_LF32).  With the device tail (option
 * "device_tail", the default where available) the saddle chain and the board search + decode of a chunk of up to 1024
 * frames run on the device while n_threads host threads (0 = agx_host_parallelism(); the pool lives as long as the
 * detector) upload the next chunk and take the frames the kernel hands back.  With the host tail the saddle
 * chain of a chunk of frames (about one frame per thread, 8 .. 64) runs on the device while the threads upload the next
 * chunks and run the board search + decode of the previous ones; no barrier between chunks.  Same tags either way.
 * d_frames: optional device copy of the same frames (skips the upload), else
 * NULL.  out: n_frames * cap_per_frame tags, frame i at out + i*cap_per_frame; counts[i] = tags of
 * frame i; frame_status[i] (may be NULL) = AGX_OK or AGX_ERR_CAPACITY.  Returns the first non-OK
 * frame status, else AGX_OK. */
int agx_detect_batch(agx_detector *det, const void *frames, const void *d_frames, int n_frames, int width,
                     int height, size_t row_stride_bytes, size_t frame_stride_bytes, int format, agx_tag *out,
                     uint32_t cap_per_frame, uint32_t *counts, int *frame_status, int n_threads);

/* detect (src/detector.rs:505-540) over a batch resident in DEVICE memory; layout and formats as
 * agx_saddles_batch_enqueue (every agx_format but AGX_LF32, which is AGX_ERR_FORMAT).  Enqueues the chain, to_luma8 (non-L8,
 * on the device; for AGX_LA8 .. AGX_RGB8P the front-end kernel's plane is that plane) and the device tail on the detector's stream and returns without waiting; the frames must stay in place until
 * agx_detect_batch_fetch has returned.  The device tail runs where option "device_tail" is -1 or 1 and this process may use it
 * (no batch-size rule); with 0, or where it is refused, the fetch runs the host tail on every frame from the compact saddle lists
 * and the u8 luma planes copied down.  Same tags, counts and statuses as agx_detect_batch on the same pixels, either way.
 * One batch in flight per handle, as for agx_saddles_batch_enqueue: any later enqueue (either pair, agx_detect_batch, agx_detect)
 * replaces it; agx_saddles_batch_fetch of it, or agx_detect_batch_fetch of a saddle batch, is AGX_ERR_STATE. */
int agx_detect_batch_enqueue(agx_detector *det, const void *d_frames, int n_frames, int width, int height,
                             size_t row_stride_bytes, size_t frame_stride_bytes, int format, uint32_t cap_per_frame);
/* The same, results also in CALLER-OWNED DEVICE memory (4-byte aligned): d_tags [n_frames][cap_per_frame] agx_tag (may be NULL
 * for cap 0), d_counts [n_frames] uint32, d_status [n_frames] int (agx_status per frame, as agx_detect_batch's frame_status).
 * Only a frame's own count of rows is written; more tags than cap_per_frame is AGX_ERR_CAPACITY with the true count and no row.
 * A frame the device tail hands back to the host tail reads count 0 and AGX_ERR_STATE until agx_detect_batch_fetch has written
 * its rows, count and status (on the detector's stream, before it returns); without the device tail that is every frame. */
int agx_detect_batch_enqueue_to(agx_detector *det, const void *d_frames, int n_frames, int width, int height,
                                size_t row_stride_bytes, size_t frame_stride_bytes, int format, agx_tag *d_tags,
                                uint32_t cap_per_frame, uint32_t *d_counts, int *d_status);
/* Wait; resolve the frames the kernel handed back on n_threads host threads (0 = agx_host_parallelism()); out / counts /
 * frame_status as agx_detect_batch (out sized n_frames * the enqueue's cap; frame_status may be NULL).  After _enqueue_to the
 * host arrays may be NULL; the device arrays are final when this returns.  Returns the first non-OK frame status, else AGX_OK;
 * AGX_ERR_STATE with nothing in flight.  The batch is resolved by this call: a second fetch is AGX_ERR_STATE. */
int agx_detect_batch_fetch(agx_detector *det, agx_tag *out, uint32_t *counts, int *frame_status, int n_threads);

/* ---- rochade_refine of caller-given points ---------------------------------------------- */

/* detector::rochade_refine(image_input, initial_corners, half_size_patch) -> Vec<Saddle> -- src/detector.rs:194-361, a `pub fn`
 * of the crate: the sub-pixel refinement of ANY list of corner guesses (last frame's corners, corners predicted from a board
 * homography, another detector's), not only of the centroids the chain's own flood fill produced.  half_size_patch is the last
 * argument of the _h forms below, 1 .. 4 (fitted patch 3x3 .. 9x9, window 5x5 .. 17x17); the forms without it pass 2, the
 * value the reference's detector passes (:430).  The chain's own refinement (agx_refined_saddle_points, the saddle and detect
 * batches) stays at 2, as refined_saddle_points has it.  Every point is answered in its own slot, in input order, with a
 * record and one of these reasons; a rejected point's record is five zero floats. */
struct agx_point {
    float x, y;
}; /* one (f32,f32) of initial_corners -- src/detector.rs:194-361; 8 bytes.  Arrays of them cross the boundary as `const void *`,
      like the saddle records of agx_saddles_batch_enqueue_to: an [n][2] float array is the same memory */
typedef struct agx_point agx_point;
enum { AGX_POINT_REFINED = 0,
       AGX_POINT_OUTSIDE = 1,     /* :266-274: the 9x9 window around round(x), round(y) leaves the image: unless both coordinates
                                     are finite, roundf(x) in [4, W-5] and roundf(y) in [4, H-5].  Decided in float before anything
                                     is converted or read -- NaN, +-inf and values beyond the int range, undefined in the reference
                                     (`as i32`, unchecked indexing), are OUTSIDE; so is every point of a frame smaller than 9x9.
                                     At half_size_patch = h the window is (4h+1)x(4h+1): roundf(x) in [2h, W-1-2h], roundf(y) in
                                     [2h, H-1-2h], and every point of a frame smaller than 4h+1 in either direction is OUTSIDE */
       AGX_POINT_NOT_SADDLE = 2,  /* :331-339: not (d < 0) */
       AGX_POINT_MOVED = 3 };     /* :342-347: |x0| or |y0| > 1, or not |c5| < k */
enum { AGX_REFINE_BLURRED = 0,    /* frames of any agx_format; refined on their blur at the handle's sigma, as
                                     refined_saddle_points does (:409-410, :430) */
       AGX_REFINE_PLANE = 1 };    /* format must be AGX_LF32 (else AGX_ERR_FORMAT): the plane IS image_input, taken as is
                                     (row stride a multiple of 4 bytes); no blur, no workspace plane */

/* rochade_refine (src/detector.rs:194-361) over a batch in DEVICE memory, stream-ordered on the detector's stream (the caller's
 * after agx_detector_set_stream); returns without waiting.  d_frames / n_frames / width / height / strides / format as
 * agx_saddles_batch_enqueue (width, height >= 1).  image: AGX_REFINE_BLURRED or AGX_REFINE_PLANE.  d_points: agx_point records; frame f's are
 * d_points[f*points_per_frame .. + n_f); n_f = d_counts[f] where d_counts is given and that is at most points_per_frame, else
 * points_per_frame.  Point i of frame f writes record and status [f*points_per_frame + i]; slots at or beyond n_f are not
 * written.  d_out ([n_frames*points_per_frame] agx_saddle) and d_status: caller-owned device memory, 4-byte aligned, or both
 * NULL -- internal buffers, copied out by agx_refine_points_fetch.  Frames, points and counts stay in place until the fetch
 * has returned.  A third kind of batch on the handle: one batch is in flight, a later enqueue of any kind replaces it;
 * agx_saddles_batch_fetch / agx_detect_batch_fetch of it are AGX_ERR_STATE.  AGX_ERR_ARG: NULL d_frames or d_points,
 * points_per_frame == 0, exactly one of d_out / d_status NULL, an unknown image. */
int agx_refine_points_enqueue(agx_detector *det, const void *d_frames, int n_frames, int width, int height,
                              size_t row_stride_bytes, size_t frame_stride_bytes, int format, int image,
                              const void *d_points, uint32_t points_per_frame, const uint32_t *d_counts,
                              agx_saddle *d_out, uint32_t *d_status);
/* Wait for the batch of agx_refine_points_enqueue (src/detector.rs:194-361).  Internal buffers: out and status, host arrays of
 * n_frames*points_per_frame entries, receive the slots the batch wrote (slots at or beyond a frame's count stay as they were).
 * Caller-owned device buffers: out and status are NULL, the call only waits.  AGX_ERR_STATE: no such batch in flight (another
 * kind, none, or fetched already). */
int agx_refine_points_fetch(agx_detector *det, agx_saddle *out, uint32_t *status);
/* agx_refine_points_enqueue with rochade_refine's third argument (src/detector.rs:194-361): half_size_patch in 1 .. 4, anything
 * else is AGX_ERR_ARG and leaves a batch in flight where it is.  Every other argument, the batch (the same third kind, fetched by
 * agx_refine_points_fetch) and the records are agx_refine_points_enqueue's, which is this call at 2 and gives the same bytes as
 * it.  AGX_REFINE_BLURRED refines on the blur at the handle's sigma as before: the patch size is chosen by the caller, to go
 * with the sigma or not.  An AGX_REFINE_PLANE plane is read inside a point's own window only.  Option "refine_general_kernel"
 * (0; tests and measurements) = 1 runs half_size_patch 2 on the kernel of the other sizes, with identical results; the
 * read-only option "last_refine_kernel" says which kernel the last refine batch ran (0: the one of 2, 1: the general one). */
int agx_refine_points_enqueue_h(agx_detector *det, const void *d_frames, int n_frames, int width, int height,
                                size_t row_stride_bytes, size_t frame_stride_bytes, int format, int image,
                                const void *d_points, uint32_t points_per_frame, const uint32_t *d_counts,
                                agx_saddle *d_out, uint32_t *d_status, int half_size_patch);
/* rochade_refine (src/detector.rs:194-361) of one image in HOST memory: uploads pixels and points, runs a batch of one, writes
 * record and status of every point (points: n_points agx_point records; out, status: n_points entries each, in input order) and *n_refined, the number of
 * AGX_POINT_REFINED ones: the reference's Vec<Saddle> is those records in input order.  n_points == 0: AGX_OK, *n_refined = 0. */
int agx_rochade_refine(agx_detector *det, const void *pixels, int width, int height, size_t row_stride_bytes, int format,
                       int image, const void *points, uint32_t n_points, agx_saddle *out, uint32_t *status,
                       uint32_t *n_refined);
/* agx_rochade_refine with rochade_refine's third argument (src/detector.rs:194-361): half_size_patch in 1 .. 4, else AGX_ERR_ARG.
 * agx_rochade_refine is this call at 2. */
int agx_rochade_refine_h(agx_detector *det, const void *pixels, int width, int height, size_t row_stride_bytes, int format,
                         int image, const void *points, uint32_t n_points, agx_saddle *out, uint32_t *status,
                         uint32_t *n_refined, int half_size_patch);
/* THE WINDOWED REFINE (k_refine_windows): agx_refine_points_enqueue_h(.., AGX_REFINE_BLURRED, ..) without its blur plane.  Every
 * pixel of gaussian_blur_f32 (src/image_util.rs:110-206) is a function of the input alone, so the (4h+1)^2 blur window of a point
 * is computed from the (4h+1+2r)^2 input pixels around it, r = ceil(2 sigma) at the handle's sigma, clamped to the frame: no
 * plane is allocated, written or read, and the cost follows the points, not the pixels.  Every record and status word equals,
 * byte for byte, what agx_refine_points_enqueue_h writes for the same full-resolution points on the same frames.
 * d_frames / n_frames / width / height / strides as agx_refine_points_enqueue; format AGX_L8, AGX_L16 (pointer and strides 2-byte
 * aligned) or AGX_LF32 (refined on its blur, unlike AGX_REFINE_PLANE); any other is AGX_ERR_FORMAT.  Slot s = f points_per_frame
 * + i reads two floats (x, y) at (char *)d_points + s point_stride_bytes: agx_point rows (8) and agx_saddle records (20) are
 * both read in place.  d_counts as agx_refine_points_enqueue.  d_status_in (optional, [n_frames points_per_frame]): a slot whose
 * word is non-zero is not refined -- its record is five zero floats and its status the word handed on, as the decode stages hand
 * status on.  factor in 1 .. 4: the point (x, y) of a frame decimated by `factor` (agx_decimate_enqueue) is taken to full
 * resolution as x * (float)factor + 0.5f * (factor - 1), one rounded multiply and one rounded add in binary32, the same for y;
 * at 1 the point is taken as it is.  AGX_POINT_OUTSIDE is decided in float before anything is read, by agx_refine_points_enqueue's
 * rule.  d_out and d_status: caller-owned device memory, required.  In place (d_out = d_points at a stride of 20, d_status =
 * d_status_in) is allowed: a slot is read before it is written and by no other slot.  Stream-ordered, nothing to fetch; a batch
 * in flight is replaced as by agx_board_fit_enqueue.
 * AGX_ERR_ARG (a batch in flight stays where it is): a NULL d_frames, d_points, d_out or d_status; points_per_frame == 0;
 * half_size_patch outside 1 .. 4; factor outside 1 .. 4; point_stride_bytes below 8 or no multiple of 4; a misaligned array;
 * agx_refine_points_enqueue's rules on the frames. */
int agx_refine_windows_enqueue(agx_detector *det, const void *d_frames, int n_frames, int width, int height,
                               size_t row_stride_bytes, size_t frame_stride_bytes, int format,
                               const void *d_points, size_t point_stride_bytes, uint32_t points_per_frame,
                               const uint32_t *d_counts, const uint32_t *d_status_in,
                               agx_saddle *d_out, uint32_t *d_status, int factor, int half_size_patch);

/* ---- decimated batches (csrc/decimate.hip; csrc/decimate_math.h) ------------------------- */

/* A batch of AGX_L8 or AGX_L16 frames averaged down by an integer factor f in 2 .. 4 (k_decimate): AprilTag's quad_decimate, the
 * first half of a coarse-to-fine detect (agx_refine_windows_enqueue's `factor` is the second).  d_dst: n_frames frames of
 * floor(width / f) x floor(height / f) in the same format with their own strides; trailing source columns and rows are dropped.
 *   out(X, Y) = (sum of the f x f source pixels at (f X + dx, f Y + dy) + f f / 2) / (f f)      in uint32
 * -- the mean, round half up.  No floating-point operation in the kernel or in the host form.  The centre of output pixel (X, Y)
 * is the source position (f X + (f - 1) / 2, f Y + (f - 1) / 2).  Nothing outside the source rows' width pixels is read, nothing
 * outside the destination rows' floor(width / f) pixels is written.  Caller-owned device memory, stream-ordered, nothing to
 * fetch; a batch in flight is replaced as by agx_board_fit_enqueue.  Source and destination must not overlap.
 * AGX_ERR_FORMAT: a format other than AGX_L8 and AGX_L16 (the luma front is not part of this).  AGX_ERR_ARG (a batch in flight
 * stays where it is): a NULL array; n_frames outside 1 .. 65535; f outside 2 .. 4; width or height below f (an output side of
 * 0) or above 65000, or a frame of 2^30 px or more; a row stride that does not cover a row or is 2^31 or more, a frame stride
 * (n_frames > 1) that does not cover a frame; AGX_L16 pointers or strides that are odd.
 * agx_decimate_tail: the host form -- no handle, no device, the same bytes. */
int agx_decimate_enqueue(agx_detector *det, const void *d_src, int n_frames, int width, int height,
                         size_t row_stride_bytes, size_t frame_stride_bytes, int format, int factor,
                         void *d_dst, size_t dst_row_stride_bytes, size_t dst_frame_stride_bytes);
int agx_decimate_tail(const void *src, int n_frames, int width, int height,
                      size_t row_stride_bytes, size_t frame_stride_bytes, int format, int factor,
                      void *dst, size_t dst_row_stride_bytes, size_t dst_frame_stride_bytes);

/* ---- decode of caller-given quads -------------------------------------------------------- */

/* TagDetector::try_decode_quad(&self, img, quad) -> Option<(usize, [(f32,f32);4])> -- src/detector.rs:448-476 -- built from the
 * crate's pub fns decode_positions (:42-72), bit_code (:74-122) and best_tag (:142-169): which tag is in ANY quad (a tracked
 * board's corners, corners predicted from a pose, agx_refine_points_enqueue's output), without the board search that detect
 * runs to find its quads.  The decode reads to_luma8 of the image; the saddle chain is not run.  Every quad is answered in its
 * own slot, in input order, with an agx_tag, one of these statuses and (optionally) bit_code's value; the agx_tag of a quad
 * that is not AGX_QUAD_DECODED is all zero. */
enum { AGX_QUAD_DECODED = 0,      /* src/detector.rs:448-476: id = index into the family's code list, xy = the input corners
                                     after rotate_left(rotation); reverse() (:467-470) */
       AGX_QUAD_OUTSIDE = 1,      /* a corner coordinate that is not finite (decided first, before anything is read); or
                                     :50-56, a rounded corner with x >= width or y >= height under Rust's saturating `as u32`
                                     (a finite negative coordinate saturates to 0 and is inside, as in the reference); or
                                     :84-93, a sample point outside the image */
       AGX_QUAD_LOW_CONTRAST = 2, /* :97-99: max - min < 50 over the samples */
       AGX_QUAD_AMBIGUOUS = 3,    /* :117-118: more than 3 samples within 10 of the mid brightness */
       AGX_QUAD_NO_MATCH = 4,     /* :160-168: no rotation within the family's Hamming distance of a code */
       AGX_QUAD_SKIPPED = 5,      /* d_point_status was given and one of the quad's corners is not AGX_POINT_REFINED: nothing
                                     of the quad's pixels is read */
       AGX_QUAD_DEGENERATE = 6 }; /* src/image_util.rs:5-37: AGX_TAG_MAP_HOMOGRAPHY refused the quad -- no projective map through
                                     its corners, or the quad is not strictly convex, or its horizon crosses the tag.  Never
                                     produced under AGX_TAG_MAP_AFFINE or by an entry that takes no model */

/* try_decode_quad (src/detector.rs:448-476) over a batch in DEVICE memory, stream-ordered on the detector's stream (the
 * caller's after agx_detector_set_stream); returns without waiting.  d_frames / n_frames / width / height / strides / format
 * as agx_detect_batch_enqueue; AGX_LF32 is AGX_ERR_FORMAT.  L8 frames are read as they are; of every other format the
 * frames' to_luma8 plane is computed on the device first (as agx_detect_batch_enqueue does).
 * Quad q of frame f has four points; point p is two floats (x, y) at
 * d_quads + ((f*quads_per_frame + q)*4 + p) * point_stride_bytes.  point_stride_bytes is a multiple of 4 and at least 8, and
 * d_quads is 4-byte aligned: 8 is a packed [n][4][2] float array, 20 reads agx_saddle records --
 * agx_refine_points_enqueue's d_out with points_per_frame = 4*quads_per_frame is a valid d_quads as it stands.
 * d_point_status: NULL, or that call's d_status, one word per point: a quad with a corner whose word is not
 * AGX_POINT_REFINED is AGX_QUAD_SKIPPED.  d_counts: NULL, or per-frame quad counts as in agx_refine_points_enqueue (a count above
 * quads_per_frame means quads_per_frame; slots at or beyond a frame's count are not written).
 * Results, slot = f*quads_per_frame + q: d_tags[slot], d_status[slot] (AGX_QUAD_*), and, if d_bits is given, d_bits[slot] =
 * bit_code's value before any rotation for AGX_QUAD_DECODED and AGX_QUAD_NO_MATCH slots, 0 for the others.  d_tags and
 * d_status are caller-owned device memory (4-byte aligned; d_bits 8-byte aligned, may be NULL on its own), or both NULL:
 * internal buffers, copied out by agx_decode_quads_fetch, whose `bits` argument then decides about the bits (d_bits must be
 * NULL here).  Frames, quads, counts and point statuses stay in place until the fetch has returned.
 * A fourth kind of batch on the handle: one batch is in flight, a later enqueue of any kind replaces it; the other kinds'
 * fetches of it are AGX_ERR_STATE.  Replacing is not waiting and not discarding: an agx_refine_points_enqueue batch whose
 * results go to caller-owned device arrays need not be fetched before those arrays are passed here -- the kernels run in
 * stream order, so the decode reads the finished records and statuses (the refine batch is then no longer fetchable).
 * AGX_ERR_ARG: NULL d_frames or d_quads, quads_per_frame == 0, a bad point stride, exactly one of d_tags / d_status NULL. */
int agx_decode_quads_enqueue(agx_detector *det, const void *d_frames, int n_frames, int width, int height,
                             size_t row_stride_bytes, size_t frame_stride_bytes, int format,
                             const void *d_quads, size_t point_stride_bytes, uint32_t quads_per_frame,
                             const uint32_t *d_counts, const uint32_t *d_point_status,
                             agx_tag *d_tags, uint32_t *d_status, uint64_t *d_bits);
/* Wait for the batch of agx_decode_quads_enqueue (src/detector.rs:448-476).  Internal buffers: out and status, host arrays
 * of n_frames*quads_per_frame entries, receive the slots the batch wrote (slots at or beyond a frame's count stay as they
 * were); bits, the same for bit_code's values, may be NULL.  Caller-owned device buffers: out, status and bits are NULL, the
 * call only waits.  AGX_ERR_STATE: no such batch in flight (another kind, none, or fetched already). */
int agx_decode_quads_fetch(agx_detector *det, agx_tag *out, uint32_t *status, uint64_t *bits);
/* try_decode_quad (src/detector.rs:448-476) of n_quads quads of one image in HOST memory: uploads pixels and quads (a packed
 * [n_quads][8] float array: x, y of the four corners), runs a batch of one and writes out, status and, unless NULL, bits
 * (n_quads entries each, in input order) and *n_decoded, the number of AGX_QUAD_DECODED ones.  n_quads == 0: AGX_OK,
 * *n_decoded = 0. */
int agx_decode_quads(agx_detector *det, const void *pixels, int width, int height, size_t row_stride_bytes, int format,
                     const void *quads, uint32_t n_quads, agx_tag *out, uint32_t *status, uint64_t *bits,
                     uint32_t *n_decoded);
/* The host's try_decode_quad (src/detector.rs:448-476) without a detector handle (no device needed, like agx_detect_tail):
 * family as in agx_detector_create, luma8 the to_luma8 plane in host memory, quads a packed [n_quads][8] float array.
 * Statuses, zero records and bits as the batch call's; bits may be NULL. */
int agx_decode_quads_tail(int family, const uint8_t *luma8, int width, int height, size_t row_stride_bytes,
                          const void *quads, uint32_t n_quads, agx_tag *out, uint32_t *status, uint64_t *bits,
                          uint32_t *n_decoded);

/* ---- the decode in three stages: decode_positions, bit_code, best_tag -------------------------- */

/* The crate's three pub fns that try_decode_quad is built from, each with its own arguments -- decode_positions(img_w, img_h,
 * quad_pts, border_bits, edge_bits, margin) (src/detector.rs:42-72), bit_code(img, decode_pts, valid_brightness_threshold,
 * max_invalid_bit) (src/detector.rs:74-122) and best_tag(bits, thres, tag_family, edge_bits) (src/detector.rs:142-169) -- over
 * device batches: a caller samples a tag on its own grid, sets the brightness rules of its camera, or matches against a code
 * list of its own.  All three follow agx_filter_saddles_enqueue / agx_collect_tags_enqueue: caller-owned device arrays only,
 * stream-ordered on the detector's stream (the caller's after agx_detector_set_stream), they return without waiting, there is
 * nothing to fetch, and they replace the batch in flight without waiting; a refused argument (AGX_ERR_ARG, AGX_ERR_FORMAT)
 * leaves a batch in flight where it is.  Slot = f*quads_per_frame + q; d_counts as in agx_decode_quads_enqueue (a count above
 * quads_per_frame means quads_per_frame; slots at or beyond a frame's count are neither read nor written).  Statuses are the
 * AGX_QUAD_* values.  Chained at (the family's border_bits / edge_bits, 0.5, 10, 3, the family's Hamming distance, its code list)
 * with no sync in between -- each d_status passed on as the next d_status_in -- they leave what agx_decode_quads_enqueue leaves,
 * byte for byte (tags, statuses, bits), and with it the input of agx_collect_tags_enqueue.  One exception, outside any image:
 * corners beyond 1e37 can overflow a sample to NaN, which try_decode_quad's `as u32` reads as pixel 0 and agx_bit_code_enqueue
 * calls AGX_QUAD_OUTSIDE.
 *
 * decode_positions (src/detector.rs:42-72).  d_quads / point_stride_bytes / n_frames / quads_per_frame / d_counts /
 * d_point_status exactly as agx_decode_quads_enqueue reads them (stride 8 or 20; a quad with a corner whose word is non-zero is
 * AGX_QUAD_SKIPPED).  img_w, img_h: the image size the corners are tested against; no pixel is read.  d_status[slot]:
 * AGX_QUAD_DECODED (Some), AGX_QUAD_OUTSIDE (None: a corner that is not finite, decided first; or :50-56, a rounded corner >=
 * img_w / img_h under the saturating `as u32`, where a finite negative corner is inside) or AGX_QUAD_SKIPPED.  d_points
 * [slots][edge_bits*edge_bits][2] floats: the samples of an AGX_QUAD_DECODED slot in the reference's order, x outer and y inner
 * (:60-70); any other slot writes no point.  The arithmetic is the project's tag_affine -- the least-squares map over the
 * axis-aligned source square in closed form, binary64, rounded once to binary32 -- and h0*x + h1*y + h2*1.0f left to right in
 * binary32: the points are those the fused decode samples at, and within 1e-3 px of any other correctly rounded solve.
 * AGX_ERR_ARG: a NULL or misaligned (4 bytes) array other than d_counts / d_point_status, n_frames <= 0, quads_per_frame == 0,
 * a bad point stride, 2^29 slots or more, edge_bits outside 1 .. 8 (the bits fit a u64), border_bits outside 0 .. 16, a
 * margin that is not finite, or a degenerate source square: (float)side_bits - 1 + margin == -margin as floats. */
int agx_decode_positions_enqueue(agx_detector *det, const void *d_quads, size_t point_stride_bytes, int n_frames,
                                 uint32_t quads_per_frame, const uint32_t *d_counts, const uint32_t *d_point_status,
                                 uint32_t img_w, uint32_t img_h, int border_bits, int edge_bits, float margin,
                                 float *d_points, uint32_t *d_status);
/* decode_positions (src/detector.rs:42-72) in HOST memory, without a detector handle (no device needed, like
 * agx_decode_quads_tail, whose first stage this is -- the same code): quads a packed [n_quads][8] float array, points
 * [n_quads][edge_bits*edge_bits][2], status [n_quads].  Statuses, untouched points and AGX_ERR_ARG as the batch call's. */
int agx_decode_positions_tail(const void *quads, uint32_t n_quads, uint32_t img_w, uint32_t img_h, int border_bits,
                              int edge_bits, float margin, float *points, uint32_t *status);

/* The sampling model of decode_positions, opened.  src/detector.rs:58 maps the tag's cell grid into the image with tag_affine
 * (src/image_util.rs:39-70), a least-squares affine fit through the four corners of what is a projective image of a square;
 * the crate's other pub fn, tag_homography (src/image_util.rs:5-37), is the projective map through the same corners, which
 * samples every cell centre of a tag seen at close range on a wide lens where the affine fit leaves its cell. */
enum { AGX_TAG_MAP_AFFINE = 0,       /* src/image_util.rs:39-70 tag_affine: what decode_positions calls (src/detector.rs:58) */
       AGX_TAG_MAP_HOMOGRAPHY = 1 }; /* src/image_util.rs:5-37 tag_homography */
/* decode_positions (src/detector.rs:42-72) with the map of src/detector.rs:58 chosen by `model`; every other argument is
 * agx_decode_positions_enqueue's.  AGX_TAG_MAP_AFFINE: that call, and its bytes.  AGX_TAG_MAP_HOMOGRAPHY: the map is
 * tag_homography (src/image_util.rs:5-37) of the same source square (-m,-m), (-m,S), (S,S), (S,-m) -- the reference's 8 x 9
 * system has a one-dimensional null space for four points, so its SVD's last vector is THE projective map through them up to
 * scale; the project evaluates that map in closed form, binary64 with + - * / only, rounded once to binary32, scaled so that
 * w = h6*c + h7*c + h8 is 1 at the square's centre c.  u, v and w are each h0*x + h1*y + h2*1.0f left to right in binary32 and
 * the point is (u / w, v / w) by correctly rounded binary32 division.  d_status[slot], decided for the whole slot before its
 * first store and in this order: AGX_QUAD_SKIPPED, AGX_QUAD_OUTSIDE (the corners, as in the existing call),
 * AGX_QUAD_DEGENERATE (no map: the closed form's denominator or the centre's w is zero or not finite, or w at one of the four
 * source corners is not > 0 after scaling -- a quad that is not strictly convex, or whose horizon crosses the tag),
 * AGX_QUAD_OUTSIDE (a sample whose w is not > 0 or not finite), else AGX_QUAD_DECODED; only that one writes points.  The status
 * is a non-zero word like the others: agx_bit_code_enqueue and agx_best_tag_enqueue pass it through, agx_collect_tags_enqueue
 * skips it.  AGX_ERR_ARG: the existing call's, and a model that is neither (a batch in flight stays where it is). */
int agx_decode_positions_enqueue_m(agx_detector *det, const void *d_quads, size_t point_stride_bytes, int n_frames,
                                   uint32_t quads_per_frame, const uint32_t *d_counts, const uint32_t *d_point_status,
                                   uint32_t img_w, uint32_t img_h, int border_bits, int edge_bits, float margin,
                                   float *d_points, uint32_t *d_status, int model);
/* agx_decode_positions_tail (src/detector.rs:42-72) with the model: the host form of the call above, the same code. */
int agx_decode_positions_tail_m(const void *quads, uint32_t n_quads, uint32_t img_w, uint32_t img_h, int border_bits,
                                int edge_bits, float margin, float *points, uint32_t *status, int model);
/* tag_affine (src/image_util.rs:39-70) or tag_homography (src/image_util.rs:5-37) of every quad slot, themselves: d_maps
 * [slots][9] floats, a row-major 3 x 3 matrix from the source square of side_bits and margin to the image (affine: tag_affine's
 * two rows, then 0, 0, 1; homography: as above, w = 1 at the square's centre) -- to warp a tag patch, or to sample on a grid of
 * the caller's own in front of agx_bit_code_enqueue.  d_quads / point_stride_bytes / n_frames / quads_per_frame / d_counts /
 * d_point_status as agx_decode_positions_enqueue; side_bits in 1 .. 40 (2*16 + 8); no image size: neither function takes one.
 * d_status[slot]: AGX_QUAD_SKIPPED, AGX_QUAD_OUTSIDE (a corner that is not finite), AGX_QUAD_DEGENERATE (homography only) or
 * AGX_QUAD_DECODED; any other slot than the last writes no map.  Like agx_decode_positions_enqueue in every respect:
 * caller-owned device arrays, stream-ordered, nothing to fetch, replaces the batch in flight without waiting.
 * AGX_ERR_ARG: a NULL or misaligned (4 bytes) array other than d_counts / d_point_status, n_frames <= 0, quads_per_frame == 0,
 * a bad point stride, 2^29 slots or more, side_bits outside 1 .. 40, a margin that is not finite, a degenerate source square,
 * an unknown model. */
int agx_tag_maps_enqueue(agx_detector *det, const void *d_quads, size_t point_stride_bytes, int n_frames,
                         uint32_t quads_per_frame, const uint32_t *d_counts, const uint32_t *d_point_status, int side_bits,
                         float margin, int model, float *d_maps, uint32_t *d_status);
/* The two pub fns (src/image_util.rs:5-37, :39-70) in HOST memory, without a detector handle: quads a packed [n_quads][8]
 * float array, maps [n_quads][9], status [n_quads].  Statuses, untouched maps and AGX_ERR_ARG as the batch call's. */
int agx_tag_maps_tail(const void *quads, uint32_t n_quads, int side_bits, float margin, int model, float *maps,
                      uint32_t *status);

/* bit_code (src/detector.rs:74-122) of ANY sample points.  d_frames / n_frames / width / height / strides / format as
 * agx_decode_quads_enqueue (AGX_LF32 is AGX_ERR_FORMAT; every format but AGX_L8 goes through the device's to_luma8 plane).
 * d_points [slots][points_per_slot][2] floats, points_per_slot in 1 .. 64 (agx_decode_positions_enqueue's d_points with
 * edge_bits*edge_bits, or a caller's own grid).  d_status_in: NULL, or one word per slot, and it may be d_status itself: a slot
 * whose word is non-zero reads no pixel, gets bits 0, and its word is passed through to d_status.  valid_brightness_threshold in
 * 0 .. 255 (a u8 in the crate), max_invalid_bit any uint32.  d_status[slot], decided in the reference's order: AGX_QUAD_OUTSIDE
 * (:84-93, a sample that rounds outside the image; and, as for a quad's corners, a sample coordinate that is not finite,
 * decided before any read), AGX_QUAD_LOW_CONTRAST (:97-99, max - min < 50), AGX_QUAD_AMBIGUOUS (:117-118, more than
 * max_invalid_bit samples within valid_brightness_threshold of the mid brightness), else AGX_QUAD_DECODED.  d_bits[slot]
 * (8-byte aligned): the first point is the most significant of the points_per_slot bits; 0 unless AGX_QUAD_DECODED.
 * AGX_ERR_ARG: a NULL or misaligned array other than d_counts / d_status_in, quads_per_frame == 0, points_per_slot or the
 * threshold out of range, 2^29 slots or more, and what agx_decode_quads_enqueue refuses of the frames. */
int agx_bit_code_enqueue(agx_detector *det, const void *d_frames, int n_frames, int width, int height,
                         size_t row_stride_bytes, size_t frame_stride_bytes, int format,
                         const float *d_points, uint32_t points_per_slot, uint32_t quads_per_frame,
                         const uint32_t *d_counts, const uint32_t *d_status_in, int valid_brightness_threshold,
                         uint32_t max_invalid_bit, uint64_t *d_bits, uint32_t *d_status);
/* bit_code (src/detector.rs:74-122) of n_slots point lists on ONE u8 plane in HOST memory (tight or padded rows), without a
 * detector handle: agx_decode_quads_tail's second stage, the same code.  Statuses, zero bits and status_in as the batch call's. */
int agx_bit_code_tail(const uint8_t *luma8, int width, int height, size_t row_stride_bytes, const float *points,
                      uint32_t points_per_slot, uint32_t n_slots, const uint32_t *status_in,
                      int valid_brightness_threshold, uint32_t max_invalid_bit, uint64_t *bits, uint32_t *status);
/* best_tag (src/detector.rs:142-169) against ANY code list.  d_bits [n_slots] (8-byte aligned); d_status_in as in
 * agx_bit_code_enqueue (NULL, or pass-through of non-zero words; may be d_status).  d_counts: NULL (then quads_per_frame is not
 * read), or per-frame counts with n_slots a multiple of quads_per_frame, as above.  thres in 0 .. 255 (a u8 in the crate): a
 * rotation matches at a distance BELOW it, so 0 matches nothing.  d_codes: a device list of n_codes in 1 .. 65535 64-bit codes,
 * or NULL with n_codes == 0: the handle's family list.  edge_bits in 1 .. 8.  The reference's result bit for bit: per rotation,
 * in rotation order, the FIRST code with the smallest distance; rotation 0 counts all 64 bits of the XOR while rotate_bits
 * (:124-140) keeps only the low edge_bits^2 bits, so bits above them matter at rotation 0 only.  d_ids, d_rotations
 * [n_slots]: the code's index and the rotation, 0 unless AGX_QUAD_DECODED; d_status: AGX_QUAD_DECODED or AGX_QUAD_NO_MATCH
 * (:160-168).  d_quads + point_stride_bytes (agx_decode_positions_enqueue's input) and d_tags, given together or not at all:
 * d_tags[slot] = {id, the corners after rotate_left(rotation); reverse()} (src/detector.rs:448-476, :467-470), exactly
 * agx_decode_quads_enqueue's record, all zero unless AGX_QUAD_DECODED.
 * AGX_ERR_ARG: a NULL or misaligned d_bits, d_ids, d_rotations or d_status, n_slots == 0 or 2^31 and more, thres, n_codes or
 * edge_bits out of range, d_codes and n_codes that do not go together, d_counts with a quads_per_frame that does not divide
 * n_slots, exactly one of d_quads / d_tags, a bad point stride. */
int agx_best_tag_enqueue(agx_detector *det, const uint64_t *d_bits, uint32_t n_slots, uint32_t quads_per_frame,
                         const uint32_t *d_counts, const uint32_t *d_status_in, int thres, const uint64_t *d_codes,
                         uint32_t n_codes, int edge_bits, const void *d_quads, size_t point_stride_bytes,
                         uint32_t *d_ids, uint32_t *d_rotations, uint32_t *d_status, agx_tag *d_tags);
/* best_tag (src/detector.rs:142-169) in HOST memory, without a detector handle: agx_decode_quads_tail's third stage, the same
 * code.  codes / n_codes as d_codes / n_codes, with `family` (as in agx_detector_create; else not read) naming the list where
 * codes is NULL; quads a packed [n_slots][8] float array, given together with tags or not at all.  Everything else as the batch
 * call's; AGX_ERR_FAMILY. */
int agx_best_tag_tail(const uint64_t *bits, uint32_t n_slots, const uint32_t *status_in, int thres, int family,
                      const uint64_t *codes, uint32_t n_codes, int edge_bits, const void *quads, uint32_t *ids,
                      uint32_t *rotations, uint32_t *status, agx_tag *tags);

/* ---- board search in caller-given saddle lists ------------------------------------------- */

/* try_find_best_board(refined: &[Saddle]) -> Option<Vec<[usize; 4]>> -- src/detector.rs:588-639, a pub fn of the crate: which
 * saddles of ANY list (last frame's corners after agx_refine_points_enqueue, another detector's, the device lists of
 * agx_saddles_batch_enqueue_to) form the quads of a board, without running the saddle chain on pixels.  Between
 * agx_refine_points_enqueue and agx_decode_quads_enqueue it completes detect's stages on the device, in stream order; each is
 * usable alone.  A frame's answer is a count, one of these statuses and its quads: four saddle numbers each, quads in
 * all_tag_indexes' order (cells in insertion order), within a quad the order init_quads gives (:577-581). */
enum { AGX_BOARD_FOUND = 0,    /* src/detector.rs:588-639 returned Some: n_quads quads */
       AGX_BOARD_NONE = 1,     /* None: an empty list (:589-591), or no board scored above 0 */
       AGX_BOARD_CAPACITY = 2, /* more quads than the caller's rows hold: the true count and no row; nothing is truncated */
       AGX_BOARD_INPUT = 3,    /* a listed saddle whose x, y or theta is not finite (the reference panics on such coordinates,
                                  :594; a non-finite theta is refused as well), or a frame-table entry with an overflow bit.
                                  Decided before any search */
       AGX_BOARD_PENDING = 4 };/* device arrays only, between enqueue and fetch: the kernel handed the frame back to the host
                                  form (src/detector.rs:588-639 on the host); final after agx_find_boards_fetch */

/* try_find_best_board (src/detector.rs:588-639) once per frame over saddle lists in DEVICE memory, stream-ordered on the
 * detector's stream (the caller's after agx_detector_set_stream); returns without waiting.  No pixels are read.
 * d_saddles is a run of saddle SLOTS: slot s holds the floats x, y, k, theta, phi at d_saddles + s*saddle_stride_bytes (a
 * multiple of 4, at least 20; 20 = agx_saddle records: agx_refine_points_enqueue's d_out and agx_saddles_batch_enqueue_to's
 * d_saddles as they stand).  k and phi are never read.
 *   d_counts       frame f owns the slots [f*saddles_per_frame, + min(d_counts[f], saddles_per_frame)); NULL: saddles_per_frame;
 *   d_frame_table  instead (at most one of the two): the agx_frame_result entries of agx_saddles_batch_enqueue_to: frame f owns
 *                  `count` slots from `offset` (saddles_per_frame does not bound them).  A frame whose status carries an overflow
 *                  bit (AGX_FRAME_CANDIDATE_ / _CLUSTER_ / _SADDLE_OVERFLOW) is AGX_BOARD_INPUT and nothing of it is read;
 *   d_point_status NULL, or one word per slot (indexed like the slots): only slots whose word is AGX_POINT_REFINED (0) enter
 *                  the list, in slot order -- agx_refine_points_enqueue's d_out / d_status are read in place, and a caller
 *                  removes the saddles of decoded quads between rounds of max_num_of_boards by marking their words non-zero:
 *                  agx_collect_tags_enqueue (below) does that on the device, AGX_POINT_USED, behind the round's decode.
 * Results, frame f: d_n_quads[f], d_status[f] (AGX_BOARD_*), d_quads[f][quads_per_frame][4]: uint32 SLOT NUMBERS WITHIN THE
 * FRAME (not positions in the list after d_point_status), and, if d_quad_points is given, [f][quads_per_frame][4][2] floats: the
 * corners' x, y in that order -- with d_n_quads as d_counts a valid d_quads (point stride 8) of agx_decode_quads_enqueue.  Only
 * rows below a frame's count are written; more quads than quads_per_frame is AGX_BOARD_CAPACITY with the true count and no row.
 * A listed saddle whose x, y or theta is not finite makes the frame AGX_BOARD_INPUT; an empty list is AGX_BOARD_NONE; both
 * before any search.  d_quads, d_n_quads and d_status are caller-owned device memory (4-byte aligned) or all NULL: internal
 * buffers, copied out by agx_find_boards_fetch; d_quad_points is optional on its own.
 * The kernel answers what the device tail of agx_detect_batch_enqueue answers (options "device_tail", "tail_debug_band"): a
 * frame with more than 1024 listed saddles, a coordinate beyond 1e6, a theta outside [-180, 180], lists beyond the kernel's
 * fixed sizes or an angle inside a guard band is AGX_BOARD_PENDING in d_status until agx_find_boards_fetch has run the host
 * form on it -- the same rows either way.  With "device_tail" 0, or where it is refused, that is every frame.
 * A fifth kind of batch on the handle (src/detector.rs:588-639): one batch is in flight, a later enqueue of any kind replaces
 * it without waiting, the other kinds' fetches of it are AGX_ERR_STATE.  A refine batch into caller-owned arrays need not be
 * fetched before those arrays are passed here, and this batch's caller-owned outputs may go straight into
 * agx_decode_quads_enqueue once no frame can be pending (else: after the fetch).
 * AGX_ERR_ARG: NULL d_saddles, a bad stride, saddles_per_frame or quads_per_frame == 0, both d_counts and d_frame_table, a mixed
 * NULL / non-NULL d_quads, d_n_quads, d_status. */
int agx_find_boards_enqueue(agx_detector *det, const void *d_saddles, size_t saddle_stride_bytes, int n_frames,
                            uint32_t saddles_per_frame, const uint32_t *d_counts, const void *d_frame_table,
                            const uint32_t *d_point_status, uint32_t quads_per_frame, uint32_t *d_quads,
                            float *d_quad_points, uint32_t *d_n_quads, uint32_t *d_status);
/* Wait for the batch of agx_find_boards_enqueue (src/detector.rs:588-639) and resolve every AGX_BOARD_PENDING frame: its listed
 * slots are copied down, the host form runs on the detector's pool (n_threads host threads; 0: agx_host_parallelism()), and the
 * frame's rows, count and status are written to the device arrays on the detector's stream before the call returns.  Internal
 * buffers: quads [n_frames][quads_per_frame][4], n_quads and status [n_frames] are host arrays (required); quad_points
 * [n_frames][quads_per_frame][4][2] may be NULL; rows at or beyond a frame's count stay as they were.  Caller-owned device
 * arrays: all four may be NULL (given ones are filled the same way).  AGX_ERR_STATE: no such batch in flight. */
int agx_find_boards_fetch(agx_detector *det, uint32_t *quads, float *quad_points, uint32_t *n_quads, uint32_t *status,
                          int n_threads);
/* try_find_best_board (src/detector.rs:588-639) of one list in HOST memory: uploads it, runs a batch of one and fetches it.
 * quads [cap][4]: saddle indices into `saddles`; *n_quads the count, *status an AGX_BOARD_* value (never PENDING).
 * n_saddles == 0: AGX_OK, AGX_BOARD_NONE. */
int agx_find_board(agx_detector *det, const agx_saddle *saddles, uint32_t n_saddles, uint32_t *quads, uint32_t cap,
                   uint32_t *n_quads, uint32_t *status);
/* The host form of try_find_best_board (src/detector.rs:588-639) without a detector handle (no device needed, like
 * agx_detect_tail): what agx_find_boards_fetch runs on a handed-back frame.  Statuses, counts and rows as the batch call's. */
int agx_find_board_tail(const agx_saddle *saddles, uint32_t n_saddles, uint32_t *quads, uint32_t cap, uint32_t *n_quads,
                        uint32_t *status);

/* ---- candidate quads of caller-given seed saddles ---------------------------------------- */

/* init_quads(refined, s0_idx, tree) -- src/detector.rs:543-586, with is_valid_quad (src/saddle.rs:17-67) -- the `pub fn` between
 * a refined saddle list and the seed quads of a board: for a caller who knows one CORNER of the board (a tracked saddle, a
 * predicted point snapped to the nearest saddle) rather than one quad.  Its rows are agx_grow_boards_enqueue's seeds as they
 * stand, so saddles -> init_quads -> grow boards (at any spacing ratio) -> decode -> collect runs without a host step.
 * Per frame over saddle lists in DEVICE memory, stream-ordered on the detector's stream; returns without waiting.  d_saddles,
 * saddle_stride_bytes, n_frames, saddles_per_frame, d_counts, d_frame_table and d_point_status are read exactly as
 * agx_find_boards_enqueue reads them (an overflow bit or a listed saddle with a non-finite x, y or theta: AGX_BOARD_INPUT).
 *   d_seed_saddles [n_frames][seeds_per_frame] uint32: slot numbers within the frame.  Frame f has min(d_seed_counts[f],
 *                  seeds_per_frame) seeds, seeds_per_frame with d_seed_counts NULL.  Every seed of the frame is looked at
 *                  before anything is written: one that names a slot at or beyond the frame's count, or a slot that is not
 *                  listed, makes the frame AGX_BOARD_INPUT.  The same saddle twice yields its quads twice.
 *                  NULL: try_find_best_board's own seeds (:601-616) -- the saddles of the fullest round(theta) bin (of equally
 *                  full bins the one with the smallest angle), taken from the back of the list -- the first seeds_per_frame of
 *                  them; 30 is the reference's loop bound (:613).
 *   n_nearest      2 .. 64: the 50 of :550, the neighbours (the seed itself among them) a seed's quads are made of.  A seed
 *                  among fewer listed saddles uses all of them; saddles at exactly the same binary32 squared distance are taken
 *                  in list order.
 * Results, frame f: d_quads [f][quads_per_frame][4]: slot numbers within the frame, seed i's quads behind seed i - 1's, each
 * seed's in init_quads' loop order and every row in its corner order (:577-581), so column 0 is the row's seed; d_n_quads[f]
 * their number -- d_quads with d_n_quads are d_seed_quads with d_seed_counts of agx_grow_boards_enqueue (seeds_per_frame =
 * quads_per_frame) --; d_quad_points (optional) as agx_find_boards_enqueue's; d_status[f]:
 *   AGX_BOARD_FOUND     at least one quad;
 *   AGX_BOARD_NONE      an empty list, no seed, or no valid quad;
 *   AGX_BOARD_CAPACITY  more quads than quads_per_frame: the true count and no row;
 *   AGX_BOARD_INPUT     as above; only d_n_quads (0), d_status and d_n_seeds_out (0) are written;
 *   AGX_BOARD_PENDING   handed back, until agx_init_quads_fetch has run the host form.
 * d_seed_quad_counts [n_frames][seeds_per_frame] (optional): the quads of each seed, 0 behind the frame's seeds -- what maps
 * agx_grow_boards_enqueue's d_best_seed back to a saddle, and what the reference's per-saddle `>= 36` rule (:626) is applied
 * with.  d_seeds_out [n_frames][seeds_per_frame], d_n_seeds_out [n_frames] (optional): the seeds taken, rows below the count.
 * These three are written for frames that end FOUND, NONE or CAPACITY.  All arrays are caller-owned device memory, 4-byte
 * aligned; d_quads, d_n_quads and d_status are required.
 * The kernel hands a frame back as AGX_BOARD_PENDING where agx_find_boards_enqueue's does: more than 1024 listed saddles, a
 * coordinate beyond 1e6, a theta outside [-180, 180], a seed with more than 256 candidate quads, a quad that hangs on a
 * white-block angle inside the guard band, option "tail_debug_band"; every frame with "device_tail" 0 or refused.
 * A further kind of batch on the handle: it replaces whatever is in flight without waiting, the other kinds' fetches of it are
 * AGX_ERR_STATE, and a refused argument leaves the batch in flight where it is.
 * AGX_ERR_ARG: agx_find_boards_enqueue's, NULL d_quads, d_n_quads or d_status, seeds_per_frame == 0, d_seed_counts without
 * d_seed_saddles, n_nearest outside 2 .. 64, 2^27 or more seed rows in the batch. */
int agx_init_quads_enqueue(agx_detector *det, const void *d_saddles, size_t saddle_stride_bytes, int n_frames,
                           uint32_t saddles_per_frame, const uint32_t *d_counts, const void *d_frame_table,
                           const uint32_t *d_point_status,
                           const uint32_t *d_seed_saddles, uint32_t seeds_per_frame, const uint32_t *d_seed_counts,
                           uint32_t n_nearest,
                           uint32_t quads_per_frame, uint32_t *d_quads, float *d_quad_points, uint32_t *d_n_quads,
                           uint32_t *d_status, uint32_t *d_seed_quad_counts, uint32_t *d_seeds_out, uint32_t *d_n_seeds_out);
/* Wait for the batch of agx_init_quads_enqueue and resolve every AGX_BOARD_PENDING frame: the host form (agx_init_quads_tail's
 * code) runs on the detector's pool (n_threads host threads; 0: agx_host_parallelism()), and the frame's rows, count, status,
 * per-seed counts and seeds are written to the device arrays on the detector's stream before the call returns.
 * AGX_ERR_STATE: no such batch in flight. */
int agx_init_quads_fetch(agx_detector *det, int n_threads);
/* The host form without a detector handle (no device needed, like agx_find_board_tail): one list, the same semantics.
 * seed_saddles [n_seeds] and quads [cap][4] are indices into `saddles`; point_status NULL or a word per saddle (0 = listed).
 * The first min(n_seeds, max_seeds) seeds are taken; seed_saddles NULL (with n_seeds 0): the reference's own seeds, at most
 * max_seeds of them.  seed_quad_counts [max_seeds], seeds_out [max_seeds] and n_seeds_out may be NULL; the first two are left as
 * they are for AGX_BOARD_INPUT.  AGX_ERR_ARG: a NULL n_quads or status, seeds without seed_saddles, max_seeds == 0, n_nearest
 * outside 2 .. 64. */
int agx_init_quads_tail(const agx_saddle *saddles, uint32_t n_saddles, const uint32_t *point_status,
                        const uint32_t *seed_saddles, uint32_t n_seeds, uint32_t max_seeds, uint32_t n_nearest,
                        uint32_t *quads, uint32_t cap, uint32_t *n_quads, uint32_t *status,
                        uint32_t *seed_quad_counts, uint32_t *seeds_out, uint32_t *n_seeds_out);

/* ---- boards from the caller's seed quads ------------------------------------------------- */

/* Board::new(refined, active_idxs, quad_idxs, spacing_ratio, tree) -- src/board.rs:26-48 -- with try_fix_missing (:52-112),
 * all_tag_indexes and score: the `pub` items try_find_best_board itself is made of, for a caller who already knows one quad of
 * the board (a row of an earlier frame's d_quads after agx_refine_points_enqueue, a quad predicted from a pose) and so needs
 * neither init_quads' 50-NN nor a board per candidate quad -- and with the crate's spacing_ratio as an argument: detect's own
 * search passes the literal 0.3 (:621; agx_params.tag_spacing_ratio is never read, as in the reference), which loses a board
 * whose tags lie more than about one tag side apart.  The neighbour's corner is looked for at a + (b - a)*(1 + spacing_ratio),
 * within sqrt(0.5)*|b - a| (:186-213). */
enum { AGX_GROW_FIX_MISSING = 1 };  /* flags: run try_fix_missing (board.rs:52-112) on the chosen board, as try_find_best_board does (:633) */

/* Per frame over saddle lists in DEVICE memory, stream-ordered on the detector's stream; returns without waiting.  d_saddles,
 * saddle_stride_bytes, n_frames, saddles_per_frame, d_counts, d_frame_table and d_point_status are read exactly as
 * agx_find_boards_enqueue reads them (at most one of d_counts and d_frame_table; an overflow bit or a listed saddle with a
 * non-finite x, y or theta: AGX_BOARD_INPUT).
 *   d_seed_quads   [n_frames][seeds_per_frame][4] uint32: slot numbers within the frame in init_quads' corner order (:577-581) --
 *                  a row of agx_find_boards_enqueue's d_quads is one as it stands.  Frame f has min(d_seed_counts[f],
 *                  seeds_per_frame) seeds, seeds_per_frame with d_seed_counts NULL.  A seed is NOT tested with is_valid_quad
 *                  (Board::new does not either: its score is at least 1).  Every seed of the frame is looked at before any
 *                  board is grown: one that names a slot at or beyond the frame's count, or a slot that is not listed, makes the
 *                  frame AGX_BOARD_INPUT; no seed at all is AGX_BOARD_NONE.
 *   spacing_ratio  finite with 1.0f + spacing_ratio > 0; at 0.3f the arithmetic is agx_find_boards_enqueue's bit for bit
 *                  (1.0f + 0.3f in binary32).
 *   stop_score     0: every seed is grown.  Else the seeds are taken in order until the best score so far is >= stop_score:
 *                  the seeds behind that one read score 0 and are never chosen.  This is the CALLER'S rule per seed quad; the
 *                  reference's own `>= 36` (:626) stops per seed SADDLE, after all of its candidate quads, and is not this.
 *   flags          AGX_GROW_FIX_MISSING or 0.
 * The board of seed i is Board::new(listed saddles, all-true mask, seed i, spacing_ratio, tree); d_seed_scores[f][i] (optional)
 * is its score.  The chosen board is the first seed whose score is strictly above every earlier one (:622's `>`): d_best_seed[f]
 * (optional).  Its quads -- after try_fix_missing under AGX_GROW_FIX_MISSING -- go out exactly as agx_find_boards_enqueue's:
 * d_quads [n_frames][quads_per_frame][4] slot numbers within the frame, cells in insertion order, d_quad_points (optional),
 * d_n_quads, d_status (AGX_BOARD_*; AGX_BOARD_CAPACITY: the true count and no row), so agx_decode_quads_enqueue and
 * agx_collect_tags_enqueue follow unchanged.  d_seed_scores and d_best_seed are written for frames that end AGX_BOARD_FOUND or
 * AGX_BOARD_CAPACITY only.  All arrays are caller-owned device memory, 4-byte aligned; d_quads, d_n_quads and d_status are
 * required.
 * The kernel hands a frame back as AGX_BOARD_PENDING where agx_find_boards_enqueue's does (more than 1024 listed saddles, a
 * coordinate beyond 1e6, a theta outside [-180, 180], a board beyond the kernel's fixed sizes, an angle inside a guard band,
 * option "tail_debug_band"; every frame with "device_tail" 0 or refused) until agx_grow_boards_fetch has run the host form.
 * A further kind of batch on the handle: it replaces whatever is in flight without waiting, the other kinds' fetches of it are
 * AGX_ERR_STATE, and a refused argument leaves the batch in flight where it is.
 * AGX_ERR_ARG: agx_find_boards_enqueue's, NULL d_quads, d_n_quads, d_status or d_seed_quads, seeds_per_frame == 0, 2^27 or more
 * seed rows in the batch, a spacing_ratio that is not finite or with 1.0f + spacing_ratio <= 0, an unknown flag. */
int agx_grow_boards_enqueue(agx_detector *det, const void *d_saddles, size_t saddle_stride_bytes, int n_frames,
                            uint32_t saddles_per_frame, const uint32_t *d_counts, const void *d_frame_table,
                            const uint32_t *d_point_status,
                            const uint32_t *d_seed_quads, uint32_t seeds_per_frame, const uint32_t *d_seed_counts,
                            float spacing_ratio, uint32_t stop_score, int flags,
                            uint32_t quads_per_frame, uint32_t *d_quads, float *d_quad_points, uint32_t *d_n_quads,
                            uint32_t *d_status, uint32_t *d_seed_scores, uint32_t *d_best_seed);
/* Wait for the batch of agx_grow_boards_enqueue and resolve every AGX_BOARD_PENDING frame: the host form (agx_grow_board_tail's
 * code) runs on the detector's pool (n_threads host threads; 0: agx_host_parallelism()), and the frame's rows, count, status,
 * seed scores and best seed are written to the device arrays on the detector's stream before the call returns.
 * AGX_ERR_STATE: no such batch in flight. */
int agx_grow_boards_fetch(agx_detector *det, int n_threads);
/* The host form without a detector handle (no device needed, like agx_find_board_tail): one list, the same semantics.
 * seed_quads [n_seeds][4] and quads [cap][4] are indices into `saddles`; point_status NULL or a word per saddle (0 = listed);
 * seed_scores [n_seeds] and best_seed may be NULL.  *n_quads, *status as agx_find_board_tail's; seed_scores and *best_seed are
 * written for AGX_BOARD_FOUND and AGX_BOARD_CAPACITY only.  AGX_ERR_ARG as the batch call's. */
int agx_grow_board_tail(const agx_saddle *saddles, uint32_t n_saddles, const uint32_t *point_status,
                        const uint32_t *seed_quads, uint32_t n_seeds, float spacing_ratio, uint32_t stop_score, int flags,
                        uint32_t *quads, uint32_t cap, uint32_t *n_quads, uint32_t *status,
                        uint32_t *seed_scores, uint32_t *best_seed);

/* ---- caller points snapped to the nearest listed saddle ------------------------------------ */

/* The link from an earlier frame's corners -- a tag table, a quad predicted from a pose, one tracked corner -- to THIS frame's
 * slot numbers: every caller point is mapped to the nearest listed saddle of its frame's list, and the rows whose points all
 * snapped are compacted into the seeds agx_grow_boards_enqueue (4 points per row: d_seed_quads / d_seed_counts) and
 * agx_init_quads_enqueue (1: d_seed_saddles / d_seed_counts) take as they stand.  The reference has no such function; the
 * distance is kdtree::distance::squared_euclidean, the fold over the two axes that init_quads' tree is asked with
 * (src/detector.rs:15, :550).  A corner may have
 * moved by any distance up to sqrt(max_dist_sq): agx_refine_points_enqueue, the other way from old corners to new records,
 * rejects a point that moved more than 1 px.
 * Per frame over saddle lists in DEVICE memory, stream-ordered on the detector's stream (the caller's after
 * agx_detector_set_stream); returns without waiting.  d_saddles, saddle_stride_bytes, n_frames, saddles_per_frame, d_counts,
 * d_frame_table and d_point_status are read exactly as agx_find_boards_enqueue reads them: only slots whose status word is 0 are
 * candidates; an overflow bit in a table entry, or a listed saddle with a non-finite x or y, makes the frame AGX_SNAP_INPUT,
 * decided before the frame's first store.  k, theta and phi are never read.  Lists of any length are answered on the device:
 * nothing is handed back, no frame is ever pending and there is nothing to fetch.
 *   d_points        row r of frame f starts at d_points + (f*rows_per_frame + r)*row_stride_bytes, its point j is two floats
 *                   (x, y) at + j*point_stride_bytes; points_per_row is 1 .. 4.  Both strides are multiples of 4, the point
 *                   stride at least 8, and the row stride covers (points_per_row - 1)*point_stride_bytes + 8.  With
 *                   &d_tags[0].xy, row stride sizeof(agx_tag) and point stride 8 a tag table of agx_collect_tags_enqueue or
 *                   agx_detect_batch_enqueue_to is read in place (rows_per_frame = its rows per frame, d_row_counts = its counts).
 *   d_row_counts    NULL, or [n_frames]: frame f has min(d_row_counts[f], rows_per_frame) rows.
 *   max_dist_sq     the SQUARED distance itself, >= 0, +inf allowed: nothing is squared on either side.
 *   flags           AGX_SNAP_REVERSE reads a row's points back to front.  A tag's xy is rotate_left(rotation); reverse() of its
 *                   quad (src/detector.rs:467-470): read backwards it is a cyclic rotation of that quad in init_quads' winding
 *                   (:577-581), which Board::new grows in all four directions alike.
 * Arithmetic, all binary32 with no contraction: dx = sx - px, dy = sy - py, d2 = dx*dx + dy*dy.  The nearest is the candidate
 * with the smallest d2 below +inf; at equal d2 the lowest slot number wins.  The point snaps if d2 <= max_dist_sq.  A point with
 * a non-finite coordinate has no d2 below +inf and never snaps.
 * Results, frame f, all caller-owned device memory, 4-byte aligned:
 *   d_slots   [n_frames][rows_per_frame][points_per_row]: the slot within the frame, or AGX_SNAP_NONE, in the order the row was
 *             read (under AGX_SNAP_REVERSE the reversed order);
 *   d_dist_sq the same shape, optional: d2 to the nearest candidate, whether it snapped or not; +inf where there is none;
 *   d_rows    [n_frames][rows_per_frame][points_per_row] with d_n_rows[f]: the rows whose points ALL snapped, to pairwise distinct
 *             slots, compacted in row order.  Two rows that snap to the same slots are both kept;
 *   d_row_index [n_frames][rows_per_frame], optional: the row each compacted row came from;
 *   d_status[f]: AGX_SNAP_OK, or AGX_SNAP_INPUT: d_n_rows[f] = 0, and nothing else of the frame is written.
 * Only entries below a frame's row count (d_slots, d_dist_sq) and below d_n_rows[f] (d_rows, d_row_index) are ever written.
 * Like agx_filter_saddles_enqueue the call replaces the batch in flight without waiting; every kind's fetch is AGX_ERR_STATE then.
 * AGX_ERR_ARG (a batch in flight stays where it is): the list-argument errors of agx_find_boards_enqueue; NULL d_points, d_slots,
 * d_rows, d_n_rows or d_status; points_per_row outside 1 .. 4; rows_per_frame == 0; a stride that is not a multiple of 4, a
 * point stride below 8 or a row stride that does not cover the row; a negative or NaN max_dist_sq; an unknown flag; a pointer
 * that is not 4-byte aligned; 2^27 or more rows in the batch. */
enum { AGX_SNAP_REVERSE = 1 };                /* flags */
enum { AGX_SNAP_OK = 0, AGX_SNAP_INPUT = 1 }; /* per frame */
#define AGX_SNAP_NONE 0xFFFFFFFFu             /* d_slots: the point did not snap */
int agx_snap_points_enqueue(agx_detector *det, const void *d_saddles, size_t saddle_stride_bytes, int n_frames,
                            uint32_t saddles_per_frame, const uint32_t *d_counts, const void *d_frame_table,
                            const uint32_t *d_point_status,
                            const void *d_points, size_t row_stride_bytes, size_t point_stride_bytes, uint32_t rows_per_frame,
                            uint32_t points_per_row, const uint32_t *d_row_counts, float max_dist_sq, int flags,
                            uint32_t *d_slots, float *d_dist_sq, uint32_t *d_rows, uint32_t *d_n_rows, uint32_t *d_row_index,
                            uint32_t *d_status);
/* The host form without a detector handle (no device needed, like agx_find_board_tail): one list and its n_rows rows, the same
 * arithmetic and semantics.  point_status NULL or a word per saddle (0 = listed); slots / dist_sq (may be NULL) [n_rows]
 * [points_per_row]; rows [n_rows][points_per_row], row_index (may be NULL) [n_rows]; *n_rows_out the compacted count, *status
 * AGX_SNAP_OK or AGX_SNAP_INPUT (then *n_rows_out = 0 and nothing else is written).  AGX_ERR_ARG as the batch call's; n_rows
 * may be 0. */
int agx_snap_points_tail(const agx_saddle *saddles, uint32_t n_saddles, const uint32_t *point_status,
                         const void *points, size_t row_stride_bytes, size_t point_stride_bytes, uint32_t n_rows,
                         uint32_t points_per_row, float max_dist_sq, int flags,
                         uint32_t *slots, float *dist_sq, uint32_t *rows, uint32_t *n_rows_out, uint32_t *row_index,
                         uint32_t *status);

/* ---- blur and Hessian-response planes at any sigma ---------------------------------------- */

/* image_util::gaussian_blur_f32(img, sigma) -- src/image_util.rs:110-206 -- and image_util::hessian_response(img) --
 * src/image_util.rs:72-109 --, two `pub fn`s of the crate, over a batch in DEVICE memory: stream-ordered on the detector's stream
 * (the caller's after agx_detector_set_stream), returns without waiting.  d_frames / n_frames / width / height / strides / format
 * as agx_saddles_batch_enqueue (every agx_format, AGX_LF32 included -- its row stride a multiple of 4 bytes; width, height >= 1).
 * sigma > 0: d_blur, if given, receives gaussian_blur_f32(to_luma32f(frame), sigma) and d_response, if given,
 * hessian_response of that blur -- what refined_saddle_points computes at src/detector.rs:410-411 for sigma 1.5; with d_response
 * alone the blur goes to a workspace plane.  The radius ceilf(2 sigma) may be 1 .. 16 (sigma up to 8.0).  sigma == 0.0f: no blur
 * (the reference's weights are NaN there) -- d_blur must be NULL and d_response receives hessian_response(to_luma32f(frame)).
 * d_blur, d_response: caller-owned device memory, 4-byte aligned, with the same strides: frame f, row y starts at
 * f*out_frame_stride_bytes + y*out_row_stride_bytes; only the width floats of a row are written, padding is never touched.  The
 * outputs must not overlap the frames or each other.  Every value is the reference's, bit for bit; the border ring of a response
 * plane -- all of it where width < 3 or height < 3 -- is +0.0.
 * AGX_ERR_ARG: NULL d_frames, both outputs NULL, sigma negative, NaN, infinite or with ceilf(2 sigma) > 16, sigma == 0 with d_blur,
 * out_row_stride_bytes below 4*width, above 0x7fffffff or not a multiple of 4, out_frame_stride_bytes below height*out_row_stride_bytes or not a
 * multiple of 4, an AGX_LF32 row stride that is not a multiple of 4.
 * A sixth kind of batch on the handle: it replaces whatever is in flight and has no fetch of its own -- the planes are complete in
 * stream order (or after agx_detector_sync), and every other kind's fetch is AGX_ERR_STATE then.  Replacing is neither waiting nor
 * discarding: a plane written here may go straight into agx_refine_points_enqueue(.., AGX_LF32, AGX_REFINE_PLANE, ..) with no
 * sync in between. */
int agx_planes_enqueue(agx_detector *det, const void *d_frames, int n_frames, int width, int height,
                       size_t row_stride_bytes, size_t frame_stride_bytes, int format, float sigma,
                       float *d_blur, float *d_response, size_t out_row_stride_bytes, size_t out_frame_stride_bytes);
/* gaussian_blur_f32(to_luma32f(image), sigma) (src/image_util.rs:110-206) of one image in HOST memory: uploads it, runs a batch
 * of one, writes the width*height floats of the plane, tightly packed, to out.  sigma as above, but not 0. */
int agx_gaussian_blur_f32(agx_detector *det, const void *pixels, int width, int height, size_t row_stride_bytes,
                          int format, float sigma, float *out);
/* hessian_response(to_luma32f(image)) (src/image_util.rs:72-109) of one image in HOST memory, no blur; out as above. */
int agx_hessian_response(agx_detector *det, const void *pixels, int width, int height, size_t row_stride_bytes,
                         int format, float *out);

/* ---- cluster centres of caller-given response planes, and the k / phi filter ----------------- */

typedef struct agx_cluster_info {
    uint32_t first_index, size;
    float cx, cy;
} agx_cluster_info;

/* src/detector.rs:414-429 on ANY response plane -- agx_planes_enqueue's d_response, or a caller's own (another derivative, a
 * masked plane, one combined from several exposures or pyramid levels) -- over a batch in DEVICE memory, stream-ordered on the
 * detector's stream (the caller's after agx_detector_set_stream); returns without waiting.  Per frame: min = the fold
 * `e < acc ? e : acc` from f32::MAX over all width*height values (:414-417; a NaN never wins), thr = min * 0.05f (:418), the
 * 4-connected components of v < thr (init_saddle_clusters / pixel_bfs, :171-187, src/image_util.rs:208-236), one cluster per
 * component in the order of its first pixel in the raster scan, and the centroid map (:421-429): agx_cluster_info =
 * {first_index = y*width + x of that pixel, size, cx, cy}.  cx, cy are the reference's bit for bit while the coordinate sums
 * stay below 2^24; beyond that they are the quotients of the exact integer sums -- f32(sum) / f32(size), the sums held in
 * 64 bits: one component of a masked plane passes 2^32 -- and AGX_CLUSTERS_INEXACT is set (as AGX_FRAME_CENTROID_INEXACT).
 * The outermost ring: the reference scans seeds in the interior only but lets a flood run into the ring where a ring pixel is
 * below thr; a component's first scanned pixel is then not its smallest pixel.  That is not emulated: a frame with any ring
 * pixel below thr is refused -- AGX_CLUSTERS_BORDER, count 0, no row -- and the other frames of the batch are unaffected.
 * Every hessian_response plane has a +0.0 ring and thr <= 0, so agx_planes_enqueue's d_response is never refused.  A frame
 * with width or height below 3 has no interior: count 0, AGX_CLUSTERS_OK.
 * d_response: 4-byte aligned; frame f, row y starts at f*frame_stride_bytes + y*row_stride_bytes; strides are multiples of 4,
 * row_stride_bytes >= 4*width, frame_stride_bytes >= height*row_stride_bytes; width, height >= 2; only the width floats of a
 * row are read.  clusters_per_frame in 1 .. 16384.  Anything else is AGX_ERR_ARG (a batch in flight stays where it is).
 * Results, frame f: d_counts[f], d_status[f] (AGX_CLUSTERS_*), d_clusters[f*clusters_per_frame + i] for i below the count and,
 * if d_points is given, the agx_point (cx, cy) at the same slot -- with d_counts a valid d_points / points_per_frame / d_counts
 * of agx_refine_points_enqueue[_h] as it stands.  Slots at or beyond the count are not written; a frame whose status is not
 * AGX_CLUSTERS_OK (INEXACT aside) writes no row.  d_clusters, d_counts, d_status: caller-owned device memory (4-byte aligned),
 * or all NULL: internal buffers, copied out by agx_clusters_fetch; d_points is optional on its own.
 * A seventh kind of batch on the handle: it replaces whatever is in flight without waiting, the other kinds' fetches of it are
 * AGX_ERR_STATE.  It runs on the handle's workspace (agx_detector_set_limits, option "force_generic" apply); HIP graphs: one
 * eager batch of the geometry first, as for agx_saddles_batch_enqueue. */
enum { AGX_CLUSTERS_OK = 0,
       AGX_CLUSTERS_CAPACITY = 1, /* more clusters than clusters_per_frame (at most 16384 can be listed): the true count, no row */
       AGX_CLUSTERS_BORDER = 2,   /* a pixel of the outermost ring is below the threshold: count 0, no row */
       AGX_CLUSTERS_OVERFLOW = 3, /* an internal list overflowed (agx_detector_set_limits): count 0, no row */
       AGX_CLUSTERS_INEXACT = 256 /* 0x100, a flag OR'd into OK / CAPACITY: a coordinate sum reached 2^24 */ };
int agx_clusters_enqueue(agx_detector *det, const float *d_response, int n_frames, int width, int height,
                         size_t row_stride_bytes, size_t frame_stride_bytes, uint32_t clusters_per_frame,
                         agx_cluster_info *d_clusters, void *d_points, uint32_t *d_counts, uint32_t *d_status);
/* Wait for the batch of agx_clusters_enqueue (src/detector.rs:414-429).  Internal buffers: counts and status ([n_frames],
 * required) and clusters ([n_frames][clusters_per_frame]) receive what the batch wrote, points ([n_frames][clusters_per_frame]
 * agx_point, may be NULL) the (cx, cy) of the rows -- copied from the enqueue's d_points where that was given --; slots at or
 * beyond a frame's count stay as they were.  Caller-owned device arrays: all four are NULL, the call only waits.  AGX_ERR_STATE: no such batch in flight (another kind, none, or fetched
 * already). */
int agx_clusters_fetch(agx_detector *det, agx_cluster_info *clusters, void *points, uint32_t *counts, uint32_t *status);
/* The same (src/detector.rs:414-429) for one plane in HOST memory: uploads it, runs a batch of one with cap rows and fetches it.
 * *n_out = the count, *status an AGX_CLUSTERS_* value; out receives the rows of an AGX_CLUSTERS_OK frame.  response and
 * row_stride_bytes as d_response's (4-byte aligned, a multiple of 4, >= 4*width), cap as clusters_per_frame: anything else is
 * AGX_ERR_ARG before anything is uploaded or a batch in flight is touched. */
int agx_cluster_centers(agx_detector *det, const float *response, int width, int height, size_t row_stride_bytes,
                        agx_cluster_info *out, uint32_t cap, uint32_t *n_out, uint32_t *status);

/* The k / phi filter of refined_saddle_points -- src/detector.rs:432-445 -- on the records of agx_refine_points_enqueue, in
 * place, stream-ordered on the detector's stream, caller-owned device arrays only; nothing to fetch (like agx_planes_enqueue it
 * replaces the batch in flight).  Once per frame over the slots below the frame's count (d_counts as in
 * agx_refine_points_enqueue; NULL: points_per_frame) whose word in d_status is AGX_POINT_REFINED: max_k = the f32::MIN-started
 * max fold of their k, s_max_k = max_k / 10.0f, and a slot that fails k >= s_max_k && phi >= min_saddle_angle && phi <=
 * max_saddle_angle (the handle's params) gets AGX_POINT_FILTERED.  Records and every other word stay as they are; a frame with
 * no refined slot changes nothing (:432-434).  d_status then serves as d_point_status of agx_find_boards_enqueue, and the
 * surviving records in slot order are refined_saddle_points' Vec.  AGX_ERR_ARG: NULL or misaligned d_records / d_status,
 * n_frames <= 0, points_per_frame == 0, 2^31 slots or more. */
enum { AGX_POINT_FILTERED = 4 }; /* :436-443: k < max_k / 10, or phi outside [min_saddle_angle, max_saddle_angle] */
int agx_filter_saddles_enqueue(agx_detector *det, const agx_saddle *d_records, uint32_t *d_status, int n_frames,
                               uint32_t points_per_frame, const uint32_t *d_counts);
/* The same filter (src/detector.rs:432-445) over ONE list in host memory, without a detector handle (no device needed): n
 * records and their status words; params may be NULL (agx_default_params). */
int agx_filter_saddles_tail(const agx_params *params, const agx_saddle *records, uint32_t *status, uint32_t n);

/* ---- the rounds of max_num_of_boards on the device: tag table and used saddles ----------------- */

/* What detect's loop does with a round's board besides finding and decoding it -- src/detector.rs:510-539: every decoded quad
 * goes into detected_tags (:520) and its four saddles leave the list before the next round (:521-536).  One round per call, once
 * per frame, on the outputs of agx_find_boards_enqueue and agx_decode_quads_enqueue as they stand; stream-ordered on the
 * detector's stream (the caller's after agx_detector_set_stream), caller-owned device arrays only, no pixels, nothing to fetch
 * (like agx_filter_saddles_enqueue it replaces the batch in flight without waiting).  With it the staged chain runs detect's
 * rounds: find boards -> (agx_find_boards_fetch where a frame may be pending) -> decode -> collect, max_num_of_boards times.
 *   d_quads [n_frames][quads_per_frame][4], d_n_quads, d_board_status [n_frames]: agx_find_boards_enqueue's d_quads, d_n_quads and
 *     d_status (slot numbers within the frame);
 *   d_quad_tags, d_quad_status [n_frames*quads_per_frame]: agx_decode_quads_enqueue's d_tags and d_status;
 *   d_tags [n_frames][tags_per_frame], d_n_tags, d_tag_status [n_frames]: the frames' tag tables, in and out.  reset != 0 takes
 *     every table as empty (count 0, AGX_TAGS_OK) whatever the arrays hold: the first round needs no memset;
 *   d_point_status: the words agx_find_boards_enqueue reads as its d_point_status, or NULL: nothing is marked (the last round).
 *     Frame f's words start at f*saddles_per_frame and its slot numbers are below saddles_per_frame; with d_frame_table (the
 *     agx_frame_result entries, as in agx_find_boards_enqueue) they start at the entry's `offset` and are below its `count`.
 * A frame whose board status is AGX_BOARD_FOUND: in quad order, every quad below the count whose status is AGX_QUAD_DECODED
 * inserts (id, xy).  A new id takes the next row; a known id -- of an earlier round or an earlier quad of this one -- keeps its
 * row and takes the new corners, so the last quad in quad order wins, as HashMap::insert has it, and the rows are in order of
 * first insertion.  All four saddle slots of every decoded quad, one that only repeats an id included, get AGX_POINT_USED in
 * d_point_status.  Records and every other word are untouched; rows at or beyond the count are never written.  AGX_BOARD_NONE
 * changes nothing (the reference's loop runs on), and neither does a round that decodes nothing.
 * d_tag_status[f]: AGX_TAGS_OK, or -- decided before anything of the frame is written, and sticky: later rounds leave such a
 * frame exactly as it is --
 *   AGX_TAGS_CAPACITY  the round needs more than tags_per_frame rows: d_n_tags[f] = the number of distinct ids it would have
 *                      reached; no row is written and no word is marked this round;
 *   AGX_TAGS_INPUT     the round's board status is AGX_BOARD_CAPACITY or AGX_BOARD_INPUT (or no AGX_BOARD_* value); an
 *                      AGX_BOARD_FOUND count above quads_per_frame; a decoded quad with an id at or above the family's code
 *                      count or a slot number at or above the frame's slot bound; a table to merge into whose count is above
 *                      tags_per_frame or that holds such an id;
 *   AGX_TAGS_PENDING   the round's board status is AGX_BOARD_PENDING: agx_find_boards_fetch has to resolve it first.
 * AGX_ERR_ARG (a batch in flight stays where it is): a NULL array other than d_frame_table and d_point_status, n_frames <= 0,
 * quads_per_frame or tags_per_frame == 0, saddles_per_frame == 0 without a table, a pointer that is not 4-byte aligned, 2^31
 * or more quad rows, tag rows or (without a table) slots. */
enum { AGX_POINT_USED = 5 }; /* src/detector.rs:521-536: a saddle of a quad that an earlier round decoded */
enum { AGX_TAGS_OK = 0, AGX_TAGS_CAPACITY = 1, AGX_TAGS_INPUT = 2, AGX_TAGS_PENDING = 3 }; /* src/detector.rs:510-539, per frame */
int agx_collect_tags_enqueue(agx_detector *det, int n_frames, uint32_t quads_per_frame,
                             const uint32_t *d_quads, const uint32_t *d_n_quads, const uint32_t *d_board_status,
                             const agx_tag *d_quad_tags, const uint32_t *d_quad_status,
                             uint32_t saddles_per_frame, const void *d_frame_table, uint32_t *d_point_status,
                             uint32_t tags_per_frame, agx_tag *d_tags, uint32_t *d_n_tags, uint32_t *d_tag_status, int reset);
/* One frame and one round of the same (src/detector.rs:510-539) in HOST memory, without a detector handle (no device needed,
 * like agx_find_board_tail): family as in agx_detector_create; quads [n_quads][4] and board_status as agx_find_board_tail
 * answered (n_quads is not read unless that is AGX_BOARD_FOUND), quad_tags / quad_status [n_quads] as agx_decode_quads_tail did;
 * point_status: n_slots words, or NULL; tags [tag_cap], *n_tags and *tag_status in and out -- the caller zeroes the last two
 * for the first round.  Statuses and everything else as the batch call's.  AGX_ERR_ARG: a NULL n_tags or tag_status, tag_cap
 * == 0 or NULL tags, NULL quads, quad_tags or quad_status with an AGX_BOARD_FOUND count above 0; AGX_ERR_FAMILY. */
int agx_collect_tags_tail(int family, uint32_t n_quads, const uint32_t *quads, uint32_t board_status,
                          const agx_tag *quad_tags, const uint32_t *quad_status, uint32_t n_slots, uint32_t *point_status,
                          uint32_t tag_cap, agx_tag *tags, uint32_t *n_tags, uint32_t *tag_status);

/* ---- the board's homography from the tag table: fit, outliers, predicted corners ------------ */

/* What a calibration pipeline does with a frame's tag table {id, 4 corners} next (the reference stops at the table; its README's
 * open item "Robustness"): relate the ids to the printed board, fit the board-to-image homography through all 4 n
 * correspondences, take the RMS reprojection error as the frame's quality, throw out tags that disagree with the board (best_tag
 * accepts a Hamming distance, so a wrong id is a real event), and predict the corners of the board's OTHER tags -- the ones the
 * search missed in this frame, and all of them in the next.  The layout is Kalibr's AprilGrid: tag first_id + r*cols + c sits at
 * column c, row r; corner j of its xy is the board point (c*(1+s) + ox[j], r*(1+s) + oy[j]) with (ox, oy)[j] = (0,0), (1,0),
 * (1,1), (0,1), in units of the tag side, s = spacing_ratio, y along increasing row.
 * Per frame over tag tables in DEVICE memory, stream-ordered on the detector's stream (the caller's after
 * agx_detector_set_stream), caller-owned device arrays only; returns without waiting, nothing is handed back and there is nothing
 * to fetch.  d_tags [n_frames][tags_per_frame], d_n_tags and d_tag_status (may be NULL) [n_frames]: the tables of
 * agx_collect_tags_enqueue and agx_detect_batch_enqueue_to, read in place.  Predicted corners are agx_tag rows:
 * agx_snap_points_enqueue reads them in place (&d_pred[0].xy, row stride sizeof(agx_tag), point stride 8, d_row_counts = d_n_pred;
 * a NaN point never snaps).
 * Arithmetic (csrc/board_fit_math.h states it once for both forms): binary64, + - * / only, no contraction.  Board and image
 * coordinates are centred and scaled into [-1, 1] (board: by its extent cols*(1+s) - s by rows*(1+s) - s; image: by img_w,
 * img_h), the 8 unknowns (h33 = 1 at the board's centre) solve the normal equations, whose 44 sums are added in a fixed order --
 * 64 lanes over the rows in table order, folded by the tree l ^ 32, 16, 8, 4, 2, 1; no floating-point atomics -- by Gaussian
 * elimination with partial pivoting.  Rounds: fit on the inlier rows; the worst inlier row is the one with the largest residual
 * (the largest of its four corners' squared distances in pixels, stored as binary32), the lowest row at equal residual; if that
 * is above max_err_sq and fewer than max_drop rows have been dropped, the row becomes AGX_FIT_ROW_OUTLIER and the fit is
 * repeated from fresh sums; otherwise the rounds end.
 * Results, frame f, all required, caller-owned device memory:
 *   d_h [n_frames][9]  H, row major, board units -> pixels, w = 1 at the board's centre;
 *   d_row_status, d_err_sq [n_frames][tags_per_frame], rows below the frame's count: AGX_FIT_ROW_INLIER, AGX_FIT_ROW_OUTLIER
 *     (dropped) or AGX_FIT_ROW_OFF_BOARD (id outside [first_id, first_id + rows*cols): never in the fit, its residual is not
 *     written); the residual under the final fit (+inf where a corner's w is not > 0);
 *   d_n_inliers[f], d_rms[f]: the inlier rows and the root mean square over their 4 n_inliers correspondences;
 *   d_pred [n_frames][rows*cols] with d_n_pred[f]: {id, xy} of every tag of the layout in id order, rounded to binary32, a point
 *     whose w is not > 0 as (NaN, NaN); under AGX_FIT_PREDICT_MISSING only the tags that are not inlier rows, compacted;
 *   d_status[f]: AGX_FIT_OK; AGX_FIT_LOOSE (everything written, but after max_drop drops the worst inlier is still above
 *     max_err_sq); or, decided before the frame's first store, with d_n_pred[f] = d_n_inliers[f] = 0 and nothing else written:
 *     AGX_FIT_FEW (fewer than min_tags inlier rows at some round), AGX_FIT_SINGULAR (a pivot that is zero, not finite or not
 *     above 2^-40 of the largest diagonal sum, or a solution that is not finite), AGX_FIT_INPUT (a count above tags_per_frame or
 *     above 640 -- no family has that many codes --, a d_tag_status word that is not AGX_TAGS_OK, a non-finite corner in an
 *     on-board row).
 * Only entries below the counts are ever written.  No table is changed: outliers are reported, never removed.
 * Like agx_snap_points_enqueue the call replaces the batch in flight without waiting; every kind's fetch is AGX_ERR_STATE then.
 * AGX_ERR_ARG (a batch in flight stays where it is): a NULL array other than d_tag_status; n_frames <= 0; tags_per_frame == 0;
 * cols or rows == 0 or rows*cols > 4096; spacing_ratio not finite or <= -1; img_w or img_h <= 0; a negative or NaN max_err_sq;
 * min_tags == 0; an unknown flag; a misaligned pointer (d_h: 8 bytes, the rest 4); 2^27 or more rows in the batch. */
enum { AGX_FIT_PREDICT_MISSING = 1 }; /* flags */
enum { AGX_FIT_OK = 0, AGX_FIT_LOOSE = 1, AGX_FIT_FEW = 2, AGX_FIT_SINGULAR = 3, AGX_FIT_INPUT = 4 }; /* per frame */
enum { AGX_FIT_ROW_INLIER = 0, AGX_FIT_ROW_OUTLIER = 1, AGX_FIT_ROW_OFF_BOARD = 2 };                 /* per row */
int agx_board_fit_enqueue(agx_detector *det, int n_frames,
                          const agx_tag *d_tags, uint32_t tags_per_frame, const uint32_t *d_n_tags, const uint32_t *d_tag_status,
                          uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, int img_w, int img_h,
                          float max_err_sq, uint32_t max_drop, uint32_t min_tags, int flags,
                          double *d_h, float *d_err_sq, uint32_t *d_row_status, uint32_t *d_n_inliers, float *d_rms,
                          agx_tag *d_pred, uint32_t *d_n_pred, uint32_t *d_status);
/* The host form without a detector handle (no device needed, like agx_collect_tags_tail): ONE frame in host memory, the same
 * arithmetic, order of summation and bytes.  tags: a table of tags_per_frame rows of which n_tags are filled, tag_status its
 * status word; h [9], err_sq / row_status [n_tags], pred [rows*cols]; *status AGX_FIT_*.  AGX_ERR_ARG as the batch call's (tags,
 * err_sq and row_status may be NULL with n_tags == 0; tags_per_frame may be 0). */
int agx_board_fit_tail(const agx_tag *tags, uint32_t tags_per_frame, uint32_t n_tags, uint32_t tag_status,
                       uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, int img_w, int img_h,
                       float max_err_sq, uint32_t max_drop, uint32_t min_tags, int flags,
                       double *h, float *err_sq, uint32_t *row_status, uint32_t *n_inliers, float *rms,
                       agx_tag *pred, uint32_t *n_pred, uint32_t *status);

/* ---- the board's pose under a lens model: R, t, outliers, predicted corners ------------------ */

/* What a calibration, VIO or hand-eye pipeline computes next from a frame's tag table once the camera's intrinsics are known: the
 * pose of the printed board in the camera frame, Xc = R X + t.  agx_board_fit_enqueue's homography is exact for a pinhole only;
 * under lens distortion its RMS measures the lens, its rounds drop good tags near the border, and its predictions drift where
 * the search loses tags.  This call is that one with the camera in the model: the same tables, layout, rounds, statuses,
 * prediction rows and contract, the 8 unknowns of H replaced by the 6 of (R, t).
 * Model (OpenCV's; Kalibr's pinhole-radtan with k3 = 0): for a point (X, Y, Z) in the camera frame, x = X/Z, y = Y/Z,
 * r2 = x^2 + y^2, x' = x (1 + k1 r2 + k2 r2^2 + k3 r2^3) + 2 p1 x y + p2 (r2 + 2 x^2), y' = y (1 + ...) + p1 (r2 + 2 y^2) + 2 p2 x y,
 * u = fx x' + cx, v = fy y' + cy; a point whose Z is not > 0 has no projection (a prediction is (NaN, NaN), a residual +inf).
 * Board points: agx_board_fit_enqueue's layout in the plane Z = 0, centred on the board's centre, times tag_size (the tag's
 * side in the caller's unit): t comes out in that unit.  camera: nine doubles in the order fx, fy, cx, cy, k1,
 * k2, p1, p2, k3, HOST memory, copied by the call.  The prototypes take them as const double *: struct agx_camera below only
 * names the nine (it is asserted here to be exactly nine doubles, so &cam.fx is the argument); no prototype takes the struct.
 * Arithmetic (csrc/board_pose_math.h states it once for both forms, the order of operations included): binary64, + - * / and
 * correctly rounded square roots (the norms of the seed and of the Gram-Schmidt only), no contraction.  Seed: every inlier
 * corner undistorted by 8 steps of the fixed-point iteration, the homography to those by agx_board_fit_enqueue's sums and
 * solve, decomposed (lambda = 2 / (|h1| + |h2|), Gram-Schmidt).  Refinement: `iterations` Gauss-Newton steps on the pixel
 * residual through the full model, analytic Jacobian, local update R <- R C(w) by the Cayley map (no sin, no cos), t <- t + dt;
 * 28 sums added in agx_board_fit_enqueue's fixed order (64 lanes, the tree l ^ 32 .. 1, no floating-point atomics), the 6 x 7
 * system by the same elimination and pivot test.  Iterate 0 of a round is the pose it starts from; the round's answer is the
 * iterate with the lowest finite sum of |e|^2, the earliest at equal bits (iterate 0 if no sum is finite), so a diverging step
 * never makes the result worse than the seed; a singular system ends the round at the iterates so far.  The answer's R is
 * re-orthonormalised once.  Rounds as agx_board_fit_enqueue's on the pose's residuals; a round after a drop starts from the
 * last round's answer (the seed is not redone) with another `iterations` steps on fresh sums.
 * Results, frame f, all required, caller-owned device memory:
 *   d_pose [n_frames][12]  R row major (board -> camera), then t;
 *   d_row_status, d_err_sq, d_n_inliers, d_rms, d_pred, d_n_pred: as agx_board_fit_enqueue's, under the pose and the lens model
 *     (d_pred rows go to agx_snap_points_enqueue as they stand);
 *   d_best_iter[f]: the iterate of the last round that became the answer, 0 .. iterations;
 *   d_status[f]: AGX_FIT_OK, AGX_FIT_LOOSE, or -- decided before the frame's first store, with d_n_pred[f] = d_n_inliers[f] = 0
 *     and nothing else written -- AGX_FIT_FEW, AGX_FIT_INPUT (both as agx_board_fit_enqueue's) or AGX_FIT_SINGULAR (the seed's
 *     system or decomposition: a refused pivot, a norm that is zero or not finite; or a round's system at its iterate 0 with
 *     iterations > 0).
 * Only entries below the counts are ever written.  No table is changed.  The call replaces the batch in flight without waiting.
 * AGX_ERR_ARG (a batch in flight stays where it is): agx_board_fit_enqueue's list (without img_w, img_h), and a NULL camera, a
 * camera field that is not finite, fx or fy not > 0, tag_size not finite or not > 0, iterations > 64, d_pose not 8-byte
 * aligned. */
struct agx_camera { double fx, fy, cx, cy, k1, k2, p1, p2, k3; };
typedef struct agx_camera agx_camera;
#ifdef __cplusplus
static_assert(sizeof(agx_camera) == 9 * sizeof(double), "agx_camera: nine doubles");
#else
_Static_assert(sizeof(agx_camera) == 9 * sizeof(double), "agx_camera: nine doubles");
#endif
int agx_board_pose_enqueue(agx_detector *det, int n_frames,
                           const agx_tag *d_tags, uint32_t tags_per_frame, const uint32_t *d_n_tags, const uint32_t *d_tag_status,
                           uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, double tag_size,
                           const double *camera,
                           float max_err_sq, uint32_t max_drop, uint32_t min_tags, uint32_t iterations, int flags,
                           double *d_pose, float *d_err_sq, uint32_t *d_row_status,
                           uint32_t *d_n_inliers, float *d_rms, uint32_t *d_best_iter,
                           agx_tag *d_pred, uint32_t *d_n_pred, uint32_t *d_status);
/* The host form without a detector handle (no device needed): ONE frame in host memory, the same arithmetic, order of summation
 * and bytes.  pose [12], err_sq / row_status [n_tags], pred [rows*cols]; *status AGX_FIT_*.
 * AGX_ERR_ARG as the batch call's (tags, err_sq and row_status may be NULL with n_tags == 0; tags_per_frame may be 0). */
int agx_board_pose_tail(const agx_tag *tags, uint32_t tags_per_frame, uint32_t n_tags, uint32_t tag_status,
                        uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, double tag_size,
                        const double *camera,
                        float max_err_sq, uint32_t max_drop, uint32_t min_tags, uint32_t iterations, int flags,
                        double *pose, float *err_sq, uint32_t *row_status, uint32_t *n_inliers, float *rms, uint32_t *best_iter,
                        agx_tag *pred, uint32_t *n_pred, uint32_t *status);
/* For tests of the best-iterate rule: the host form run on the same frame, of which only *status and iter_sums [iterations + 1]
 * (8-byte aligned) are handed out -- the sum of |e|^2 of every iterate of the last round, NaN for an iterate that was not
 * reached.  AGX_ERR_ARG as agx_board_pose_tail's. */
int agx_debug_board_pose_sums(const agx_tag *tags, uint32_t tags_per_frame, uint32_t n_tags, uint32_t tag_status,
                              uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, double tag_size,
                              const double *camera,
                              float max_err_sq, uint32_t max_drop, uint32_t min_tags, uint32_t iterations, int flags,
                              uint32_t *status, double *iter_sums);

/* The same three calls under a lens model of the caller's choice: int lens_model in front of camera, everything else -- tables,
 * layout, seed, rounds, statuses, results, contract -- as above.  AGX_LENS_RADTAN: the calls above, and their bytes.
 * AGX_LENS_EQUIDISTANT: the pinhole-equidistant model of wide-angle and fisheye lenses (Kalibr's pinhole-equi, OpenCV's fisheye,
 * Kannala-Brandt with four coefficients), which no radial-tangential polynomial follows beyond a field angle of about 45 degrees.
 * For a point (X, Y, Z) in the camera frame with Z > 0: x = X/Z, y = Y/Z, r = sqrt(x^2 + y^2), theta = atan(r),
 * theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8), s = theta_d / r, u = fx s x + cx, v = fy s y + cy.
 * A point whose Z is not > 0 has no projection, as above: the model is not carried behind the camera.
 * camera: nine doubles in the order fx, fy, cx, cy, k1, k2, k3, k4, 0, HOST memory, copied by the call; the ninth must be 0
 * (struct agx_camera names the radial-tangential order only: its p1 and p2 hold k3 and k4 here).
 * Arithmetic (csrc/board_pose_math.h, for both forms): the square root of r as above; atan by + - * / alone (1 / r above 1, a
 * subtraction formula against the break points k / 8, an odd polynomial through z^13), within 1e-14 of the correctly rounded
 * value (agx_debug_pose_atan hands it out).  Small-r rule: for x^2 + y^2 < 2^-13, theta / r is the series
 * 1 - r^2/3 + r^4/5 - r^6/7 + r^8/9 and the Jacobian's (ds/dr) / r is its limit 2 (k1 - 1/3) + 4 (k2 - k1 + 1/5) r^2: a point on
 * the optical axis projects to (cx, cy) exactly and nothing is divided by zero.  Jacobian: analytic, d theta / d r = 1 / (1 + r^2),
 * no further transcendental.  Seed: an observed pixel goes to theta_d = |((u - cx) / fx, (v - cy) / fy)|, to theta by 8 Newton
 * steps on theta D(theta) = theta_d from theta = theta_d (no early exit), theta >= 1.5 rad is clamped to 1.5 rad (the seed only: a
 * pinhole ray must exist; the refinement runs through the forward model and has no such limit), and to r = tan(theta) by the
 * series of tan(theta / 8) through its 15th power and 3 doublings t <- 2 t / (1 - t^2); then the homography and its
 * decomposition as above.  A value that is not finite ends as AGX_FIT_SINGULAR.
 * AGX_LENS_DOUBLE_SPHERE: the double-sphere model (Usenko, Demmel, Cremers 2018; Kalibr's ds, Basalt's default) of lenses of
 * 180 degrees and more.  camera: nine doubles in the order fx, fy, cx, cy, xi, alpha, 0, 0, 0 (agx_camera's k1 and k2 hold xi and
 * alpha here).  For a point (X, Y, Z) in the camera frame: d1 = sqrt(X^2 + Y^2 + Z^2), k = xi d1 + Z, d2 = sqrt(X^2 + Y^2 + k^2),
 * den = alpha d2 + (1 - alpha) k, u = fx (X / den) + cx, v = fy (Y / den) + cy.  Validity: with w1 = alpha / (1 - alpha) for
 * alpha <= 0.5, else (1 - alpha) / alpha, and w2 = (w1 + xi) / sqrt(2 w1 xi + xi^2 + 1), the point has a projection iff d1 > 0 and
 * Z > -w2 d1.  Nothing else refuses it: Z <= 0 is NO refusal under this model -- a corner more than 90 degrees off the axis inside
 * that cone is fitted and predicted like any other.  w2 is computed once per call, on the host, for both forms.
 * Arithmetic: + - * / and the correctly rounded square root only -- no atan, no series, no iteration.  Jacobian: d(u, v) /
 * d(X, Y, Z) directly in closed form (not through x = X / Z).  Seed: an observed pixel goes through the closed-form unprojection
 * mx = (u - cx) / fx, my = (v - cy) / fy, r2 = mx^2 + my^2, mz = (1 - alpha^2 r2) / (alpha sqrt(1 - (2 alpha - 1) r2) + 1 - alpha),
 * ray = (mz xi + sqrt(mz^2 + (1 - xi^2) r2)) / (mz^2 + r2) (mx, my, mz) - (0, 0, xi), and (ray_x, ray_y) / ray_z enters the
 * homography.  The seed, and only the seed, clamps (a pinhole ray must exist): a pixel whose ray lies 1.5 rad or more off the axis,
 * or has ray_z <= 0, or that is outside the unprojection's domain (1 - (2 alpha - 1) r2 < 0, for alpha > 0.5 only), takes the
 * direction (mx, my) at the radius tan(1.5).  A pixel on the principal point gives (0, 0) with no division by r.
 * AGX_ERR_ARG (a batch in flight stays where it is): the calls' own list, a lens_model that is none of the three, under
 * AGX_LENS_EQUIDISTANT a ninth double that is not 0, and under AGX_LENS_DOUBLE_SPHERE an alpha outside [0, 1], a xi outside
 * (-1, 1], or a seventh, eighth or ninth double that is not exactly 0. */
enum { AGX_LENS_RADTAN = 0, AGX_LENS_EQUIDISTANT = 1 };
enum { AGX_LENS_DOUBLE_SPHERE = 2 };
int agx_board_pose_enqueue_m(agx_detector *det, int n_frames,
                             const agx_tag *d_tags, uint32_t tags_per_frame, const uint32_t *d_n_tags, const uint32_t *d_tag_status,
                             uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, double tag_size,
                             int lens_model, const double *camera,
                             float max_err_sq, uint32_t max_drop, uint32_t min_tags, uint32_t iterations, int flags,
                             double *d_pose, float *d_err_sq, uint32_t *d_row_status,
                             uint32_t *d_n_inliers, float *d_rms, uint32_t *d_best_iter,
                             agx_tag *d_pred, uint32_t *d_n_pred, uint32_t *d_status);
int agx_board_pose_tail_m(const agx_tag *tags, uint32_t tags_per_frame, uint32_t n_tags, uint32_t tag_status,
                          uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, double tag_size,
                          int lens_model, const double *camera,
                          float max_err_sq, uint32_t max_drop, uint32_t min_tags, uint32_t iterations, int flags,
                          double *pose, float *err_sq, uint32_t *row_status, uint32_t *n_inliers, float *rms, uint32_t *best_iter,
                          agx_tag *pred, uint32_t *n_pred, uint32_t *status);
int agx_debug_board_pose_sums_m(const agx_tag *tags, uint32_t tags_per_frame, uint32_t n_tags, uint32_t tag_status,
                                uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, double tag_size,
                                int lens_model, const double *camera,
                                float max_err_sq, uint32_t max_drop, uint32_t min_tags, uint32_t iterations, int flags,
                                uint32_t *status, double *iter_sums);
/* For tests of the arithmetic, no handle and no device: the host form's atan of r [n] (each >= 0 and finite) into out [n]; and
 * its projection of n points (X, Y, Z) of the camera frame, xyz [n][3], into uv [n][2] under lens_model and camera ((NaN, NaN)
 * where Z is not > 0; under AGX_LENS_DOUBLE_SPHERE where the point is outside the valid cone instead).  AGX_ERR_ARG: a NULL array with n > 0, an r that is negative or not finite; agx_board_pose_tail_m's
 * rules on lens_model and camera. */
int agx_debug_pose_atan(const double *r, uint32_t n, double *out);
int agx_debug_pose_project(int lens_model, const double *camera, const double *xyz, uint32_t n, double *uv);

/* ---- the camera from the batch: nine doubles and every frame's pose from a batch of tag tables ------------------------------- */

/* What a calibration pipeline is for.  Every call above that takes a camera takes nine doubles under a lens model; this call
 * produces them.  Inputs: the tag tables of n_frames frames (agx_collect_tags_enqueue / agx_detect_batch_enqueue_to), and what
 * agx_board_pose_enqueue_m wrote for them under the seed camera -- d_pose_in [n_frames][12], d_row_status, d_fit_status (its
 * d_pose, d_row_status, d_status), read in place.  A frame is usable iff its d_fit_status word is AGX_FIT_OK (AGX_FIT_LOOSE too
 * under AGX_CALIB_ACCEPT_LOOSE), its table is within tags_per_frame and 640 rows, its d_tag_status word (when given) is
 * AGX_TAGS_OK, and at least min_tags of its rows are marked AGX_FIT_ROW_INLIER with an id on the board; those rows' 4 corners
 * are its correspondences.  This is fixed for the whole call: there are no outlier rounds here -- alternate this call with the
 * pose call, whose rounds do that.
 * Minimised: the sum of squared pixel residuals over the camera's free doubles and the 6 pose unknowns of every usable frame, by
 * `iterations` Levenberg-damped Gauss-Newton steps with the poses eliminated frame by frame (the Schur complement): per frame the
 * 136 sums of J^T J, J^T e and |e|^2 in agx_board_fit_enqueue's fixed order of summation, diagonals times (1 + damping), the
 * 6 x 16 elimination; the frames' reduced 9 x 9 blocks folded in frame order by the same lane / tree rule, scaled symmetrically by
 * their diagonal, and solved under the 2^-40 pivot rule.  csrc/calib_math.h states it once for both forms: binary64, + - * / and
 * the correctly rounded square root, no contraction.  The parameter Jacobian is analytic for all three lens models.
 * camera: the seed, nine HOST doubles under lens_model (agx_board_pose_enqueue_m's rules).  fixed_mask: bit i holds camera double
 * i at the seed's bits; the slots a lens model defines as 0 are always held.  Iterate 0 is the inputs; the outputs are the
 * iterate with the lowest finite total cost, the lowest iterate at equal cost (iterate 0 while none is finite), so the result is
 * never worse than the inputs.  An iterate whose camera leaves the model's domain (fx <= 0, alpha outside [0, 1], ...) has cost
 * +inf; it, an iterate with a corner that has no projection, and a refused system end the steps at the iterates so far.
 * Results, caller-owned device memory, all required:
 *   d_camera [9];  d_pose [n_frames][12], written for usable frames only, may be d_pose_in itself;
 *   d_frame_n [n_frames]: the frame's correspondences (0: not usable);  d_frame_cost [n_frames]: its sum of |e|^2 at the answer;
 *   d_report: one struct agx_calib_report (8-byte aligned) -- status AGX_CALIB_*, the answer's iterate, the last iterate
 *     evaluated, the usable frames, their correspondences, the answer's RMS in pixels, and cost[i], the total |e|^2 of iterate i
 *     (NaN: not reached).
 * AGX_CALIB_FEW: fewer usable frames than min_frames, or fewer correspondences (corners) than free unknowns (free camera doubles
 * + 6 per usable frame).  The count is of corners, not of equations, although a corner gives two: the rule is stricter than the
 * problem needs and refuses some batches that are determined -- three frames of one tag each with eight doubles free, say (12
 * corners, 24 equations, 26 unknowns is refused rightly; with the camera held, 12 against 18 is refused although 24 equations
 * determine it) -- and never one that is not.  AGX_CALIB_SINGULAR: iterate 0's system is refused by the pivot rule (the frames do not determine the free
 * doubles: fx against the distance of fronto-parallel boards, say).  Under both only d_report is written.
 * 2 (iterations + 1) + 1 launches, stream-ordered; the state stays in a workspace on the handle and nothing returns to the host.
 * The call replaces the batch in flight without waiting.  AGX_ERR_ARG (a batch in flight stays where it is): a NULL array
 * (d_tag_status may be NULL), n_frames outside 1 .. 65535, tags_per_frame == 0, rows * cols outside 1 .. 4096, a spacing_ratio
 * that is not finite or not > -1, agx_board_pose_enqueue_m's rules on lens_model, camera and tag_size, a damping that is negative
 * or not finite, iterations > 64, min_tags or min_frames == 0, fixed_mask >= 512, an unknown flag, a binary64 array or the report
 * not 8-byte aligned, another array not 4-byte aligned, 2^27 tag rows or more. */
enum { AGX_CALIB_OK = 0, AGX_CALIB_FEW = 1, AGX_CALIB_SINGULAR = 2 };
enum { AGX_CALIB_ACCEPT_LOOSE = 1 };
struct agx_calib_report {
    uint32_t status, best_iter, iterations_run, n_frames_used, n_corners, reserved;
    double rms;
    double cost[65];
};
typedef struct agx_calib_report agx_calib_report;
int agx_calibrate_enqueue(agx_detector *det, int n_frames,
                          const agx_tag *d_tags, uint32_t tags_per_frame, const uint32_t *d_n_tags, const uint32_t *d_tag_status,
                          uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, double tag_size,
                          int lens_model, const double *camera,
                          uint32_t fixed_mask, double damping, uint32_t iterations, uint32_t min_tags, uint32_t min_frames, int flags,
                          const double *d_pose_in, const uint32_t *d_row_status, const uint32_t *d_fit_status,
                          double *d_camera, double *d_pose, float *d_frame_cost, uint32_t *d_frame_n, void *d_report);
/* The host form without a detector handle (no device needed): n_frames frames in host memory, the same arithmetic, order of
 * summation and bytes.  AGX_ERR_ARG as the batch call's. */
int agx_calibrate_tail(int n_frames,
                       const agx_tag *tags, uint32_t tags_per_frame, const uint32_t *n_tags, const uint32_t *tag_status,
                       uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, double tag_size,
                       int lens_model, const double *camera,
                       uint32_t fixed_mask, double damping, uint32_t iterations, uint32_t min_tags, uint32_t min_frames, int flags,
                       const double *pose_in, const uint32_t *row_status, const uint32_t *fit_status,
                       double *camera_out, double *pose, float *frame_cost, uint32_t *frame_n, void *report);
/* The closed-form seed, host only (OpenCV's initCameraMatrix2D): from the homographies h [n][9] of agx_board_fit_enqueue /
 * _tail (board units -> pixels) whose fit_status word is AGX_FIT_OK or AGX_FIT_LOOSE, the principal point ((img_w - 1) / 2,
 * (img_h - 1) / 2) and fx, fy from the 2 x 2 normal equations of the two orthogonality constraints per homography (Zhang 2000);
 * zero distortion: camera_out [9] = fx, fy, cx, cy, 0, 0, 0, 0, 0.  *status: AGX_CALIB_OK; AGX_CALIB_FEW (no usable homography)
 * or AGX_CALIB_SINGULAR (1 / fx^2 and 1 / fy^2 are not determined -- fronto-parallel boards -- or not positive), camera_out
 * untouched.  AGX_ERR_ARG: a NULL array, n == 0, img_w or img_h < 1. */
int agx_calibrate_seed_tail(const double *h, const uint32_t *fit_status, uint32_t n, int img_w, int img_h,
                            double *camera_out, uint32_t *status);
/* For tests of the arithmetic, no handle and no device: the 2 x 9 derivative of agx_debug_pose_project's (u, v) by the nine
 * camera doubles at n points of the camera frame, xyz [n][3], into out [n][2][9] (NaN where the point has no projection).
 * AGX_ERR_ARG as agx_debug_pose_project's. */
int agx_debug_calib_param_jacobian(int lens_model, const double *camera, const double *xyz, uint32_t n, double *out);

/* ---- the rig from the batch: the cameras' extrinsics and the board's pose at every instant from synchronised tag tables ------- */

/* What the people who print AprilGrids calibrate with them: stereo pairs, multi-camera heads, a fisheye next to a pinhole.
 * n_cams cameras (2 .. 8) look at one board at n_instants synchronised instants; frame f = c * n_instants + s is camera c at
 * instant s, n_cams * n_instants in 1 .. 65535; every array "per frame" is in that order.  Each camera has its own lens model
 * and nine doubles (lens_models [n_cams], cameras [n_cams][9]: HOST memory, copied by the call; held here -- alternate with
 * agx_calibrate_enqueue per camera to move them).
 * Unknowns: E_c, camera from rig, for c = 1 .. n_cams - 1 (E_0 is the identity and is never written differently: that fixes the
 * gauge), and T_s, rig from board, for every usable instant; both 12 doubles, R row major then t, d_pose's layout.  Minimised: the
 * sum over the counted frames' inlier corners of | project<lens_c>(camera_c, E_c o T_s o X) - observed |^2.
 * A frame is usable by agx_calibrate_enqueue's rule, word for word (d_fit_status, AGX_CALIB_ACCEPT_LOOSE, d_tag_status, the 640
 * rows, min_tags inlier rows on the board).  An instant is usable iff at least min_cams (>= 1; 2 is the usual choice) of its
 * frames are; the frames of an unusable instant do not count.  A camera c >= 1 without a counted frame is held: d_extrinsics[c]
 * keeps the seed's bits and d_cam_n[c] = 0.
 * Inputs read in place: d_pose_in [frames][12], d_row_status, d_fit_status as agx_board_pose_enqueue_m wrote them under each
 * camera; d_extrinsics_in [n_cams][12], the seed (agx_rig_seed_tail), which may be d_extrinsics itself; entry 0 is not read.
 * T_s's seed is made on the device: E_c^-1 o pose_in[c, s] for the lowest usable c of the instant.
 * The arithmetic (csrc/rig_math.h, once for both forms; binary64, + - * / and the correctly rounded square root, no
 * contraction): the update is agx_board_pose_enqueue's local Cayley update (R <- R C(w), t <- t + dt) on E_c and on T_s; per
 * counted frame the 91 sums of the 12 x 12 J^T J over [dE_c | dT_s], J^T e and |e|^2 in agx_board_fit_enqueue's fixed order
 * (camera 0's frames the T_s part alone, 28); per instant V_s and its gradient summed in camera order, diagonals times
 * (1 + damping), the 6 x 6 elimination, and the instant's contribution to the reduced 6 (n_cams - 1) square system, dense across
 * the cameras that share the instant; the contributions folded in instant order by agx_calibrate_enqueue's lane / tree rule,
 * scaled symmetrically by the diagonal and solved with partial pivoting under the 2^-40 rule; back-substitution gives dT_s.
 * Iterate 0 is the inputs; the answer is the iterate with the lowest finite total cost, the lowest iterate at ties, so it is
 * never worse than the inputs; a corner without a projection or a refused system ends the steps at the iterates so far.  A seed
 * extrinsic that is not finite cannot be refused here (it is device memory): it makes iterate 0's cost not finite, the call
 * ends at iterate 0 and the seed is the answer.
 * Results, caller-owned device memory, all required: d_extrinsics [n_cams][12] (entry 0 the identity); d_rig_pose
 * [n_instants][12], written for usable instants only; d_frame_n [frames]: the frame's correspondences (0: not counted);
 * d_frame_cost [frames]: its sum of |e|^2 at the answer; d_cam_n [n_cams]: the camera's counted frames; d_report: one struct
 * agx_rig_report (8-byte aligned).
 * AGX_RIG_FEW: fewer usable instants than min_instants, no free camera, or fewer corners than 6 * n_cams_free + 6 *
 * n_instants_used.  AGX_RIG_SINGULAR: iterate 0's reduced system is refused by the pivot rule -- undamped, two groups of cameras
 * that never share an instant (cameras 0, 1 at some instants, 2, 3 at others, min_cams = 2: nothing ties the second group to the
 * first).  Under both only d_report is written.
 * 3 (iterations + 1) launches (k_rig_blocks, k_rig_instants, k_rig_solve per iterate), stream-ordered; the state stays in a
 * workspace on the handle and nothing returns to the host.  The call replaces the batch in flight without waiting.
 * AGX_ERR_ARG (a batch in flight stays where it is): a NULL array (d_tag_status may be NULL), n_cams outside 2 .. 8, a frame
 * count outside 1 .. 65535, agx_board_pose_enqueue_m's rules on any camera and on tag_size, agx_calibrate_enqueue's rules on
 * the layout, damping, iterations, min_tags, min_instants (as its min_frames), flags and alignment, min_cams == 0. */
enum { AGX_RIG_OK = 0, AGX_RIG_FEW = 1, AGX_RIG_SINGULAR = 2 };
enum { AGX_RIG_CAM_ATTACHED = 0, AGX_RIG_CAM_DETACHED = 1 };
struct agx_rig_report {
    uint32_t status, best_iter, iterations_run, n_instants_used, n_frames_used, n_corners, n_cams_free, reserved;
    double rms;
    double cost[65];
};
typedef struct agx_rig_report agx_rig_report;
int agx_rig_calibrate_enqueue(agx_detector *det, int n_cams, int n_instants,
                              const agx_tag *d_tags, uint32_t tags_per_frame, const uint32_t *d_n_tags, const uint32_t *d_tag_status,
                              uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, double tag_size,
                              const int *lens_models, const double *cameras,
                              double damping, uint32_t iterations, uint32_t min_tags, uint32_t min_cams, uint32_t min_instants, int flags,
                              const double *d_pose_in, const uint32_t *d_row_status, const uint32_t *d_fit_status,
                              const double *d_extrinsics_in, double *d_extrinsics, double *d_rig_pose,
                              float *d_frame_cost, uint32_t *d_frame_n, uint32_t *d_cam_n, void *d_report);
/* The host form without a detector handle (no device needed): the same arithmetic, order of summation and bytes.  AGX_ERR_ARG
 * as the batch call's, and a seed extrinsic that is not finite (readable here). */
int agx_rig_calibrate_tail(int n_cams, int n_instants,
                           const agx_tag *tags, uint32_t tags_per_frame, const uint32_t *n_tags, const uint32_t *tag_status,
                           uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, double tag_size,
                           const int *lens_models, const double *cameras,
                           double damping, uint32_t iterations, uint32_t min_tags, uint32_t min_cams, uint32_t min_instants, int flags,
                           const double *pose_in, const uint32_t *row_status, const uint32_t *fit_status,
                           const double *extrinsics_in, double *extrinsics, double *rig_pose,
                           float *frame_cost, uint32_t *frame_n, uint32_t *cam_n, void *report);
/* The closed-form seed, host only: pose [frames][12] and fit_status [frames] of agx_board_pose_enqueue_m per camera; frame_n
 * [frames] (correspondences per frame) or NULL.  Cameras are attached level by level from camera 0: a camera c that is not
 * attached yet attaches through the lowest-numbered camera r attached in an earlier level with which it shares an instant where
 * both status words are AGX_FIT_OK (and, with frame_n, both counts are > 0); among those instants the one with the largest
 * frame_n[c, s] + frame_n[r, s], the lowest s at ties (and with frame_n NULL);  E_c = pose[c, s] o pose[r, s]^-1 o E_r.
 * extrinsics_out [n_cams][12]; cam_status [n_cams]: AGX_RIG_CAM_ATTACHED, or AGX_RIG_CAM_DETACHED with the identity.
 * AGX_ERR_ARG: a NULL array (frame_n may be NULL), n_cams outside 2 .. 8, a frame count outside 1 .. 65535. */
int agx_rig_seed_tail(int n_cams, int n_instants, const double *pose, const uint32_t *fit_status, const uint32_t *frame_n,
                      double *extrinsics_out, uint32_t *cam_status);
/* For tests of the arithmetic, no handle and no device: the derivative of the projected pixel of the board points XY [n][2]
 * (Z = 0) under camera, extrinsic [12] and rig_pose [12] by the 6 + 6 update unknowns (w, dt of E_c, then of T_s; the residual
 * observed - projected has the opposite sign), out [n][2][12]; NaN where the point has no projection.  extrinsic NULL: camera
 * 0, whose first six columns are 0.  AGX_ERR_ARG as agx_debug_pose_project's. */
int agx_debug_rig_jacobian(int lens_model, const double *camera, const double *extrinsic, const double *rig_pose, const double *XY,
                           uint32_t n, double *out);

/* ---- rectified batches: the lens model applied to the pixels (csrc/rectify.hip; the arithmetic once, in csrc/rectify_math.h) ---- */

/* Everything above works on the tag table, behind the detection; these three work in front of it.  The board search assumes a
 * straight lattice and the decode samples through an affine or projective map: neither knows about the lens, and on a strong
 * fisheye tags are lost.  A rectified batch -- the frames as the ideal pinhole `new_camera` would have seen them -- is also what
 * stereo matching, the straight-lattice agx_board_fit_enqueue and consumers outside this library expect of a calibrated camera.
 *
 * THE MAP, once per camera (k_rectify_map; one lane per destination pixel; not the hot path).  For destination pixel (i, j) of a
 * dst_width x dst_height pinhole new_camera = fx' fy' cx' cy' (four doubles, HOST memory, copied by the call): the ray
 * d = ((i - cx') / fx', (j - cy') / fy', 1); (X, Y, Z) = R d with rotation = R, nine doubles, row major, rectified frame ->
 * camera frame, HOST memory (NULL: the identity); (u, v) = the projection of (X, Y, Z) under lens_model and camera -- the one of
 * agx_board_pose_enqueue_m, the function agx_debug_pose_project hands out, binary64 in its order of operations.  The entry is two
 * int (32-bit) words in units of 1/32 source pixel, mx = floor(32 u + 1/2), my = floor(32 v + 1/2) in binary64, valid if the
 * projection exists (Z > 0, under AGX_LENS_DOUBLE_SPHERE Z > -w2 d1 instead; u and v finite) and 0 <= mx <= 32 (src_width - 1), 0 <= my <= 32 (src_height - 1); otherwise both
 * words are AGX_MAP_NONE.  d_map [dst_height][dst_width][2] with map_row_stride_bytes between rows (a multiple of 8, at least
 * 8 dst_width; padding bytes are not written), caller-owned device memory, 8-byte aligned; stream-ordered, nothing to fetch; a
 * batch in flight is replaced as by agx_board_fit_enqueue.
 * The caller's responsibility: the radial-tangential polynomial is applied as it stands.  Beyond the radius where it stops being
 * monotone, far rays fold back into the image (as in OpenCV's initUndistortRectifyMap); choosing new_camera and the target size
 * inside that radius is the caller's job.  The equidistant model has no such radius below Z = 0.  The double-sphere model
 * is carried past Z = 0: a rotated ray with Z <= 0 inside the valid cone has a map entry and a rectified point.
 * AGX_ERR_ARG (a batch in flight stays where it is): agx_board_pose_enqueue_m's rules on lens_model and camera; a NULL or
 * non-finite new_camera, or fx' or fy' not > 0; a non-finite rotation; a size below 1 or above 16384; a NULL or misaligned d_map,
 * a stride that is no multiple of 8 or below 8 dst_width.
 * agx_rectify_map_tail: the host form -- no handle, no device, the same bytes. */
#define AGX_MAP_NONE (-2147483647 - 1)
int agx_rectify_map_enqueue(agx_detector *det, int lens_model, const double *camera, const double *new_camera, const double *rotation,
                            int src_width, int src_height, int dst_width, int dst_height,
                            int *d_map, size_t map_row_stride_bytes);
int agx_rectify_map_tail(int lens_model, const double *camera, const double *new_camera, const double *rotation,
                         int src_width, int src_height, int dst_width, int dst_height,
                         int *map, size_t map_row_stride_bytes);

/* THE REMAP, once per batch (k_remap; the hot path).  d_src: n_frames frames of src_width x src_height, AGX_L8 or AGX_L16, row and
 * frame strides as in every batch entry; d_dst: n_frames frames of dst_width x dst_height in the same format with their own
 * strides; d_map as above (the caller's own map is as good).  Per destination pixel with entry (mx, my): AGX_MAP_NONE, or any
 * entry that is not inside the source (0 <= mx <= 32 (src_width - 1), 0 <= my <= 32 (src_height - 1)), gives `border`; otherwise
 * x0 = mx >> 5, ax = mx & 31, x1 = min(x0 + 1, src_width - 1), the same in y, and
 *   value = ((32 - ax)(32 - ay) p00 + ax (32 - ay) p10 + (32 - ax) ay p01 + ax ay p11 + 512) >> 10     in uint32
 * -- bilinear with 5-bit weights, round half up.  No floating-point operation in the kernel or in the host form; nothing outside
 * the source frames is read, nothing outside the destination rows' dst_width pixels is written.  Caller-owned device memory,
 * stream-ordered, nothing to fetch; a batch in flight is replaced as by agx_board_fit_enqueue.  Source and destination must not
 * overlap.
 * AGX_ERR_ARG (a batch in flight stays where it is): a NULL array; n_frames outside 1 .. 65535; a format other than AGX_L8 and
 * AGX_L16 (the luma front is not part of this); a source side outside 1 .. 65000 or a source frame of 2^30 px or more; a
 * destination side outside 1 .. 16384; a row stride that does not cover a row, a frame stride (n_frames > 1) that does not cover
 * a frame, a frame (row stride x height) of 2^31 bytes or more; AGX_L16 pointers or strides that are odd; the map's rules above;
 * border above 255 (AGX_L8) or 65535 (AGX_L16).
 * agx_remap_tail: the host form -- no handle, no device, the same bytes. */
int agx_remap_enqueue(agx_detector *det, const void *d_src, int n_frames, int src_width, int src_height,
                      size_t src_row_stride_bytes, size_t src_frame_stride_bytes, int format,
                      const int *d_map, size_t map_row_stride_bytes, int dst_width, int dst_height,
                      void *d_dst, size_t dst_row_stride_bytes, size_t dst_frame_stride_bytes, uint32_t border);
int agx_remap_tail(const void *src, int n_frames, int src_width, int src_height,
                   size_t src_row_stride_bytes, size_t src_frame_stride_bytes, int format,
                   const int *map, size_t map_row_stride_bytes, int dst_width, int dst_height,
                   void *dst, size_t dst_row_stride_bytes, size_t dst_frame_stride_bytes, uint32_t border);

/* POINTS BACK TO THE SENSOR (k_rectified_points).  Point i of n_points is two floats (x, y), rectified pixels, at
 * d_points + i * point_stride_bytes; it goes through the map's ray, rotation and projection (binary64; the map's entry is this
 * function at integer positions) and (u, v), sensor pixels, rounded to binary32, is written at d_out + i * out_stride_bytes;
 * (NaN, NaN) for a point with no projection (a point that is not finite among them).  In place (d_out = d_points, the same
 * stride) is allowed.  Corner j of an agx_tag table is read in place at (char *)d_tags + 4 + 8 j with a stride of 36: four calls
 * put a table detected in the rectified batch into sensor pixels, which is what agx_board_pose_enqueue_m wants for residuals in
 * sensor pixels.  Caller-owned device memory, stream-ordered, nothing to fetch; a batch in flight is replaced as above.
 * AGX_ERR_ARG: the map's rules on lens_model, camera, new_camera and rotation; a NULL list with n_points > 0; 2^30 points or
 * more; a pointer or stride that is no multiple of 4, a stride below 8.
 * agx_rectified_points_tail: the host form. */
int agx_rectified_points_enqueue(agx_detector *det, int lens_model, const double *camera, const double *new_camera,
                                 const double *rotation, const void *d_points, size_t point_stride_bytes, uint32_t n_points,
                                 void *d_out, size_t out_stride_bytes);
int agx_rectified_points_tail(int lens_model, const double *camera, const double *new_camera, const double *rotation,
                              const void *points, size_t point_stride_bytes, uint32_t n_points,
                              void *out, size_t out_stride_bytes);

/* ---- the board through the lens: a pose and a camera to the pixels the sensor sees (csrc/render.hip; csrc/render_math.h) ---- */

/* The forward model of agx_board_pose_enqueue_m, applied to the printed board itself: for every frame f of a device batch the
 * board of the layout (cols, rows, first_id, spacing_ratio; tag first_id + r cols + c at column c, row r; the plane Z = 0 centred on
 * the board's centre, in tag_size's unit -- agx_board_pose_enqueue's board frame) as the camera (lens_model, camera: nine HOST
 * doubles, agx_board_pose_enqueue_m's rules) sees it from the pose d_poses[f] = 12 doubles, R row major then t: exactly
 * agx_board_pose_enqueue_m's d_pose, readable in place.  For overlays of the board at an estimated pose, synthetic batches under
 * any lens without a host round trip, and ground truth that is the forward model itself (k_render_boards<LENS>).
 * d_frames: n_frames frames of width x height, AGX_L8 or AGX_L16, row and frame strides as in every batch entry.  `family`'s code
 * table (agx_family) gives the tags' bits.  params: HOST memory, copied by the call -- struct agx_render_params below names its
 * six 32-bit fields (the prototypes take it as const void *): black, white, background in the format's range; page_margin, the
 * white border around the board in tag sides; supersample S in 1 .. 4; flags.
 * A pixel (i, j) takes S x S samples at (i + (a + 1/2) / S - 1/2, j + (b + 1/2) / S - 1/2).  A sample (u, v) is inverted to the
 * board point (X, Y) whose FORWARD projection -- the one of agx_debug_pose_project -- is (u, v): a seed from the lens's
 * unprojection and the ray's intersection with the board's plane, then 4 Newton steps on the 2 x 2 system with the pose's own
 * analytic Jacobian (no early exit).  The sample is on the page iff that point projects, its projection lies within 2^-20 px of
 * (u, v), and (X, Y) lies on the page; any other sample -- outside the double-sphere cone, or with Z not > 0 under the other two
 * models, among them -- is background.  No clamp of the seed decides by itself.  The board: a black square of side spacing_ratio
 * at every lattice point (the outer ring included), every tag with its black border and the family's code bits, rows printed
 * from the high end of Y (Kalibr's board, y up), white elsewhere on the page: the tag's corners in the order (0,0), (1,0),
 * (1,1), (0,1) of its board square decode to its own id at quarter turn 0.  Shading is integer only:
 *   value = (n_white white + n_black black + n_bg bg + S S / 2) / (S S)      in uint32,
 * bg = background, or under AGX_RENDER_KEEP_BACKGROUND the pixel's current value (an overlay on a real frame; a pixel with no
 * sample on the page is then not written at all).  Binary64 with + - * / and correctly rounded square roots up to the
 * classification, nothing floating after it.  Never a byte beyond `width` pixels of a row is written.
 * Ground truth: d_truth [n_frames][rows cols] agx_tag rows {id, xy} of every tag of the layout in id order with d_n_truth[f] =
 * rows cols -- the bytes agx_board_pose_enqueue_m's d_pred has for the same pose, (NaN, NaN) for a corner without a projection;
 * the rows feed agx_snap_points_enqueue and agx_decode_quads_enqueue in place.
 * d_status[f], decided before the frame's first store: AGX_RENDER_OK; AGX_RENDER_EMPTY, none of the board's four outer corners
 * projects (the frame is all background, or under AGX_RENDER_KEEP_BACKGROUND untouched; d_n_truth[f] = 0); AGX_RENDER_INPUT, a
 * pose entry that is not finite or two columns of R whose dot product is further than 2^-20 from 1 (with itself) or 0 (nothing of
 * the frame is written; d_n_truth[f] = 0).  Caller-owned device memory, stream-ordered, nothing to fetch; a batch in flight is
 * replaced as by agx_board_fit_enqueue.
 * AGX_ERR_FAMILY: an unknown family.  AGX_ERR_ARG (a batch in flight stays where it is): a NULL array; n_frames outside
 * 1 .. 65535; a format other than AGX_L8 and AGX_L16; a side outside 1 .. 16384; agx_remap_enqueue's rules on strides and 16-bit
 * alignment; rows cols outside 1 .. 4096, a spacing_ratio that is negative or not finite; agx_board_pose_enqueue_m's rules on
 * lens_model, camera and tag_size; first_id + rows cols beyond the family's code table; S outside 1 .. 4; a colour above 255
 * (AGX_L8) or 65535 (AGX_L16); a page_margin that is negative or not finite; an unknown flag; d_poses not 8-byte aligned, another
 * array not 4-byte aligned.
 * agx_render_boards_tail: the host form -- ONE frame in host memory, no handle, no device, the same bytes. */
enum { AGX_RENDER_OK = 0, AGX_RENDER_EMPTY = 1, AGX_RENDER_INPUT = 2 };
enum { AGX_RENDER_KEEP_BACKGROUND = 1 };
struct agx_render_params { uint32_t black, white, background; float page_margin; uint32_t supersample, flags; };
typedef struct agx_render_params agx_render_params;
#ifdef __cplusplus
static_assert(sizeof(agx_render_params) == 24, "agx_render_params: six 32-bit fields");
#else
_Static_assert(sizeof(agx_render_params) == 24, "agx_render_params: six 32-bit fields");
#endif
int agx_render_boards_enqueue(agx_detector *det, int n_frames, int width, int height,
                              size_t row_stride_bytes, size_t frame_stride_bytes, int format, int family,
                              uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, double tag_size,
                              int lens_model, const double *camera, const double *d_poses, const void *params,
                              void *d_frames, agx_tag *d_truth, uint32_t *d_n_truth, uint32_t *d_status);
int agx_render_boards_tail(int width, int height, size_t row_stride_bytes, int format, int family,
                           uint32_t cols, uint32_t rows, uint32_t first_id, float spacing_ratio, double tag_size,
                           int lens_model, const double *camera, const double *pose, const void *params,
                           void *frame, agx_tag *truth, uint32_t *n_truth, uint32_t *status);

/* ---- detector groups: several GPUs of one node driven from ONE process ----------------- */

/* The reference's detect(&self) is stateless, so a batch shards by frame:
 * rank r of a group owns one device, runs the whole chain for its own frames on its own stream,
 * and the only exchange step is the gather of the per-rank result slabs to the root device
 * (devices[0]).  A Rust host drives all GPUs of a node through these calls without torch. */
typedef struct agx_group agx_group;
enum {
    AGX_GATHER_RCCL = 0, /* ncclSend / ncclRecv in one group over xGMI (librccl opened on first use);
                            devices must be distinct */
    AGX_GATHER_PEER = 1  /* hipMemcpyPeerAsync + events over the same links; accepts a device more than
                            once (test configuration on one-GPU boxes) */
};
/* One detector (TagDetector::new, src/detector.rs:364-406) per entry of devices[] (NULL:
 * 0..n_devices-1). */
int agx_group_create(int family, const agx_params *params, const int *devices, int n_devices, int transport,
                     agx_group **out);
void agx_group_destroy(agx_group *group);
int agx_group_size(const agx_group *group);
/* Borrow rank r's detector (limits, options, profiling); owned by the group. */
agx_detector *agx_group_detector(agx_group *group, int rank);
/* refined_saddle_points (src/detector.rs:408-446) over n_devices * frames_per_rank frames: rank r's
 * frames are resident on ITS device at d_frames[r] (layout as agx_saddles_batch_enqueue).  Enqueues
 * every rank's chain and the gather and returns without waiting.  records_per_frame: average saddle
 * records per frame the per-rank result slab holds (0 = 512). */
int agx_group_saddles_enqueue(agx_group *group, const void *const *d_frames, int frames_per_rank, int width,
                              int height, size_t row_stride_bytes, size_t frame_stride_bytes, int format,
                              uint32_t records_per_frame);
/* Wait for the gather; frame f of rank r is global frame r*frames_per_rank + f of out / counts /
 * frame_status (sized n_devices*frames_per_rank, as agx_saddles_batch_fetch). */
int agx_group_saddles_fetch(agx_group *group, agx_saddle *out, uint32_t cap_per_frame, uint32_t *counts,
                            int *frame_status);
/* detect (src/detector.rs:505-540) over n_devices * frames_per_rank frames, rank r's resident on ITS device at
 * d_frames[r]; layout and formats as agx_detect_batch_enqueue (every agx_format but AGX_LF32, which is
 * AGX_ERR_FORMAT).  Enqueues every rank's chain, to_luma8, device tail (where option "device_tail" of the rank's
 * detector and this process allow it, as agx_detect_batch_enqueue) and the pack kernel -- frame table + the frames'
 * tag records back to back, in frame order -- and then the gather of the per-rank tables and tag slabs to the root
 * device, and returns without waiting; the frames must stay in place until agx_group_detect_fetch has returned.
 * tags_per_frame: average tag records per frame the per-rank slab holds (0 = 128).  AGX_ERR_ARG for more than
 * 65535 frames per rank, or a slab (frames_per_rank * tags_per_frame records of 36 bytes) of 2^31 bytes or more.
 * One batch per group is in
 * flight, of either kind: a later enqueue replaces it; fetching it with the other kind's fetch, or with a borrowed
 * detector's own agx_detect_batch_fetch / agx_saddles_batch_fetch, is AGX_ERR_STATE. */
int agx_group_detect_enqueue(agx_group *group, const void *const *d_frames, int frames_per_rank, int width,
                             int height, size_t row_stride_bytes, size_t frame_stride_bytes, int format,
                             uint32_t cap_per_frame, uint32_t tags_per_frame);
/* Wait for the gather; then the frames the device tails handed back (without the device tail: every frame) take the
 * host tail on their own rank's device data, the ranks in turn, each on n_threads host threads (0 =
 * agx_host_parallelism()).  Frame f of rank r is global frame r*frames_per_rank + f of out ([n][cap_per_frame] of
 * the enqueue), counts and frame_status (may be NULL); per frame as agx_detect_batch_fetch -- and AGX_ERR_CAPACITY
 * with the true count and no row for a frame that found its rank's slab full (agx_group_last_error names the rank,
 * the frame and the slab; tags_per_frame = the largest count always fits).  Nothing is ever truncated.  Returns the
 * first non-OK frame status, else AGX_OK.  The batch is resolved by this call: a second fetch, or a fetch with
 * nothing enqueued, is AGX_ERR_STATE (a NULL group or NULL counts is AGX_ERR_ARG whatever is in flight; the state is
 * checked next, and only then a NULL out against the cap_per_frame of the batch in flight: AGX_ERR_ARG, the batch
 * stays in flight).  Afterwards options "last_device_tail_frames" / "_fallbacks" / "_uncertain" of
 * agx_group_detector(group, r) describe rank r's share of the batch. */
int agx_group_detect_fetch(agx_group *group, agx_tag *out, uint32_t *counts, int *frame_status, int n_threads);
/* group == NULL: the reason of this thread's last failed agx_group_create. */
const char *agx_group_last_error(const agx_group *group);

/* Host tail only: TagDetector::detect's board search + decode (src/detector.rs:510-539)
 * from a saddle list and the u8 luma plane (to_luma8, :507), both in host memory.
 * saddles is not modified. */
int agx_detect_from_saddles(const agx_detector *det, const agx_saddle *saddles, uint32_t n_saddles,
                            const uint8_t *luma8, int width, int height, size_t row_stride_bytes,
                            agx_tag *out, uint32_t cap, uint32_t *n_out);

/* The same host tail without a detector handle (no device needed): family and params as in
 * agx_detector_create (params may be NULL). */
int agx_detect_tail(int family, const agx_params *params, const agx_saddle *saddles, uint32_t n_saddles,
                    const uint8_t *luma8, int width, int height, size_t row_stride_bytes, agx_tag *out,
                    uint32_t cap, uint32_t *n_out);

/* The same with the board search of the frame on n_threads host threads (created for this call; a
 * detector handle keeps its own: option "tail_threads").  Same result as n_threads = 1. */
int agx_detect_tail_threads(int family, const agx_params *params, const agx_saddle *saddles, uint32_t n_saddles,
                            const uint8_t *luma8, int width, int height, size_t row_stride_bytes, agx_tag *out,
                            uint32_t cap, uint32_t *n_out, int n_threads);

/* to_luma8 (src/detector.rs:507) of a host image (any agx_format but AGX_LF32) into a tightly packed host plane. */
int agx_luma8(const void *pixels, int width, int height, size_t row_stride_bytes, int format,
              uint8_t *out);

/* ---- measurement and parity-test hooks ------------------------------------------------ */

/* Per-kernel device time of the chain, from hipEvents recorded on the detector's stream
 * around each launch while profiling is on.  names/ms/launches are arrays of
 * AGX_N_KERNELS entries (the chain has four launches since round 3: entries behind the last one
 * carry a NULL name and zeros); ms accumulates since the last reset.  At a blur sigma other than 1.5
 * (agx_detector_set_blur_sigma) the launches of the any-sigma front -- k_gauss_blur, k_response_front -- are NOT timed and entry 0
 * stays as it is; the sparse stages' entries are timed as ever (tools/bench_sigma.py brackets the rest with its own events).
 * Likewise at a chain half_size_patch that defers the refinement (agx_detector_set_half_size_patch): k_generic_cluster and
 * k_refine_clusters are NOT timed, the flood entry then times the clustering alone and the last entry the emission alone
 * (tools/bench_patch.py brackets the sparse stages with its own events). */
#define AGX_N_KERNELS 5
int agx_profile_enable(agx_detector *det, int on); /* 0 off, 1 = the blur kernel only (2 events per batch), 2 = every kernel */
int agx_profile_reset(agx_detector *det);
int agx_profile_read(agx_detector *det, const char **names, double *ms_total, uint64_t *launches);

/* Copy an intermediate product of frame `frame` of the last batch to host memory.
 * what: AGX_DBG_BLUR / AGX_DBG_RESP (width*height floats; AGX_DBG_RESP is the Hessian response
 * the blur kernel evaluated in its registers and needs option "store_response" = 1 set before
 * the batch was enqueued -- the chain itself never stores it), AGX_DBG_MIN (1 float),
 * AGX_DBG_CENTERS (n clusters * {u32 first_index, u32 size, f32 cx, f32 cy} sorted by
 * first_index), AGX_DBG_REFINED (unfiltered rochade_refine output, agx_saddle each, in
 * cluster order).  *n_items receives the element count; returns AGX_ERR_CAPACITY if
 * cap_bytes is too small. */
enum { AGX_DBG_BLUR = 0, AGX_DBG_RESP = 1, AGX_DBG_MIN = 2, AGX_DBG_CENTERS = 3, AGX_DBG_REFINED = 4,
       AGX_DBG_COUNTERS = 5, /* 8 x uint32: status flags (AGX_FRAME_*), flood seeds, second-tier seeds,
                                clusters, generic-path candidates, generic-path roots, refined, saddles */
       AGX_DBG_RESP_RECOMPUTED = 6, /* width*height floats: the response recomputed from the stored blur
                                       plane by a separate kernel (cross-check of AGX_DBG_RESP) */
       AGX_DBG_VERIFY_STATS = 7,    /* 20 x uint32: re-test statistics of K2 (debug_ablation bits 128 / 2048), phase times of
                                       K2 (8192) / of the flood + refine kernel (16384) in 10 ns ticks */
       AGX_DBG_LUMA8 = 9,   /* width*height bytes: to_luma8 as the device computed it for the last agx_detect on an
                               L16 / RGB8 image (agx_detect converts on the device; agx_luma8 is the host's) */
       AGX_DBG_WAVE_TIMES = 10, /* pairs of uint64 (start, end; 10 ns ticks of s_memrealtime) of every wave of one sparse
                                   kernel of the last batch; `frame` selects the kernel (1 verify, 2 flood + refine, 3 rare);
                                   needs debug_ablation & 4096 (tools/wave_timeline.py) */
       AGX_DBG_REDZONES = 8, /* 6 x uint32: guarded buffers, damaged guard bytes, first damaged buffer, its byte
                               offset from the payload start (int32), device address of buffer 0 (lo, hi: for the
                               check of the check).  Buffers = the chain's workspace, then the staging buffer, the luma
                               planes and the device tail's code list, tag rows and frame table (mapped pinned host memory), then
                               agx_detect_batch_enqueue_to's device-memory tag rows and frame table, agx_detect_batch_fetch's
                               pinned luma planes, the front-end kernel's luma plane (AGX_LA8 .. AGX_RGBA16), the stored / recomputed response planes, agx_refine_points_enqueue's internal records and statuses and agx_rochade_refine's points, agx_decode_quads_enqueue's internal tags, statuses and bits and agx_decode_quads' quads, and agx_find_boards_enqueue's internal quads, quad points, counts and statuses and agx_find_board's list, and agx_planes_enqueue's workspace blur planes and the device plane of agx_gaussian_blur_f32 / agx_hessian_response, and agx_clusters_enqueue's internal rows, points, counts and statuses and agx_cluster_centers' plane, as far as they exist.  Needs no enqueued batch.  Guard bytes exist only in handles created with
                               AGX_REDZONE_BYTES=<n> in the environment (memory-safety tests of the kernels) */
       AGX_DBG_TAIL_TABLE_ADDR = 11 /* 2 x uint64: host address and payload bytes of the device tail's frame table (the check
                                       of the check for a buffer in mapped host memory).  Needs no enqueued batch */ };
/* (agx_cluster_info, the element of AGX_DBG_CENTERS: declared with agx_clusters_enqueue above) */
/* Test hook of the host tail: for n pairs of vectors (v0x, v0y, v1x, v1y) the reference's
 * angle(v0, v1) in degrees (math_util.rs:27-33) and the bounded approximation the board search uses
 * to decide threshold comparisons that are not close (csrc/host_tail.cpp, LazyAngle); has_approx[i] = 0
 * where the approximation is not used (zero / non-finite operands).  The CPU suite checks the bound. */
int agx_debug_angle_pairs(const float *vectors, size_t n, float *exact, float *approx, uint8_t *has_approx);
/* The coarser first-level approximation in front of it (a three-term polynomial in float, max error 0.04 degrees, guard band
 * 0.1): most of the search's ~16 000 angle comparisons per frame are decided from it.  Same hook, same check. */
int agx_debug_angle_pairs_coarse(const float *vectors, size_t n, float *coarse, uint8_t *has_coarse);
/* Test hook of the device tail (option "device_tail"): the kernel evaluates angle_degree's atan2f by glibc's own
 * single-precision routine, restated (csrc/libm_f32.h).  *mismatches = on how many of n pseudo-random operand pairs (any two
 * floats, cross / dot products of image-sized vectors, ratios at the ends of the routine's reduction intervals, plus the
 * special cases) this process's atan2f disagrees with the restatement; the option is refused unless that is 0. */
int agx_debug_libm_atan2f_check(uint64_t n, uint64_t seed, uint64_t *mismatches);
/* The one test of is_valid_quad the device tail cannot restate bit for bit is "filter white block" (saddle.rs:26-38: cosf, sinf):
 * for n triples (s0.theta, v02.x, v02.y) the angle as the reference evaluates it (binary32, this process's libm) and as the
 * kernel's decisive evaluation does (binary64).  The kernel decides 60 <= angle <= 120 from the latter only when it is farther
 * than 1e-4 degrees from both thresholds; the CPU suite checks that the two never differ by more than half of that. */
int agx_debug_white_block_angles(const float *triples, size_t n, float *reference, double *binary64);
int agx_debug_fetch(agx_detector *det, int frame, int what, void *host_out, size_t cap_bytes,
                    size_t *n_items);

/* Constants computed at create time (for parity tests): 7 blur weights, 25 cone taps,
 * 25x6 pseudo-inverse (row i, column j at [i*6+j]). */
int agx_detector_constants(const agx_detector *det, float *blur_w7, float *cone25, float *pmat150);
/* The taps of gaussian_blur_f32 at `sigma` (src/image_util.rs:110-206, the kernel at :111-124): *radius = ceilf(2 sigma) and the
 * 2*radius + 1 weights; no handle, no device.  AGX_ERR_CAPACITY: cap is smaller than that (*radius is set); AGX_ERR_ARG: sigma is
 * not positive and finite, or ceilf(2 sigma) > 16. */
int agx_debug_blur_weights(float sigma, float *weights, int cap, int *radius);
/* The constants of rochade_refine at half_size_patch (src/detector.rs:194-361; the pseudo-inverse at :208-237, the cone kernel at
 * :240-254): *n_points = (2*half_size_patch + 1)^2, cone receives n_points floats and pmat n_points*6, row i, column j at
 * [i*6+j]; no handle, no device.  The pseudo-inverse is the exact one of the quadratic design matrix rounded to binary32, with no
 * negative zeros; at 2 both are agx_detector_constants'.  AGX_ERR_CAPACITY: cap_points is smaller than that (*n_points is set);
 * AGX_ERR_ARG: half_size_patch outside 1 .. 4, or a NULL output. */
int agx_debug_refine_constants(int half_size_patch, float *cone, float *pmat, int cap_points, int *n_points);

const char *agx_status_string(int status);
/* Message of the last failure on this detector (HIP error text etc.); never NULL.
 * det == NULL: the reason of the last failed agx_detector_create. */
const char *agx_last_error(const agx_detector *det);
int agx_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* APRILGRID_AMD_H */
