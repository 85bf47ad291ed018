// chain_kernels.h -- host-visible interface of the HIP saddle chain (chain_kernels.hip).
// Internal to the library; the public boundary is include/aprilgrid_amd.h.
#pragma once
#include <cstddef>
#include <cstdint>

namespace agx {

enum Kernel : int {
    K_BLUR_HESSIAN = 0,  // K1: luma -> 7-tap blur (stored) -> Hessian determinant -> per-frame min
    K_THRESHOLD = 1,     // K2: verify K1's candidate superset mask against the final threshold
                         //     (exact response recomputed from the blur plane at set bits only),
                         //     then mask scan -> flood seeds
    K_FLOOD_REFINE = 2,  // K3: bit-parallel flood fill per seed (32x32 window per lane) -> cluster record ->
                         //     rochade_refine of the cluster, by the same lane
    K_RARE = 3,          // K4: per frame: second flood tier (128x64 per wave), generic clustering fallback for frames
                         //     with larger components, k/phi filter and reference-order emission; clears the
                         //     next batch's counters
    K_SPARSE = 4,        // K2 + K3 + K4 of one frame in one 1024-thread workgroup (k_sparse_frame): batches that fill the chip
                         //     with one workgroup per frame run K1 + K_SPARSE, the others K1 .. K4
    K_COUNT = 5
};

// One record of K4's output list.
struct RefinedRec {
    uint32_t key;  // smallest linear pixel index of the cluster == reference emission rank
    float x, y, k, theta, phi;
};

// Per-frame counters, zeroed (hipMemsetAsync) before every batch.
struct FrameCounters {
    // its own 128-byte line: every wave of K1 publishes to / polls this word
    uint32_t min_key_inv;  // ~order_preserving(min response); atomicMax
    uint32_t pad0[31];
    uint32_t n_seeds;      // flood seeds
    uint32_t n_clusters;   // cluster records of the first flood tier (k_flood_refine) or of the generic path
    uint32_t n_refined;    // rochade_refine survivors
    uint32_t max_k_bits;   // max k (k >= 0 so the raw bits order correctly)
    uint32_t flags;        // FLAG_* below
    uint32_t n_out;        // saddles after the filter
    uint32_t out_offset;   // start of this frame's saddles in the compact output array
    uint32_t n_cand;       // generic path: candidate pixels
    uint32_t n_roots;      // generic path: union-find roots
    uint32_t n_big;        // seeds handed to the wave-wide second flood tier
    uint32_t refine_done;  // emit_large_split (k_rare with several workgroups per frame): lock + state of the frame's place in the
                           // compact output -- 0 free, 1 taken by the part that arrived first (CAS), 2 allocated and it fits,
                           // 3 allocated but over capacity; the frame's other parts spin on it until it is >= 2.  Must be 0 at
                           // batch start (the counters' clearing provides that).  Not touched on any other path.
    uint32_t n_clusters2;  // (unused since the second flood tier runs inside k_flood_refine; always 0)
    uint32_t stats[20];    // debug_ablation & 128: verify statistics by word row within a 128-row segment
};
static_assert(sizeof(FrameCounters) == 256, "FrameCounters is cleared as 64 dwords");
enum : uint32_t {
    FLAG_CAND_OVERFLOW = 1u,   // seed list (fast path) or candidate list (generic path) full
    FLAG_ROOT_OVERFLOW = 2u,   // cluster list full
    FLAG_OUT_OVERFLOW = 4u,
    FLAG_CENTROID_INEXACT = 8u,  // a cluster's coordinate sum reached 2^24 (f32 sums of the
                                 // reference would round there)
    FLAG_BIG_CLUSTER = 16u,      // a component left the flood windows: frame redone generically
    FLAG_RING_BELOW = 32u,       // k_plane_front (agx_clusters_enqueue): a pixel of the outermost ring is below the threshold
    FLAG_LARGE_RESULT = 64u      // more than 1024 refined records: emitted by k_rare's large-list sort
};

struct RefineConsts {
    float cone[25];    // normalised 5x5 cone kernel, detector.rs:240-254
    float pmat[150];   // 25x6 pseudo-inverse, [i*6+j], detector.rs:208-237
};

// Device workspace + geometry of one batch.  All pointers are device pointers.
struct ChainArgs {
    // input
    const uint8_t *frames;
    long long frame_stride;  // bytes
    int row_stride;          // bytes
    int byte_rows;           // rows / frames are not 4-byte aligned: the blur kernel gathers bytes
    int fmt;                 // agx_format
    int W, H, n_frames;
    long long plane;  // W*H
    // K1 tiling (host-chosen, see plan_k1)
    int threads;        // workgroup size (multiple of 64)
    int n_strips;       // column strips per row
    int strip_cols;     // columns per strip (multiple of 4)
    int rows_per_seg;   // output rows per workgroup
    int n_segs;
    int k1_group;       // frames per dispatch group of K1 (0 or >= n_frames: the whole batch segment-major)
    int k1_async_poll;  // K1 polls the frame's running minimum by asynchronous vector loads (few waves) / awaited scalar loads
    float publish_factor;  // a wave publishes its running minimum m only if m < factor * the frame's known minimum
    float w[7];  // blur taps
    // dense planes [n_frames][H][W]
    float *blur;
    float *resp_dbg;       // parity tests only ("store_response"): K1's in-register response, [n_frames][H][W]; else null
    float *dummy;          // one row (W + 8 floats): target of K1's out-of-segment stores
    // weakest (largest) response among the candidates K1 admitted, per 4 columns x 32 rows:
    // [n_frames][mask_yb][mask_wpr / 4] (same indexing as the mask, x/4); -inf where none
    float *cand_max;
    uint32_t *slot_plane;  // generic path only (sparse-touched)
    // Candidate bit mask, TRANSPOSED: one word = 32 consecutive rows of one column.
    // mask[frame][yb][MASK_PAD_X + x] holds rows 32*yb .. 32*yb+31 of column x (bit = row & 31).
    // MASK_PAD_X zero words on both sides of a word row and the word rows past the image are
    // never written and stay zero from allocation (flood windows reach into them).
    uint32_t *mask;
    int mask_wpr;            // words per word-row: round_up4(W + 2*MASK_PAD_X)
    int mask_yb;             // word rows: H/32 + 4
    long long mask_plane;    // words per frame = mask_wpr * mask_yb
    int force_generic;       // test hook: treat every frame as FLAG_BIG_CLUSTER
    int sparse_after_verify; // k_sparse_frame runs behind k_verify_seeds (sparse path 3): it skips its own verify stage
    // debug_ablation & 4096: every wave of the sparse kernels records when it started and ended (100 MHz
    // constant clock, s_memrealtime) -- record (kernel - 1) * WAVE_TIMES_STRIDE + blockIdx.x of this array
    // (two 64-bit words each; the generic path's slot plane serves as storage).  Else null.
    unsigned long long *wave_times;
    int dbg;                 // timing ablations only (results invalid): 1 = K1 skips blur stores,
                             // 4 = K1 skips the Hessian/min, 8 = K1 stores into an L2-resident
                             // region, 16 = no shared-min refresh
    // per-frame
    FrameCounters *ctr;
    FrameCounters *ctr_next;  // the other counter set: k_rare clears records [0, n_frames] of it for the next batch (or null)
    uint32_t *total_out;  // single counter: compact output allocation
    uint32_t cap_cand, cap_roots, cap_out;
    uint32_t *seeds;      // [n_frames][cap_roots] pixel index of each flood seed
    // cluster records [n_frames][cap_roots]
    uint32_t *clu_key;    // smallest pixel index of the cluster
    uint32_t *clu_cnt;
    // integer coordinate sums, on the generic path their low words (K4 leaves the f32 centroid bits here)
    uint32_t *clu_sx, *clu_sy;
    // generic path: candidate arrays [n_frames][cap_cand]
    uint32_t *cand;    // pixel index | left<<30 | up<<31
    uint32_t *parent;
    unsigned long long *sumx, *sumy;
    uint32_t *cnt, *minidx;
    uint32_t *roots;      // [n_frames][cap_roots]
    RefinedRec *refined;  // [n_frames][cap_roots]
    // output
    float *out;  // compact agx_saddle array (internal: n_frames*cap_out records, or caller-owned)
    uint32_t out_total_cap;  // records `out` can hold
    uint32_t *frame_table;   // optional caller-owned [n_frames][4]: count, offset, status, clusters
    float min_angle, max_angle;
};

// Tuning overrides from the environment (AGX_K1_*, AGX_G_*, AGX_RARE_PARTS, AGX_SPARSE_PATH: measurement only).  A name is read
// from the environment once per process and kept; tuning_env_reload() forgets what was read (option "reload_tuning_env").
int tuning_env(const char *name, int dflt);
void tuning_env_reload();

// Choose K1's tiling for a frame size / batch size.  Returns false if unsupported.
bool plan_k1(ChainArgs &a, int override_rows_per_seg);

// Enqueue one kernel of the chain on `stream` (hipStream_t as void*).  Returns hipError_t.
// deferred_refine (agx_detector_set_half_size_patch: the chain's refinement as launches of its own, see launch_refine_clusters):
// K_FLOOD_REFINE then launches the instantiation that clusters without refining, K_RARE the one that only emits.  ChainArgs
// carries nothing of this, so that the kernels of the default plan keep their argument layout.
int launch_kernel(int which, const ChainArgs &a, const RefineConsts &rc, void *stream, bool deferred_refine = false);

// k_refine_points (agx_refine_points_enqueue): rochade_refine (detector.rs:194-361, half_size_patch = 2) of caller-given points
// on the f32 plane(s) `img` -- the chain's blur planes, or a caller's own.  All pointers are device pointers.
struct RefinePointsArgs {
    const float *img;        // frame f's plane at img + f * frame_stride
    long long frame_stride;  // floats
    long long pitch;         // floats between rows (>= W)
    int W, H;
    int padded;              // at least 3 readable floats behind the last plane (the aligned 16-byte window loads may be used)
    const float *points;     // [n_frames][points_per_frame] (x, y)
    uint32_t points_per_frame;
    const uint32_t *counts;  // [n_frames] points of frame f (capped at points_per_frame), or null: points_per_frame each
    float *out;              // [n_frames][points_per_frame][5]: x, y, k, theta, phi; five zeros for a rejected point
    uint32_t *status;        // [n_frames][points_per_frame]: AGX_POINT_*
};
// grid (ceil(points_per_frame / 64), n_frames <= 65535), one point per lane; hipError_t
int launch_refine_points(const RefinePointsArgs &p, const RefineConsts &rc, int n_frames, void *stream);

// k_refine_patch<HALF> (agx_refine_points_enqueue_h): the same rochade_refine at half_size_patch = HALF in 1 .. 4, sixteen lanes
// to a point.  The constants of one half size, as they lie in the handle's device table: record `half - 1` of
// REFINE_PATCH_MAX_HALF such records.
constexpr int REFINE_PATCH_MAX_HALF = 4;
constexpr int REFINE_PATCH_MAX_TAPS = (2 * REFINE_PATCH_MAX_HALF + 1) * (2 * REFINE_PATCH_MAX_HALF + 1);  // 81
struct RefinePatchConsts {
    float cone[REFINE_PATCH_MAX_TAPS];      // normalised ks x ks cone kernel, the first ks*ks entries (detector.rs:240-254)
    float pmat[REFINE_PATCH_MAX_TAPS * 6];  // ks*ks x 6 pseudo-inverse, [i*6+j] (detector.rs:208-237)
};
// grid (ceil(points_per_frame / 4), n_frames <= 65535); `consts` is the device record of `half`; a plane is never read outside
// a point's own (4*half+1)^2 window, whatever p.padded says.  hipError_t
int launch_refine_patch(const RefinePointsArgs &p, const RefinePatchConsts *consts, int half, int n_frames, void *stream);

// k_refine_windows<HALF> (agx_refine_windows_enqueue): the same rochade_refine on the frames' blur at the taps `w`, with the blur
// window of every point computed from the input in LDS: no plane is read or written.  All pointers are device pointers.
struct RefineWindowsArgs {
    const uint8_t *frames;   // frames of format `fmt`: 0 AGX_L8, 1 AGX_L16, 3 AGX_LF32
    long long frame_stride;  // bytes
    int row_stride;          // bytes
    int fmt;
    int W, H;
    const void *points;      // slot s: two floats (x, y) at points + s * point_stride, s = f * points_per_frame + i
    size_t point_stride;     // bytes, a multiple of 4, >= 8
    uint32_t points_per_frame;
    const uint32_t *counts;     // as RefinePointsArgs
    const uint32_t *status_in;  // [n_frames][points_per_frame], or null: a slot whose word is non-zero is handed on, not refined
    float *out;                 // as RefinePointsArgs
    uint32_t *status;
    int factor;           // 1: the point as it is; else x * scale + offset, two rounded operations
    float scale, offset;  // (float)factor, 0.5f * (factor - 1)
    int radius;           // 1 .. GB_MAX_RADIUS
    float w[2 * 16 + 1];  // the blur taps (GaussBlurArgs::w)
    int points_per_group;  // set by the launch: points of a workgroup, and the floats of LDS between two of them
    uint32_t lds_stride;
};
// the points a workgroup takes at this half size and radius: whole waves (multiples of 4), at most 16, within 64 KB of LDS
int refine_windows_points_per_group(int half, int radius);
// grid (ceil(points_per_frame / points per group), n_frames <= 65535); `consts` is the device record of `half`.  hipError_t
int launch_refine_windows(const RefineWindowsArgs &p, const RefinePatchConsts *consts, int half, int n_frames, void *stream);

// The chain's deferred refinement, between launch_kernel(K_FLOOD_REFINE, .., true) and launch_kernel(K_RARE, .., true):
// k_generic_cluster (a.n_frames workgroups; generic_frame for the frames that need it) and k_refine_clusters<half>, rochade_refine
// at half_size_patch `half` in 1 .. 4 of every frame's cluster table on its blur plane (a fixed number of one-wave workgroups per
// frame that loop over the table).  `consts`: the handle's device table of REFINE_PATCH_MAX_HALF records.  hipError_t
int launch_generic_cluster(const ChainArgs &a, void *stream);
int launch_refine_clusters(const ChainArgs &a, const RefinePatchConsts *consts, int half, void *stream);

size_t k5_lds_bytes(const ChainArgs &a);

constexpr size_t WAVE_TIMES_STRIDE = (size_t)1 << 20;  // records per kernel (debug_ablation & 4096)

constexpr int MASK_PAD_X = 64;  // zero columns on each side of the transposed mask (flood windows)  // flood window rows below the last image row

// Debug: recompute the Hessian response plane of `frame` from its blur plane into dst.
// Per-device kernel attributes (current device); hipError_t.
int init_device_kernels();

int launch_debug_resp(const ChainArgs &a, int frame, float *dst, void *stream);
// The batch's frame rows ([n_frames + 1][4]: count, offset, flags, clusters; the last row: total) and compact saddle array into
// mapped pinned host memory (device addresses h_table_dev / h_out_dev) by a kernel on `stream`.
int launch_publish(const ChainArgs &a, uint32_t h_out_records, uint32_t *h_table_dev, float *h_out_dev, void *stream);
// Zero n_records counter records on `stream` (used instead of a memset while the stream is being captured).
int launch_clear_counters(FrameCounters *ctr, size_t n_records, void *stream);
// k_front_luma: the integer luma plane of n_frames frames of one of the layouts AGX_LA8 .. AGX_RGBA16 (format 4 .. 11) in device
// memory -> tight [n_frames][H][W] u8 (8-bit layouts; 16-bit layouts with out8 != 0: to_luma8) or u16 (16-bit layouts, out8 == 0).
// Rows `row_stride` bytes apart, frames `frame_stride`; the planes of AGX_RGB8P are H * row_stride bytes apart.
int launch_front_luma(const void *src, size_t row_stride, size_t frame_stride, int n_frames, int format, void *dst, int out8, int W,
                      int H, void *stream);
// u8 luma (to_luma8) of n_frames L16 (format 1) / RGB8 (format 2) frames in device memory, or of a layout of
// launch_front_luma (by that kernel): rows `pitch` bytes apart, frames `frame_stride` bytes apart -> tight [n_frames][H][W]
int launch_luma8(const void *src, size_t pitch, size_t frame_stride, int n_frames, int format, uint8_t *dst, int W, int H,
                 void *stream);


// k_gauss_blur (agx_planes_enqueue): gaussian_blur_f32 (image_util.rs:110-206) of to_luma32f of n_frames frames, radius
// 1 .. GB_MAX_RADIUS.  All pointers are device pointers.
constexpr int GB_MAX_RADIUS = 16;
constexpr int GB_TX = 64, GB_TY = 64;  // output tile of a workgroup
constexpr int GB_HPITCH = GB_TX + 1;   // LDS pitch of the horizontal pass's result
struct GaussBlurArgs {
    const uint8_t *src;  // frames of format 0 .. 3 (AGX_L8, AGX_L16, AGX_RGB8, AGX_LF32)
    long long src_frame_stride;  // bytes
    int src_row_stride;          // bytes
    int W, H;
    float *dst;                  // frame f, row y at dst + f * dst_frame_stride + y * dst_row_stride; W floats per row are written
    long long dst_frame_stride;  // floats
    long long dst_row_stride;    // floats
    int radius;
    float w[2 * GB_MAX_RADIUS + 1];  // the taps (uniform: the kernel reads them by scalar loads)
};
size_t gauss_blur_lds_bytes(int radius);
// grid (ceil(W / GB_TX), min(ceil(H / GB_TY), 65535), n_frames <= 65535); hipError_t
int launch_gauss_blur(const GaussBlurArgs &a, int format, int n_frames, void *stream);

// k_hessian_response (agx_planes_enqueue): hessian_response (image_util.rs:72-109) of to_luma32f of n_frames frames of format
// 0 .. 3 (3: an f32 plane as it is, such as k_gauss_blur's).  Strides as GaussBlurArgs.
struct HessianArgs {
    const uint8_t *src;
    long long src_frame_stride;
    int src_row_stride;
    int W, H;
    float *dst;
    long long dst_frame_stride, dst_row_stride;
};
int launch_hessian_response(const HessianArgs &a, int format, int n_frames, void *stream);

// k_response_front: the chain's front behind k_gauss_blur for a blur sigma other than 1.5.  From the workspace blur plane a.blur
// it fills what K1 otherwise hands to the sparse stages: a.ctr[frame].min_key_inv (final when the first of its two launches is
// through), every mask word of the image area (exact: resp < 0.05 * min), every cand_max block of those words and, if non-null,
// a.resp_dbg.  Reads of `a`: blur, resp_dbg, ctr, mask, cand_max and their geometry; nothing of K1's tiling.
// grid (ceil(W / 64), min(ceil(H / 128), 65535), n_frames <= 65535); hipError_t
int launch_response_front(const ChainArgs &a, void *stream);

// k_plane_front (agx_clusters_enqueue): the front for a caller's response plane -- the products of k_response_front, taken from
// the plane as it is instead of from a blur plane: a.ctr[frame].min_key_inv = the fold `e < acc ? e : acc` from f32::MAX over all
// W*H values (detector.rs:414-417; final when the first of its two launches is through), every mask word of the image area
// (exact: v < 0.05 * min, interior pixels only: no ring bits) and every cand_max block of those words.  A ring pixel below the
// threshold raises FLAG_RING_BELOW of the frame (frames with an interior).  Reads of `a`: ctr, mask, cand_max and their geometry,
// W, H, n_frames.  Only the W floats of a row are read, each once per launch.
struct PlaneFrontArgs {
    const float *src;        // frame f, row y at src + f * frame_stride + y * row_stride
    long long frame_stride;  // floats
    long long row_stride;    // floats
};
// grid (ceil(W / 64), min(ceil(H / 128), 65535), n_frames <= 65535); hipError_t
int launch_plane_front(const ChainArgs &a, const PlaneFrontArgs &p, void *stream);

// k_emit_clusters (agx_clusters_enqueue): the cluster table the cluster-only sparse stages leave per frame (clu_key, clu_cnt and
// the f32 centroid bits in clu_sx / clu_sy, ctr.n_clusters, ctr.flags) -> the caller's rows in the order of clu_key, one
// 1024-thread workgroup per frame.  Status values are AGX_CLUSTERS_* of include/aprilgrid_amd.h.
constexpr uint32_t EMIT_CLUSTERS_MAX = 16384;  // rows per frame: the keys are ordered in 64 KB of LDS
struct EmitClustersArgs {
    uint32_t per_frame;  // clusters_per_frame, 1 .. EMIT_CLUSTERS_MAX
    uint32_t *rows;      // [n_frames][per_frame][4]: first_index, size, cx, cy (agx_cluster_info)
    float *points;       // [n_frames][per_frame][2]: cx, cy (agx_point), or null
    uint32_t *counts;    // [n_frames]
    uint32_t *status;    // [n_frames]
};
int launch_emit_clusters(const ChainArgs &a, const EmitClustersArgs &e, void *stream);

// k_filter_saddles (agx_filter_saddles_enqueue): the k / phi filter (detector.rs:432-445) of every frame's refined slots, one
// wave per frame: status words that are 0 (AGX_POINT_REFINED) become `filtered` where the record fails.
struct FilterSaddlesArgs {
    const float *records;  // [n_frames][per_frame][5]: x, y, k, theta, phi
    uint32_t *status;      // [n_frames][per_frame]
    const uint32_t *counts;  // [n_frames] (capped at per_frame), or null: per_frame each
    uint32_t per_frame;
    float min_angle, max_angle;
    uint32_t filtered;     // AGX_POINT_FILTERED
};
int launch_filter_saddles(const FilterSaddlesArgs &f, int n_frames, void *stream);

}  // namespace agx
