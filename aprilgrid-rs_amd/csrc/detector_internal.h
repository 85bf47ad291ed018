// detector_internal.h -- the detector handle as the library's own files see it (detector.cpp, detect_batch.cpp, group.cpp);
// not part of the ABI.
#pragma once
#include <hip/hip_runtime_api.h>

#include <string>
#include <vector>

#include "../../include/aprilgrid_amd.h"
#include "chain_kernels.h"
#include "host_tail.hpp"

#define AGX_UPLOAD_STREAMS 3
// a HIP call that must succeed: else AGX_ERR_HIP with the call and HIP's reason in agx_last_error
#define HIP_TRY(det, expr)                                                                          \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return agx::fail((det), AGX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

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

class WorkerPool;  // detect_batch.cpp
WorkerPool *create_worker_pool(int n_threads);
void destroy_worker_pool(WorkerPool *pool);
TailWorkers *create_tail_workers(int n_threads);  // nullptr for n_threads <= 1
void destroy_tail_workers(TailWorkers *w);

// The batch in flight on a handle: one at a time, the last one enqueued.  agx_detector::batch says whose it is and so which fetch
// resolves it; the payload of that kind (below) is valid while it does.  begin_batch() is the only place that forgets a batch;
// every enqueue calls it behind its argument checks, so a refused enqueue leaves the batch in flight where it was.  Forgetting
// a batch does not wait for it or undo it: a refine batch whose results go to the caller's device arrays may be followed by a
// decode batch that reads those arrays without a fetch in between -- same stream, in order.  ("The batch in flight")
enum BatchKind {
    BATCH_NONE,     // nothing to fetch (also behind agx_planes_enqueue, which has no fetch)
    BATCH_SADDLES,  // the chain's results: stays fetchable after a fetch (refetch_single, agx_detect's retry, agx_debug_fetch)
    BATCH_DETECT,   // the chain's results + DetectPending; agx::fetch_compact reads the chain's part while the fetch resolves it
    BATCH_REFINE,   // RefinePending; nothing of the chain is there to be fetched, even where K1 ran for the blur planes
    BATCH_DECODE,   // DecodePending
    BATCH_FIND,     // FindPending
    BATCH_CLUSTERS, // ClustersPending; the chain's kernels ran on the workspace, but nothing of the chain is there to be fetched
    BATCH_GROW,     // GrowPending
    BATCH_INIT,     // InitPending
    BATCH_KINDS
};
// where a kind's results are: the fetch copies them out of the handle's side buffers / they are in the caller's device arrays
// already / (BATCH_DETECT only) they are a group's, and only agx_group_detect_fetch resolves the batch
enum { RESULTS_HOST = 1, RESULTS_CALLER = 2, RESULTS_GROUP = 3 };

struct DetectPending {
    int results = 0;           // RESULTS_*
    bool device_tail = false;  // the device tail runs behind the chain; else the fetch runs the host tail on every frame
    int n_frames = 0, width = 0, height = 0;
    uint32_t cap = 0;
    const uint8_t *d_luma = nullptr;  // the batch's u8 luma on the device: the L8 frames themselves or the k_luma8 planes
    size_t luma_row = 0, luma_frame = 0;
    agx_tag *d_tags = nullptr;  // RESULTS_CALLER: [n_frames][cap]; RESULTS_GROUP: the group's tag slab of this rank
    uint32_t *d_counts = nullptr;  // RESULTS_GROUP: the group's packed frame table [n_frames][4]
    int *d_status = nullptr;
};

struct RefinePending {
    int results = 0;  // RESULTS_HOST: in SB_REFINE_OUT / SB_REFINE_STATUS, or RESULTS_CALLER
    int n_frames = 0;
    uint32_t points_per_frame = 0;
    const uint32_t *d_counts = nullptr;  // the caller's per-frame counts (RESULTS_HOST: the fetch copies only the slots that were written)
};

struct DecodePending {
    int results = 0;  // RESULTS_HOST: in SB_DECODE_TAGS / _STATUS / _BITS, or RESULTS_CALLER
    int n_frames = 0;
    uint32_t quads_per_frame = 0;
    const uint32_t *d_counts = nullptr;  // the caller's per-frame counts (RESULTS_HOST: the fetch copies only the slots that were written)
};

// The three stages over caller-given saddle lists (agx_find_boards_*, agx_grow_boards_*, agx_init_quads_*), as the handle's
// per-stage records are indexed
enum { LIST_FIND, LIST_GROW, LIST_INIT, LIST_STAGES };

// The fetch reads the inputs again for the frames the kernel handed back (AGX_BOARD_PENDING).
struct FindPending {
    int results = 0;  // RESULTS_HOST: in SB_FIND_QUADS / _COUNTS / _STATUS, or RESULTS_CALLER
    int n_frames = 0;
    uint32_t saddles_per_frame = 0, quads_per_frame = 0;
    size_t stride = 0;
    const uint8_t *d_saddles = nullptr;
    const uint32_t *d_counts = nullptr, *d_frame_table = nullptr, *d_point_status = nullptr;
    uint32_t *d_quads = nullptr, *d_n_quads = nullptr, *d_status = nullptr;
    float *d_quad_points = nullptr;  // the caller's, SB_FIND_POINTS (RESULTS_HOST without the caller's), or null
    // the stages with seeds (GrowPending, InitPending): frame f has min(d_seed_counts[f], seeds_per_frame) of them, or seeds_per_frame
    const uint32_t *d_seed_counts = nullptr;
    uint32_t seeds_per_frame = 0;
};

// FindPending's list and result arrays (always RESULTS_CALLER) and what the host form needs besides
struct GrowPending : FindPending {
    const uint32_t *d_seed_quads = nullptr;
    uint32_t stop_score = 0;
    float spacing_ratio = 0.3f;
    int flags = 0;
    uint32_t *d_seed_scores = nullptr, *d_best_seed = nullptr;
};

// FindPending's list and result arrays (always RESULTS_CALLER) and the seeds
struct InitPending : FindPending {
    const uint32_t *d_seed_saddles = nullptr;
    uint32_t n_nearest = 50;
    uint32_t *d_seed_quad_counts = nullptr, *d_seeds_out = nullptr, *d_n_seeds_out = nullptr;
};

struct ClustersPending {
    int results = 0;  // RESULTS_HOST: in SB_CLUSTERS_ROWS / _POINTS / _COUNTS / _STATUS, or RESULTS_CALLER
    int n_frames = 0;
    uint32_t clusters_per_frame = 0;
    const agx_point *d_points = nullptr;  // RESULTS_HOST: where the batch wrote the points -- the caller's d_points, else SB_CLUSTERS_POINTS
};

// A batch of equally sized frames in device memory as an entry point was handed it, and what differs between the entry points'
// checks of one (check_frame_batch)
struct FrameBatch {
    const void *frames = nullptr;
    int n_frames = 0, width = 0, height = 0;
    size_t row_stride = 0, frame_stride = 0;  // bytes
    int format = -1;
};
struct BatchRules {
    int min_side;            // smallest width / height: 2 where the chain runs, 1 elsewhere
    bool lf32;               // AGX_LF32 is accepted (refused where the entry point needs to_luma8)
    bool lone_frame_stride;  // the frame stride of a single frame takes part in the alignment tests (else only from 2 frames on)
    bool align16;            // the 16-bit layouts' 2-byte alignment is checked (agx_refine_points_enqueue leaves it to the chain)
    bool front_rows;         // the front-end layouts' row limit is checked (agx_refine_points_enqueue leaves it to the chain)
};

struct EventPair {
    hipEvent_t a, b;
    int kernel;  // K_* (agx_profile_read's totals), or K_COUNT + XT_* (the time of the last one)
};
// Launches outside agx_profile_read's table that profiling level 2 times all the same: the device time of the last one, read
// back as option "last_response_front_us" / "last_clusters_front_us" / "last_clusters_emit_us" (tools/bench_clusters.py)
enum { XT_RESPONSE_FRONT, XT_PLANE_FRONT, XT_EMIT_CLUSTERS, XT_COUNT };

// A buffer outside the chain's workspace, device memory or pinned host memory, with the handle's guard bytes in front and
// behind.  The slot is the only record of it: who needs the buffer asks the slot (side_ensure below grows it).
struct SideBuf {
    void *base = nullptr;     // start of the front guard (what hipMalloc / hipHostMalloc returned)
    void *payload = nullptr;  // base + guard
    void *mapped = nullptr;   // device address of the payload of a mapped host buffer
    size_t bytes = 0;         // payload
    bool host = false;        // pinned host memory
    template <class T> T *ptr() const { return static_cast<T *>(payload); }  // null while the slot is empty
    template <class T> T *dev() const { return static_cast<T *>(mapped); }
};
enum {
    SB_STAGE,       // staging of host frames (agx_detect, agx_detect_batch)
    SB_LUMA_D,      // u8 luma of L16 / colour frames, computed on the device ...
    SB_LUMA_H,      // ... and its pinned host copy
    SB_CODES,       // the device tail: the family's code list
    SB_TAGS,        // mapped pinned [tail_frames][tail_tag_cap] agx_tag
    SB_TAIL_TABLE,  // mapped pinned [tail_frames][4]: count, status, ticks, saddles | seeds << 16
    SB_DTAGS,       // agx_detect_batch_enqueue_to: the same pair in device memory, [dtail_frames][dtail_tag_cap] ...
    SB_DTABLE,      // ... and [dtail_frames][4]
    SB_FETCH_LUMA,  // agx_detect_batch_fetch: pinned luma planes of the frames the host tail takes
    SB_FRONT,       // k_front_luma's integer luma plane of a batch in one of the layouts AGX_LA8 .. AGX_RGBA16
    SB_RESP_STORE,  // option "store_response": the [n_frames][H][W] planes K1's parity-test instantiation writes
    SB_DBG_RESP,    // agx_debug_fetch(AGX_DBG_RESP_RECOMPUTED): one plane
    SB_REFINE_OUT,     // agx_refine_points_enqueue without caller-owned results: [n_frames][points_per_frame] agx_saddle ...
    SB_REFINE_STATUS,  // ... and [n_frames][points_per_frame] uint32 (AGX_POINT_*)
    SB_REFINE_POINTS,  // agx_rochade_refine: the host's points on the device
    SB_REFINE_CONSTS,  // k_refine_patch, k_refine_clusters: RefinePatchConsts of half_size_patch 1 .. 4, uploaded by the first batch that needs them
    SB_DECODE_TAGS,    // agx_decode_quads_enqueue without caller-owned results: [n_frames][quads_per_frame] agx_tag ...
    SB_DECODE_STATUS,  // ... [n_frames][quads_per_frame] uint32 (AGX_QUAD_*) ...
    SB_DECODE_BITS,    // ... and [n_frames][quads_per_frame] uint64 (bit_code's value)
    SB_DECODE_QUADS,   // agx_decode_quads: the host's quads on the device
    SB_FIND_QUADS,     // agx_find_boards_enqueue without caller-owned results: [n_frames][quads_per_frame][4] uint32 ...
    SB_FIND_POINTS,    // ... [n_frames][quads_per_frame][4][2] float (unless the caller gave d_quad_points) ...
    SB_FIND_COUNTS,    // ... [n_frames] uint32 ...
    SB_FIND_STATUS,    // ... and [n_frames] uint32 (AGX_BOARD_*)
    SB_FIND_SADDLES,   // agx_find_board: the host's list on the device
    SB_PLANES_BLUR,    // agx_planes_enqueue without d_blur: the tight [n_frames][H][W] blur planes the response is taken of
    SB_PLANES_OUT,     // agx_gaussian_blur_f32 / agx_hessian_response: the plane on the device before it is copied down
    SB_CLUSTERS_ROWS,    // agx_clusters_enqueue without caller-owned results: [n_frames][clusters_per_frame] agx_cluster_info ...
    SB_CLUSTERS_POINTS,  // ... [n_frames][clusters_per_frame] agx_point (unless the caller gave d_points) ...
    SB_CLUSTERS_COUNTS,  // ... [n_frames] uint32 ...
    SB_CLUSTERS_STATUS,  // ... and [n_frames] uint32 (AGX_CLUSTERS_*)
    SB_CLUSTERS_PLANE,   // agx_cluster_centers: the host's plane on the device
    SB_CALIB_WORK,       // agx_calibrate_enqueue: the state, the frames' blocks and poses between its launches (calibrate.h: CalibWork)
    SB_RIG_WORK,         // agx_rig_calibrate_enqueue: the state, the frames' sums and the instants' blocks between its launches (rig.h: RigWork)
    SB_COUNT
};
}  // namespace agx

struct agx_detector {
    int family = AGX_T36H11;
    agx::FamilyInfo fam{};
    agx_params params{};
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;  // what the kernels are enqueued on: own_stream, or the caller's after agx_detector_set_stream
    agx::RefineConsts rc{};
    float blur_w[7]{};
    // agx_detector_set_blur_sigma: the chain's blur sigma.  Bit-equal to 1.5f: the chain starts with K1 (blur_w above); else with
    // k_gauss_blur (front_radius, front_w: the taps of agx_debug_blur_weights(blur_sigma)) + k_response_front
    float blur_sigma = 1.5f;
    int front_radius = 3;
    float front_w[2 * agx::GB_MAX_RADIUS + 1]{};
    int last_chain_front = 0;  // option "last_chain_front": the last chain batch ran 0 = K1, 1 = the any-sigma front
    // agx_detector_set_half_size_patch: rochade_refine's half_size_patch behind every chain entry.  2 refines inside the flood
    // stages (k_flood_refine, k_sparse_frame, k_rare); every other size, and 2 under option "chain_refine_general", clusters
    // there and refines by k_refine_clusters (enqueue_chunk)
    int half_size_patch = 2;
    int chain_refine_general = 0;  // option "chain_refine_general": half_size_patch 2 takes the deferred refinement too
    int last_chain_refine = 0;     // option "last_chain_refine": the last chain batch refined 0 = inside the flood stages, 1 = by k_refine_clusters
    uint32_t lim_cand = 0, lim_roots = 0, lim_out = 0;
    int force_generic = 0;
    int k1_rows = 0;
    int sparse_path = 0;  // option "sparse_path": 0 = by batch size, 1 = K2 + K3 + K4 (three launches), 2 = k_sparse_frame (one)
    bool last_sparse_frame = false;  // the last batch ran K1 + K_SPARSE
    int last_sparse_path = 1;        // 1 three launches, 2 k_sparse_frame alone, 3 k_verify_seeds + k_sparse_frame
    int n_cus = 0;                   // compute units of the device (hipDeviceProp_t::multiProcessorCount)
    int dbg = 0;
    int store_resp = 0;           // option "store_response": K1's parity-test instantiation (writes SB_RESP_STORE)
    bool resp_stored = false;     // the last batch ran with store_response
    int ws_W = 0, ws_H = 0;       // geometry the mask plane was last zeroed for

    // workspace (device)
    agx::ChainArgs args{};
    size_t cap_frames = 0;        // frames the dense planes hold
    long long cap_plane = 0;      // pixels per frame the dense planes hold
    uint32_t alloc_cand = 0, alloc_roots = 0, alloc_out = 0;
    std::vector<void *> device_allocs;
    // AGX_REDZONE_BYTES (environment, read when the handle is created; tests only): every workspace
    // buffer gets this many guard bytes in front and behind, filled with 0xA5; agx_debug_fetch
    // (AGX_DBG_REDZONES) reports the guard bytes that no longer hold the pattern
    size_t redzone = 0;
    std::vector<size_t> alloc_bytes;  // payload bytes per entry of device_allocs
    // the buffers outside the workspace: the same guard bytes around each; AGX_DBG_REDZONES counts the ones that exist after the
    // workspace's, in this order
    agx::SideBuf side[agx::SB_COUNT];
    // SB_FRONT holds the plane the chain reads instead of the frames; front_src / front_format / front_frames name the batch it
    // holds, so that to_luma8 is derived from it instead of from the frames again (an 8-bit layout: it IS that plane).  They are
    // valid only from batch_enqueue_impl to the next enqueue on the handle, whose begin_batch resets them first (format -1: none):
    // whoever asks for the luma of a batch does so right behind that batch's enqueue, on the same stream
    const void *front_src = nullptr;
    int front_format = -1, front_frames = 0;
    // pinned host mirrors
    agx::FrameCounters *h_ctr = nullptr;
    size_t h_ctr_frames = 0;
    uint32_t *h_total = nullptr;
    float *h_out = nullptr;
    size_t h_out_records = 0;
    float *d_out_internal = nullptr;  // workspace copy of args.out
    float *h_out_dev = nullptr;       // device address of h_out (mapped pinned memory): a single frame's list is written there directly
    bool out_in_host = false;         // last batch's compact output went straight to h_out
    uint32_t *h_table = nullptr, *h_table_dev = nullptr;  // mapped pinned [frames + 1][4]: per frame count, offset, status, clusters (k_publish / the single frame's k_rare)
    size_t h_table_rows = 0;
    size_t mask_words = 0;
    bool external_out = false;       // last batch wrote into caller-owned device memory

    // two counter sets used alternately: the last kernel of a batch clears the other set, so only a
    // batch that finds its set not known to be clear pays a memset
    agx::FrameCounters *d_ctr[2] = {nullptr, nullptr};
    size_t ctr_cleared[2] = {0, 0};  // records of the set known to be zero (0 = in use / unknown)
    int ctr_cur = 0;

    int batch = agx::BATCH_NONE;  // agx::BatchKind: the batch in flight
    int profiling = 0;  // 0 off, 1 = K1 only, 2 = every kernel
    int prof_stride = 1;        // level 1: time the selected kernel of every prof_stride-th batch only
    int prof_kernel = agx::K_BLUR_HESSIAN;  // level 1: which kernel (option "profile_kernel", default the blur kernel)
    uint64_t prof_batches = 0;  // batches enqueued while profiling
    std::vector<agx::EventPair> pending_events;
    std::vector<hipEvent_t> free_events;
    double prof_ms[agx::K_COUNT]{};
    uint64_t prof_launches[agx::K_COUNT]{};

    // agx_detect_batch: the next chunk's upload runs on a stream of its own under the current chunk's chain and fetch
    hipStream_t upload_streams[AGX_UPLOAD_STREAMS] = {nullptr, nullptr, nullptr};  // one per staging slot, all or none
    bool upload_streams_ready = false;
    agx::TailWorkers *tail_workers = nullptr;  // option "tail_threads" > 1: one frame's board search on several threads
    int tail_threads = 1;
    agx::WorkerPool *pool = nullptr;  // agx_detect_batch: worker threads of the host tail
    int pool_threads = 0;
    std::vector<agx_saddle> scratch_saddles;  // host staging of agx_detect / agx_detect_planes (reused)

    // option "device_tail": agx_detect_batch's board search + decode on the device (tail_kernels.hip); frames the kernel
    // hands back (TAIL_UNCERTAIN / TAIL_CAPACITY) take the host tail
    int device_tail = -1;  // -1: by the batch's size, where this process's atan2f is the routine the kernel restates; 0 off; 1 on
    bool tail_ready = false;        // code list on the device and the kernel's attributes set for this device: all or nothing
    int tail_debug_band_mdeg = 0;   // option "tail_debug_band" (tests of the hand-back path), thousandths of a degree
    size_t tail_frames = 0, dtail_frames = 0;      // layout of SB_TAGS + SB_TAIL_TABLE and of SB_DTAGS + SB_DTABLE: rows ...
    uint32_t tail_tag_cap = 0, dtail_tag_cap = 0;  // ... and tags per row (0: the pair does not exist)
    int last_tail_frames = 0, last_tail_fallbacks = 0, last_tail_uncertain = 0;  // of the last agx_detect_batch call
    agx::DetectPending detect;          // BATCH_DETECT: what agx_detect_batch_fetch needs of it
    agx::RefinePending refine;          // BATCH_REFINE: what agx_refine_points_fetch needs of it
    int refine_general_kernel = 0;      // option "refine_general_kernel": half_size_patch 2 runs k_refine_patch<2> too
    int last_refine_kernel = 0;         // option "last_refine_kernel": the last refine batch ran 0 = k_refine_points, 1 = k_refine_patch
    std::vector<agx::RefinePatchConsts> patch_consts;  // host copy of SB_REFINE_CONSTS (the upload's source)
    bool patch_consts_uploaded = false;
    std::vector<uint32_t> refine_host;  // its host staging when per-frame counts were given (records, statuses, counts)
    agx::DecodePending decode;          // BATCH_DECODE: what agx_decode_quads_fetch needs of it
    std::vector<uint64_t> decode_host;  // its host staging when per-frame counts were given (bits, tags, statuses, counts)
    agx::FindPending find;              // BATCH_FIND: what agx_find_boards_fetch needs of it
    int last_list_frames[agx::LIST_STAGES]{}, last_list_handed_back[agx::LIST_STAGES]{};  // of each stage's last fetch (LIST_*)
    agx::ClustersPending clusters;      // BATCH_CLUSTERS: what agx_clusters_fetch needs of it
    agx::GrowPending grow;              // BATCH_GROW: what agx_grow_boards_fetch needs of it
    agx::InitPending init;              // BATCH_INIT: what agx_init_quads_fetch needs of it
    int last_extra_us[agx::XT_COUNT]{};  // harvest_events: the XT_* launches' last times (profiling level 2)

    std::string last_error;
};

namespace agx {
int fail(agx_detector *d, int status, const std::string &msg);  // sets agx_last_error, returns status
// This batch replaces whatever was in flight: nothing is fetchable and SB_FRONT names no batch until the enqueue says otherwise
inline void begin_batch(agx_detector *det)
{
    det->batch = BATCH_NONE;
    det->front_format = -1;
}
// the chain's results of the batch in flight are there to be read (agx_saddles_batch_fetch's rule, agx_debug_fetch, the tails)
inline bool chain_in_flight(const agx_detector *det) { return det->batch == BATCH_SADDLES || det->batch == BATCH_DETECT; }
// A fetch of `wanted`'s pair: AGX_OK where that is the batch in flight, else AGX_ERR_STATE with the pair that is (or none)
int refuse_other_batch(agx_detector *det, int wanted);
// AGX_OK, or the status and message of the first rule b breaks: null frames / frame count, format, then size and strides
int check_frame_batch(agx_detector *det, const FrameBatch &b, const BatchRules &rules);
// The payload of slot `which`, at least `bytes` long, or nullptr (the slot is then empty).  kind: 0 device, 1 pinned host,
// 2 pinned host mapped into the device (dev() = its device address).  A slot that is large enough is returned as it is;
// otherwise the handle's stream is waited for first -- work in flight may still read the buffer about to be freed -- and the
// slot is freed and allocated again: whatever pointed into it is void.
// DetectPending::d_luma and args.frames point into SB_LUMA_D / SB_FRONT from an agx_detect_batch_enqueue to its fetch.  Those
// two slots are grown only behind an enqueue's begin_batch (batch_enqueue_impl; chunk_luma8 and agx_detect, which follow their
// own enqueue), when no batch points into them any more; the fetch itself grows SB_FETCH_LUMA only.
void *side_ensure(agx_detector *d, int which, size_t bytes, int kind);
// Two slots that are only of use together (SB_LUMA_D + SB_LUMA_H, SB_TAGS + SB_TAIL_TABLE, SB_DTAGS + SB_DTABLE): both as
// asked for, or both empty
bool side_ensure_pair(agx_detector *d, int a, size_t bytes_a, int kind_a, int b, size_t bytes_b, int kind_b);
void side_free(agx_detector *d, int which);
// the last batch's compact list in the detector's pinned host mirror (valid until the next enqueue; frame f's list =
// counts[f] records from offsets[f]) + per-frame status (AGX_ERR_CAPACITY: a device-side list of the frame overflowed, its
// count is 0); waits for the device
int fetch_compact(agx_detector *det, const agx_saddle **records, uint32_t *counts, uint32_t *offsets, int *status);
// Wait for whatever is enqueued and forget it (an error path between enqueue and fetch).
void abandon_batch(agx_detector *det);
// disagreements between this process's atan2f and the routine the device tail restates (libm_f32.h), checked once per process
// on 2^20 operand pairs: the device tail is offered only where there are none
uint64_t libm_check_once();
// detect over a batch in device memory, stream-ordered (detect_batch.cpp)
// results: RESULTS_* (RESULTS_GROUP: d_counts = the packed frame table, d_tags = the slab of slab_records records)
int detect_enqueue_impl(agx_detector *det, const void *d_frames, int n_frames, int width, int height, size_t row_stride_bytes,
                        size_t frame_stride_bytes, int format, uint32_t cap_per_frame, int results, agx_tag *d_tags,
                        uint32_t *d_counts, int *d_status, uint32_t slab_records);
int detect_fetch_impl(agx_detector *det, agx_tag *out, uint32_t *counts, int *frame_status, int n_threads);
// try_decode_quad of caller-given quads over a batch in device memory (detect_batch.cpp: to_luma8, k_decode_quads, the fetch)
int decode_quads_enqueue_impl(agx_detector *det, const void *d_frames, int n_frames, int width, int height, size_t row_stride_bytes,
                              size_t frame_stride_bytes, int format, const void *d_quads, size_t point_stride_bytes,
                              uint32_t quads_per_frame, const uint32_t *d_counts, const uint32_t *d_point_status, agx_tag *d_tags,
                              uint32_t *d_status, uint64_t *d_bits);
int decode_quads_fetch_impl(agx_detector *det, agx_tag *out, uint32_t *status, uint64_t *bits);
// the decode's three stages on caller-owned device arrays (detect_batch.cpp: k_decode_positions, to_luma8 + k_bit_code, k_best_tag)
// edge_bits 1 .. 8, border_bits 0 .. 16, a finite margin and a source square of tag_affine that is not a point
bool decode_square_ok(int border_bits, int edge_bits, float margin);
int decode_positions_enqueue_impl(agx_detector *det, const void *d_quads, size_t point_stride_bytes, int n_frames, uint32_t quads_per_frame,
                                  const uint32_t *d_counts, const uint32_t *d_point_status, uint32_t img_w, uint32_t img_h, int border_bits,
                                  int edge_bits, float margin, float *d_points, uint32_t *d_status, int model);
// side_bits 1 .. 40, a finite margin and a source square that is not a point; tag_affine / tag_homography per slot (k_tag_maps)
bool tag_square_ok(int side_bits, float margin);
int tag_maps_enqueue_impl(agx_detector *det, const void *d_quads, size_t point_stride_bytes, int n_frames, uint32_t quads_per_frame,
                          const uint32_t *d_counts, const uint32_t *d_point_status, int side_bits, float margin, int model, float *d_maps,
                          uint32_t *d_status);
int bit_code_enqueue_impl(agx_detector *det, const void *d_frames, int n_frames, int width, int height, size_t row_stride_bytes,
                          size_t frame_stride_bytes, int format, const float *d_points, uint32_t points_per_slot, uint32_t quads_per_frame,
                          const uint32_t *d_counts, const uint32_t *d_status_in, int valid_brightness_threshold, uint32_t max_invalid_bit,
                          uint64_t *d_bits, uint32_t *d_status);
int best_tag_enqueue_impl(agx_detector *det, const uint64_t *d_bits, uint32_t n_slots, uint32_t quads_per_frame, const uint32_t *d_counts,
                          const uint32_t *d_status_in, int thres, const uint64_t *d_codes, uint32_t n_codes, int edge_bits, const void *d_quads,
                          size_t point_stride_bytes, uint32_t *d_ids, uint32_t *d_rotations, uint32_t *d_status, agx_tag *d_tags);
// try_find_best_board of caller-given saddle lists over a batch in device memory (detect_batch.cpp: k_find_boards, the fetch)
int find_boards_enqueue_impl(agx_detector *det, const void *d_saddles, size_t saddle_stride_bytes, int n_frames, uint32_t saddles_per_frame,
                             const uint32_t *d_counts, const void *d_frame_table, const uint32_t *d_point_status, uint32_t quads_per_frame,
                             uint32_t *d_quads, float *d_quad_points, uint32_t *d_n_quads, uint32_t *d_status);
int find_boards_fetch_impl(agx_detector *det, uint32_t *quads, float *quad_points, uint32_t *n_quads, uint32_t *status, int n_threads);
// boards from caller-given seed quads over the same lists (detect_batch.cpp: k_grow_boards, the fetch's host form)
int grow_boards_enqueue_impl(agx_detector *det, const void *d_saddles, size_t saddle_stride_bytes, int n_frames, uint32_t saddles_per_frame,
                             const uint32_t *d_counts, const void *d_frame_table, const uint32_t *d_point_status, const uint32_t *d_seed_quads,
                             uint32_t seeds_per_frame, const uint32_t *d_seed_counts, float spacing_ratio, uint32_t stop_score, int flags,
                             uint32_t quads_per_frame, uint32_t *d_quads, float *d_quad_points, uint32_t *d_n_quads, uint32_t *d_status,
                             uint32_t *d_seed_scores, uint32_t *d_best_seed);
int grow_boards_fetch_impl(agx_detector *det, int n_threads);
// init_quads of caller-given seed saddles over the same lists (detect_batch.cpp: k_init_quads, the fetch's host form)
int init_quads_enqueue_impl(agx_detector *det, const void *d_saddles, size_t saddle_stride_bytes, int n_frames, uint32_t saddles_per_frame,
                            const uint32_t *d_counts, const void *d_frame_table, const uint32_t *d_point_status, const uint32_t *d_seed_saddles,
                            uint32_t seeds_per_frame, const uint32_t *d_seed_counts, uint32_t n_nearest, uint32_t quads_per_frame,
                            uint32_t *d_quads, float *d_quad_points, uint32_t *d_n_quads, uint32_t *d_status, uint32_t *d_seed_quad_counts,
                            uint32_t *d_seeds_out, uint32_t *d_n_seeds_out);
int init_quads_fetch_impl(agx_detector *det, int n_threads);
// caller points to the nearest listed saddle over the same lists (detect_batch.cpp: k_snap_points; nothing to fetch)
int snap_points_enqueue_impl(agx_detector *det, const void *d_saddles, size_t saddle_stride_bytes, int n_frames, uint32_t saddles_per_frame,
                             const uint32_t *d_counts, const void *d_frame_table, const uint32_t *d_point_status, const void *d_points,
                             size_t row_stride_bytes, size_t point_stride_bytes, uint32_t rows_per_frame, uint32_t points_per_row,
                             const uint32_t *d_row_counts, float max_dist_sq, int flags, uint32_t *d_slots, float *d_dist_sq, uint32_t *d_rows,
                             uint32_t *d_n_rows, uint32_t *d_row_index, uint32_t *d_status);
// what both forms of the stage refuse in their point arguments (detector.cpp's agx_snap_points_tail checks the same)
bool snap_point_args_ok(size_t row_stride_bytes, size_t point_stride_bytes, uint32_t points_per_row, float max_dist_sq, int flags);
int group_detect_fetch_impl(agx_detector *det, const char *back, agx_tag *out, uint32_t *counts, int *frame_status, int n_threads);
// What group.cpp calls for rank r's share of a detect batch (detector.cpp: the entry points' argument checks and guard around
// the two functions above).  After the enqueue det->detect.device_tail says whether the pack kernel ran.
int group_detect_enqueue(agx_detector *det, const void *d_frames, int n_frames, int width, int height, size_t row_stride_bytes,
                         size_t frame_stride_bytes, int format, uint32_t cap_per_frame, uint32_t *d_table, agx_tag *d_slab,
                         uint32_t slab_records);
int group_detect_fetch(agx_detector *det, const char *back, agx_tag *out, uint32_t *counts, int *frame_status, int n_threads);
}  // namespace agx
