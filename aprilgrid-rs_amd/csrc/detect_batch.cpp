// detect_batch.cpp -- TagDetector::detect (reference src/detector.rs:505-540) over a batch of
// frames: the saddle chain of a chunk of frames runs on the device while a pool of host threads
// runs the uploads and the board search + decode (detect's loop body, :510-539) of the chunks around it.
// The host tail is the reference's exhaustive search (about a millisecond per frame and thread), so the
// end-to-end rate is set by the number of host threads the process is granted; the pool keeps them busy
// and the device work disappears behind them.
//
// The entry points -- agx_detect_batch with the host tail (detect_batch_impl) or the device tail (detect_batch_device_tail),
// agx_detect_batch_enqueue[_to] / _fetch and a group's per-rank fetch (both through resolve_on_host) -- are each a chunk or
// group loop over one set of pieces: choose_tail, device_luma, FrameResults (every per-frame rule and the call's return code),
// HostTail (a frame's host tail as a pool task), SlotRing, read_tail_table and take_host_frames.  The two upload schedulers
// stay inside their functions: they were measured separately (profiles/r6_upload_scheduling_ab.txt) and differ on purpose.
#include <hip/hip_runtime_api.h>

#include <sched.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <exception>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/aprilgrid_amd.h"
#include "detector_internal.h"
#include "host_tail.hpp"
#include "decode_stages.h"
#include "tail_kernels.h"

namespace agx {

// A fixed set of worker threads with a task queue; wait() blocks until every submitted task is done.
// submit_front() puts a task ahead of everything queued (agx_detect_batch's uploads: a chunk of frames must not
// wait behind the hundreds of board searches already queued).
class WorkerPool {
public:
    explicit WorkerPool(int n)
    {
        threads_.reserve((size_t)std::max(n, 0));
        try {
            for (int i = 0; i < n; ++i) threads_.emplace_back([this] { run(); });
        } catch (...) {  // no more threads (std::system_error): the ones already running are joined before the error leaves
            stop_and_join();
            throw;
        }
    }
    ~WorkerPool() { stop_and_join(); }
    void stop_and_join() noexcept
    {
        try {
            {
                std::lock_guard<std::mutex> lk(m_);
                stop_ = true;
            }
            cv_.notify_all();
            for (std::thread &t : threads_)
                if (t.joinable()) t.join();
        } catch (...) {
        }
    }
    WorkerPool(const WorkerPool &) = delete;
    WorkerPool &operator=(const WorkerPool &) = delete;
    int size() const { return (int)threads_.size(); }
    void submit(std::function<void()> f) { push(std::move(f), false); }
    void submit_front(std::function<void()> f) { push(std::move(f), true); }
    // Blocks until every submitted task is done; false if one of them ended in an exception since the last wait (a task must
    // not unwind out of its thread: run() catches, the caller of wait() learns of it)
    bool wait()
    {
        std::unique_lock<std::mutex> lk(m_);
        done_.wait(lk, [this] { return pending_ == 0; });
        const bool ok = !failed_;
        failed_ = false;
        return ok;
    }

private:
    void push(std::function<void()> f, bool front)
    {
        {
            std::lock_guard<std::mutex> lk(m_);
            if (front) q_.push_front(std::move(f));
            else q_.push_back(std::move(f));
            ++pending_;
        }
        cv_.notify_one();
    }
    void run()
    {
        for (;;) {
            std::function<void()> f;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [this] { return stop_ || !q_.empty(); });
                if (q_.empty()) return;  // stop_ and nothing left
                f = std::move(q_.front());
                q_.pop_front();
            }
            bool threw = false;
            try {
                f();
            } catch (...) {
                threw = true;
            }
            {
                std::lock_guard<std::mutex> lk(m_);
                if (threw) failed_ = true;
                if (--pending_ == 0) done_.notify_all();
            }
        }
    }
    std::vector<std::thread> threads_;
    std::deque<std::function<void()>> q_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    size_t pending_ = 0;
    bool stop_ = false, failed_ = false;
};

void destroy_worker_pool(WorkerPool *p) { delete p; }
WorkerPool *create_worker_pool(int n_threads) { return new WorkerPool(n_threads); }

// Workers of one frame's board search (option "tail_threads"): n - 1 pool threads plus the caller.
class PoolTailWorkers : public TailWorkers {
public:
    explicit PoolTailWorkers(int n) : n_(n), pool_(n - 1) {}
    int size() const override { return n_; }
    void run(int n, const std::function<void(int)> &f) override
    {
        int submitted = 1;
        std::exception_ptr mine;
        try {
            for (int t = 1; t < n; ++t, ++submitted) pool_.submit([&f, t] { f(t); });
            if (n > 0) f(0);
        } catch (...) {  // (the tasks already queued hold a reference to f: they finish before the error leaves)
            mine = std::current_exception();
        }
        const bool ok = pool_.wait();
        if (mine) std::rethrow_exception(mine);
        if (!ok) throw std::bad_alloc();  // a share of the search ran out of memory on its thread
    }

private:
    int n_;
    WorkerPool pool_;
};
TailWorkers *create_tail_workers(int n_threads) { return n_threads > 1 ? new PoolTailWorkers(std::min(n_threads, 64)) : nullptr; }
void destroy_tail_workers(TailWorkers *w) { delete w; }

// ---- what agx_detect_batch and the enqueue / fetch pair need of the handle beyond its fields -----------------------------------
// The detector's worker pool: created on first use, replaced when n_threads changes (throws where threads cannot be created:
// the entry points catch)
static WorkerPool *worker_pool(agx_detector *det, int n_threads)
{
    if (n_threads < 1) return nullptr;
    if (det->pool && det->pool_threads != n_threads) {
        destroy_worker_pool(det->pool);
        det->pool = nullptr;
    }
    if (!det->pool) {
        det->pool_threads = 0;
        det->pool = create_worker_pool(n_threads);
        det->pool_threads = n_threads;
    }
    return det->pool;
}
// The upload streams, one per staging slot (created on first use, all of them or none: a failure half way destroys what
// exists, so that a later call starts over instead of finding a half-initialised set); nullptr on failure
static const hipStream_t *upload_streams(agx_detector *det)
{
    if (!det->upload_streams_ready) {
        hipError_t e = hipSuccess;
        for (int i = 0; i < AGX_UPLOAD_STREAMS && e == hipSuccess; ++i)
            e = hipStreamCreateWithFlags(&det->upload_streams[i], hipStreamNonBlocking);
        if (e != hipSuccess) {
            for (int i = 0; i < AGX_UPLOAD_STREAMS; ++i) {
                if (det->upload_streams[i]) (void)hipStreamDestroy(det->upload_streams[i]);
                det->upload_streams[i] = nullptr;
            }
            return nullptr;
        }
        det->upload_streams_ready = true;
    }
    return det->upload_streams;
}
// u8 luma of a chunk of L16 / colour frames (device pointers), computed on the device behind whatever is on the detector's
// stream: *d_out = where it is on the device (the device tail reads it there) and, with h_out, copied into pinned host memory:
// [n_frames][H][W] at *h_out (valid after the stream has been waited for -- the chunk's fetch does).  The staging is a ring
// of n_slots chunks of chunk_capacity_frames; the caller reuses a slot when the host tails that read it are done.
static int chunk_luma8(agx_detector *det, const void *d_frames, int n_frames, int width, int height, size_t row_stride, size_t frame_stride,
                       int format, int slot, int n_slots, size_t chunk_capacity_frames, const uint8_t **h_out, const uint8_t **d_out)
{
    const size_t plane = (size_t)width * (size_t)height, one = plane * chunk_capacity_frames;
    if (slot < 0 || slot >= n_slots) return AGX_ERR_ARG;
    // a layout of the front-end kernel whose plane the chain of these very frames has just read (the batch enqueued last):
    // 8-bit: that plane IS their to_luma8; 16-bit: k_luma8 narrows it (2 bytes per pixel to read instead of the frames' 4 .. 8)
    const bool same_batch = format_front(format) && chain_in_flight(det) && det->front_format == format && det->front_src == d_frames &&
                            det->front_frames == n_frames;
    const bool front = same_batch && !format_16bit(format), front16 = same_batch && format_16bit(format);
    uint8_t *d_front = det->side[SB_FRONT].ptr<uint8_t>();
    if (front && !h_out) {
        if (d_out) *d_out = d_front;
        return AGX_OK;
    }
    if (!side_ensure_pair(det, SB_LUMA_D, (size_t)n_slots * one, 0, SB_LUMA_H, (size_t)n_slots * one, 1)) return AGX_ERR_HIP;
    uint8_t *d = det->side[SB_LUMA_D].ptr<uint8_t>() + (size_t)slot * one, *h = det->side[SB_LUMA_H].ptr<uint8_t>() + (size_t)slot * one;
    if (front) d = d_front;
    else if (front16) {
        if (launch_luma8(d_front, (size_t)width * 2, plane * 2, n_frames, AGX_L16, d, width, height, det->stream) != 0) return AGX_ERR_HIP;
    } else if (launch_luma8(d_frames, row_stride, frame_stride, n_frames, format, d, width, height, det->stream) != 0) return AGX_ERR_HIP;
    if (d_out) *d_out = d;
    if (!h_out) return AGX_OK;
    if (hipMemcpyAsync(h, d, plane * (size_t)n_frames, hipMemcpyDeviceToHost, det->stream) != hipSuccess) return AGX_ERR_HIP;
    *h_out = h;
    return AGX_OK;
}
// Option "device_tail": the board search + decode of the batch that was just enqueued, behind it on the detector's stream.
// The device evaluates angle_degree's atan2f by glibc's routine (libm_f32.h): offered only where this process's atan2f IS that
// routine -- checked once per process on 2^20 operand pairs (more in tests/test_abi_cpu.py)
uint64_t libm_check_once()
{
    // (AGX_DEBUG_LIBM_MISMATCH=1: tests of the refusal path pretend that one input differs)
    static const uint64_t mismatches = libm_atan2f_mismatches(1u << 20, 1) + (uint64_t)(tuning_env("AGX_DEBUG_LIBM_MISMATCH", 0) != 0);
    return mismatches;
}
// 0: the host tail; 1: the device tail (asked for); 2: the device tail is available and the call may choose by its size
static int device_tail_mode(const agx_detector *det)
{
    if (det->device_tail < 0) return libm_check_once() == 0 ? 2 : 0;
    return det->device_tail;
}
static void set_tail_stats(agx_detector *det, int frames, int fallbacks, int uncertain)
{
    det->last_tail_frames = frames;
    det->last_tail_fallbacks = fallbacks;
    det->last_tail_uncertain = uncertain;
}
// One-time set-up of the device tail on this handle's device: the family's code list in device memory and the kernel's
// attributes (155 KB of LDS).  All or nothing: a failure leaves nothing behind, and a later call starts over.
static int tail_prepare(agx_detector *det)
{
    if (det->tail_ready) return AGX_OK;
    if (hipSetDevice(det->device) != hipSuccess) return AGX_ERR_HIP;  // (the kernel's attributes are set on the current device)
    const size_t bytes = (size_t)det->fam.n_codes * sizeof(uint64_t);
    void *d_codes = side_ensure(det, SB_CODES, bytes, 0);
    if (!d_codes || hipMemcpy(d_codes, det->fam.codes, bytes, hipMemcpyHostToDevice) != hipSuccess || init_tail_kernels() != 0) {
        side_free(det, SB_CODES);
        return AGX_ERR_HIP;
    }
    det->tail_ready = true;
    return AGX_OK;
}
// d_luma = the frames' u8 luma in device memory (L8 frames: the frames themselves).  The results: tags[f * stride ..] (stride
// = the pair's tag capacity, >= this call's tag_cap), table[4 f] = count, table[4 f + 1] = TAIL_* status (+ 2: the frame's 100 MHz
// ticks, + 3: saddles | seeds << 16) -- in mapped pinned host memory (fetch_tail waits for them) or, to_device
// (agx_detect_batch_enqueue_to), in a pair of device buffers that publish_tags and the fetch read.  Either pair grows to the
// largest frame count and the largest capacity seen.
static int enqueue_tail(agx_detector *det, const void *d_luma, size_t luma_row_stride, size_t luma_frame_stride, uint32_t tag_cap, bool to_device)
{
    if (!chain_in_flight(det) || det->external_out) return AGX_ERR_STATE;
    const ChainArgs &a = det->args;
    if (tag_cap == 0 || luma_row_stride > 0x7fffffffu) return AGX_ERR_ARG;
    if (tag_cap > 128u) tag_cap = 128u;  // (the kernel's own list of distinct ids; frames beyond it take the host tail)
    if (const int rc = tail_prepare(det)) return rc;
    size_t &frames = to_device ? det->dtail_frames : det->tail_frames;
    uint32_t &stride = to_device ? det->dtail_tag_cap : det->tail_tag_cap;
    const int sb_tags = to_device ? SB_DTAGS : SB_TAGS, sb_table = to_device ? SB_DTABLE : SB_TAIL_TABLE;
    const SideBuf &tags = det->side[sb_tags], &table = det->side[sb_table];
    if ((size_t)a.n_frames > frames || tag_cap > stride) {
        const size_t F = std::max((size_t)a.n_frames, frames);
        const uint32_t cap = std::max(tag_cap, stride);
        frames = 0;  // (nothing usable until both tables exist)
        stride = 0;
        const int kind = to_device ? 0 : 2;
        if (!side_ensure_pair(det, sb_tags, F * cap * sizeof(agx_tag), kind, sb_table, F * 4 * sizeof(uint32_t), kind)) return AGX_ERR_HIP;
        frames = F;
        stride = cap;
    }
    TailArgs t{};
    t.saddles = a.out;
    t.ctr = a.ctr;
    t.n_frames = a.n_frames;
    t.luma = static_cast<const uint8_t *>(d_luma);
    t.luma_frame_stride = (long long)luma_frame_stride;
    t.luma_row_stride = (int)luma_row_stride;
    t.W = a.W;
    t.H = a.H;
    t.edge = det->fam.edge;
    t.border = det->fam.border;
    t.hamming = det->fam.hamming;
    t.n_codes = det->fam.n_codes;
    t.codes = det->side[SB_CODES].ptr<uint64_t>();
    t.max_boards = det->params.max_num_of_boards;
    t.tags = to_device ? tags.ptr<agx_tag>() : tags.dev<agx_tag>();
    t.table = to_device ? table.ptr<uint32_t>() : table.dev<uint32_t>();
    t.tag_cap = tag_cap;  // this call's: a frame with more tags is handed back (TAIL_CAPACITY), whatever the table could hold
    t.tag_stride = stride;
    t.debug_band = (float)det->tail_debug_band_mdeg * 1e-3f;
    t.debug = tuning_env("AGX_TAIL_DEBUG", 0);
    t.debug_frame = tuning_env("AGX_TAIL_DEBUG_FRAME", 0);
    if (launch_board_tail(t, det->stream) != 0) return AGX_ERR_HIP;
    return AGX_OK;
}
// agx_detect_batch_enqueue_to: the device tail's results of the batch (device buffers) into the caller's layout, behind the
// tail on the detector's stream (tail_kernels.hip, k_publish_tags)
static int publish_tags(agx_detector *det, uint32_t cap_per_frame, agx_tag *d_tags, uint32_t *d_counts, int *d_status)
{
    if (!chain_in_flight(det) || !det->dtail_frames) return AGX_ERR_STATE;
    const int e = launch_publish_tags(det->side[SB_DTABLE].ptr<uint32_t>(), det->side[SB_DTAGS].ptr<agx_tag>(), det->dtail_tag_cap, det->args.ctr,
                                      det->args.n_frames, cap_per_frame, d_tags, d_counts, d_status, det->stream);
    return e == 0 ? AGX_OK : AGX_ERR_HIP;
}
// agx_group_detect_enqueue: the same results packed -- frame table + slab in the group's device buffers (k_pack_scan, k_pack_tags)
static int pack_tags(agx_detector *det, uint32_t cap_per_frame, uint32_t *d_table, agx_tag *d_slab, uint32_t slab_records)
{
    if (!chain_in_flight(det) || !det->dtail_frames) return AGX_ERR_STATE;
    const int e = launch_pack_tags(det->side[SB_DTABLE].ptr<uint32_t>(), det->side[SB_DTAGS].ptr<agx_tag>(), det->dtail_tag_cap, det->args.ctr,
                                   det->args.n_frames, cap_per_frame, d_table, d_slab, slab_records, det->stream);
    return e == 0 ? AGX_OK : AGX_ERR_HIP;
}
// Waits for the device; then the tail's results in mapped pinned host memory, rows *tag_stride apart
static int fetch_tail(agx_detector *det, const agx_tag **tags, const uint32_t **table, uint32_t *tag_stride)
{
    if (hipStreamSynchronize(det->stream) != hipSuccess) return AGX_ERR_HIP;
    *tags = det->side[SB_TAGS].ptr<agx_tag>();
    *table = det->side[SB_TAIL_TABLE].ptr<uint32_t>();
    *tag_stride = det->tail_tag_cap;
    return AGX_OK;
}

// ---- the pieces every detect-over-a-batch entry point is put together from ---------------------------------------------------
// Which tail a call takes: 1 the device tail, 0 the host tail, < 0 the call's error.  Asked for (option "device_tail" 1): the
// one-time set-up's failure (code list, 155 KB of LDS for the kernel) is the call's; left to choose: `by_size` decides, and a
// failed set-up means the host tail, which needs nothing from the device.
static int choose_tail(agx_detector *det, bool by_size)
{
    const int mode = device_tail_mode(det);
    if (mode != 1 && !(mode == 2 && by_size)) return 0;
    const int prc = tail_prepare(det);
    if (prc && mode == 1) return prc;
    return prc ? 0 : 1;
}

// The frames' u8 luma in device memory, as the kernels that decode from it read it (detector.rs:507): L8 frames are their own;
// anything else is converted behind whatever is on the detector's stream (chunk_luma8, one slot of `capacity_frames`)
struct DeviceLuma {
    const uint8_t *d = nullptr;
    size_t row = 0, frame = 0;
};
static int device_luma(agx_detector *det, const void *d_frames, int n_frames, int width, int height, size_t row_stride, size_t frame_stride,
                       int format, size_t capacity_frames, DeviceLuma &l)
{
    l.d = static_cast<const uint8_t *>(d_frames);
    l.row = row_stride;
    l.frame = frame_stride;
    if (format == AGX_L8) return AGX_OK;
    l.row = (size_t)width;
    l.frame = (size_t)width * (size_t)height;
    return chunk_luma8(det, d_frames, n_frames, width, height, row_stride, frame_stride, format, 0, 1, capacity_frames, nullptr, &l.d);
}

// The per-frame outcome of one call: where a frame's rows go, its count, its status, and what the call's return code is derived
// from.  The calling thread and the pool's tasks write to it, each frame by one of them.
class FrameResults {
public:
    // Rows at out + f * cap; counts and statuses straight into the caller's arrays (agx_detect_batch; status may be null) ...
    FrameResults(agx_tag *out, uint32_t cap, uint32_t *counts, int *status) : out_(out), cap_(cap), counts_(counts), status_(status) {}
    // ... or held here (the fetches: 0 and AGX_OK until a frame is stored, handed over once the call is known to have succeeded),
    // and with `rows` the rows as well (_enqueue_to: bound for the caller's device arrays)
    void hold(int n_frames, bool rows)
    {
        cnt_.assign((size_t)n_frames, 0u);
        st_.assign((size_t)n_frames, AGX_OK);
        if (rows) rows_.resize((size_t)n_frames);
        counts_ = cnt_.data();
        status_ = st_.data();
    }
    // Frame f has these tags.  More than cap: AGX_ERR_CAPACITY with the true count, and no row is written -- reported, never
    // truncated.  tags == nullptr: the rows are where they belong already (_enqueue_to: k_publish_tags has put them there).
    void store(int f, const agx_tag *tags, size_t n)
    {
        counts_[f] = (uint32_t)n;
        int s = AGX_OK;
        if (n > cap_) s = record(AGX_ERR_CAPACITY);
        else if (tags && n && !rows_.empty()) rows_[(size_t)f].assign(tags, tags + n);
        else if (tags && n) std::memcpy(out_ + (size_t)f * cap_, tags, n * sizeof(agx_tag));
        if (status_) status_[f] = s;
    }
    // A list of frame f's chain overflowed with status s: no tags, that status -- reported, never truncated
    void chain_overflowed(int f, int s)
    {
        counts_[f] = 0;
        if (status_) status_[f] = record(s);
    }
    // Host memory ran out inside frame f's search: the call fails as a whole
    void out_of_memory(int f)
    {
        counts_[f] = 0;
        if (status_) status_[f] = AGX_ERR_NOMEM;
        nomem_.store(true);
    }
    bool out_of_memory() const { return nomem_.load(); }
    // The call's return code once every frame is in.  agx_detect_batch: the first status other than AGX_OK that was recorded ...
    int first_recorded() const { return nomem_.load() ? AGX_ERR_NOMEM : first_bad_.load(); }
    // ... the fetches: that of the lowest frame, as the held counts and statuses (those of the frames `only` marks; nullptr:
    // all) go to the caller's arrays (either may be null)
    int hand_over(uint32_t *counts, int *status, int n_frames, const char *only) const
    {
        int rc = AGX_OK;
        for (int f = 0; f < n_frames; ++f) {
            if (only && !only[f]) continue;
            if (counts) counts[f] = cnt_[(size_t)f];
            if (status) status[f] = st_[(size_t)f];
            if (rc == AGX_OK) rc = st_[(size_t)f];
        }
        return rc;
    }
    // The call failed as a whole (not a frame's own status): no frame's result is valid -- every frame's slot says so, so that a
    // caller who looks at the per-frame arrays only cannot mistake an untouched slot for "no tags"
    static void fail_all(int rc, uint32_t *counts, int *status, int n_frames)
    {
        for (int f = 0; f < n_frames; ++f) {
            if (counts) counts[f] = 0;
            if (status) status[f] = rc;
        }
    }
    uint32_t cap() const { return cap_; }
    const uint32_t *counts() const { return counts_; }
    const int *statuses() const { return status_; }
    const std::vector<agx_tag> &held_rows(int f) const { return rows_[(size_t)f]; }

private:
    int record(int s)
    {
        int exp = AGX_OK;
        first_bad_.compare_exchange_strong(exp, s);
        return s;
    }
    agx_tag *out_;
    uint32_t cap_;
    uint32_t *counts_;
    int *status_;
    std::vector<uint32_t> cnt_;
    std::vector<int> st_;
    std::vector<std::vector<agx_tag>> rows_;
    std::atomic<int> first_bad_{AGX_OK};
    std::atomic<bool> nomem_{false};
};

// Buffers that pool tasks read, reused in turn: a slot is refilled when ITS tasks are done (a counter per slot) -- no barrier
// over the pool between refills.
class SlotRing {
public:
    static constexpr int kSlots = 4;
    void wait_free(int r)
    {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return left_[r] == 0; });
    }
    // make(0) .. make(n - 1) onto the pool, each of which calls done(r) as its last act
    template <class Make>
    void submit(WorkerPool &pool, int r, int n, Make make)
    {
        {
            std::lock_guard<std::mutex> lk(m_);
            left_[r] = n;
        }
        int submitted = 0;
        try {
            for (; submitted < n; ++submitted) pool.submit(make(submitted));
        } catch (...) {  // a task could not be queued: the slot's counter must not wait for tasks that will never run
            std::lock_guard<std::mutex> lk(m_);
            left_[r] -= n - submitted;
            throw;
        }
    }
    void done(int r)
    {
        bool last;
        {
            std::lock_guard<std::mutex> lk(m_);
            last = --left_[r] == 0;
        }
        if (last) cv_.notify_all();
    }

private:
    std::mutex m_;
    std::condition_variable cv_;
    int left_[kSlots] = {0, 0, 0, 0};  // tasks of the slot not finished yet (guarded by m_)
};

// The host tail of one frame as a pool task: board search + decode of its saddle list over its u8 luma -- `px` at `pitch`, which
// is that luma (format AGX_L8: an L8 frame itself, or a plane converted on the device) or the caller's host frame in `format`,
// run through the host's own to_luma8 first.  Nothing unwinds out of a worker thread: host memory exhaustion becomes the
// frame's status.
struct HostTail {
    const FamilyInfo *fam;
    int max_boards, f;
    const agx_saddle *saddles;
    uint32_t n_saddles;
    const uint8_t *px;
    size_t pitch;
    int width, height, format;
    FrameResults *res;
    SlotRing *ring;  // with a ring: the slot whose buffers this task reads
    int slot;
    void operator()() const
    {
        try {
            std::vector<uint8_t> grey;
            const uint8_t *g = px;
            size_t gstride = pitch;
            if (format != AGX_L8) {
                grey.resize((size_t)width * (size_t)height);
                (void)luma8(px, width, height, pitch, format, grey.data());
                g = grey.data();
                gstride = (size_t)width;
            }
            const std::vector<agx_tag> &tags = detect_tail_scratch(*fam, max_boards, saddles, n_saddles, g, width, height, gstride);
            res->store(f, tags.data(), tags.size());
        } catch (...) {
            res->out_of_memory(f);
        }
        if (ring) ring->done(slot);
    }
};

// The device tail's table of n frames (table[4 f] count, table[4 f + 1] TAIL_* status), the first of which is the call's frame
// f0: TAIL_OK frames are stored from `rows` (`stride` apart; nullptr: counts only); the others are the host tail's --
// back[f] = 1, or 2 where the kernel handed the frame back as uncertain.  True if any frame was handed back.
static bool read_tail_table(const uint32_t *table, const agx_tag *rows, uint32_t stride, int f0, int n, FrameResults &res, char *back)
{
    bool any = false;
    for (int f = 0; f < n; ++f) {
        const uint32_t st = table[4 * f + 1], nt = table[4 * f];
        back[f] = st == TAIL_OK ? 0 : (st & TAIL_UNCERTAIN) ? 2 : 1;
        // (the kernel was given min(cap, 128) as its limit and hands frames beyond it back; never truncated either way)
        if (!back[f]) res.store(f0 + f, rows ? rows + (size_t)f * stride : nullptr, nt);
        else any = true;
    }
    return any;
}
// AGX_TAIL_DEBUG: the table's status bits and the kernel's ticks per frame, to stderr
static void print_tail_table(const uint32_t *table, int nf, int c0)
{
    int h[32] = {0};
    for (int f = 0; f < nf; ++f)
        for (int b = 0; b < 32; ++b) h[b] += (table[4 * f + 1] >> b) & 1u;
    for (int b = 0; b < 32; ++b)
        if (h[b]) std::fprintf(stderr, "tail status bit %d: %d frames\n", b, h[b]);
    std::vector<std::pair<uint32_t, int>> tk;
    double sum = 0;
    for (int f = 0; f < nf; ++f) {
        tk.push_back({table[4 * f + 2], f});
        sum += table[4 * f + 2];
    }
    std::sort(tk.begin(), tk.end());
    std::fprintf(stderr, "tail ticks per frame (100 MHz): mean %.0f median %u p90 %u max %u; slowest:", sum / nf, tk[(size_t)nf / 2].first,
                 tk[(size_t)nf * 9 / 10].first, tk.back().first);
    for (int i = 0; i < 5 && i < nf; ++i) {
        const int f = tk[(size_t)(nf - 1 - i)].second;
        std::fprintf(stderr, " [frame %d: %u ticks, %u saddles, %u seeds, %u tags]", c0 + f, table[4 * f + 2], table[4 * f + 3] & 0xffff, table[4 * f + 3] >> 16, table[4 * f]);
    }
    std::fprintf(stderr, "\n");
}

// Of the n frames from the call's frame f0 on that `back` marks (nullptr: every frame), given their chain statuses: a frame
// whose list overflowed is reported; the others are the host tail's -- appended to host_frames (counted from f0) and, with
// `stats` (the device tail handed them back), counted as fallbacks, those marked 2 as uncertain.
struct TailStats {
    int fallback = 0, uncertain = 0;
};
static void take_host_frames(const char *back, const int *chain_status, int f0, int n, FrameResults &res, std::vector<int> &host_frames,
                             TailStats *stats)
{
    for (int f = 0; f < n; ++f) {
        if (back && !back[f]) continue;
        if (chain_status[f] != AGX_OK) {
            res.chain_overflowed(f0 + f, chain_status[f]);
            continue;
        }
        if (stats) {
            ++stats->fallback;
            stats->uncertain += back && back[f] == 2;
        }
        host_frames.push_back(f);
    }
}

}  // namespace agx

using namespace agx;

// CPUs of this process: affinity mask, narrowed by the CPU quota of its cgroup and of the cgroups above it
// (v2: cpu.max "quota period" | "max period"; v1: cpu.cfs_quota_us / cpu.cfs_period_us)
static int cgroup_cpu_quota(const std::string &cg_root = "/sys/fs/cgroup", const char *proc_cgroup = "/proc/self/cgroup")
{
    auto read_pair = [](const std::string &path, long long &a, long long &b) -> bool {
        FILE *f = std::fopen(path.c_str(), "r");
        if (!f) return false;
        char buf[64] = {0};
        const bool got = std::fgets(buf, sizeof buf, f) != nullptr;
        std::fclose(f);
        if (!got) return false;
        if (!std::strncmp(buf, "max", 3)) { a = -1; b = 100000; return true; }
        return std::sscanf(buf, "%lld %lld", &a, &b) >= 1;
    };
    long long best = -1;  // CPUs, rounded up; -1 = no quota found
    auto take = [&](long long quota, long long period) {
        if (quota <= 0 || period <= 0) return;
        const long long cpus = std::max(1ll, (quota + period - 1) / period);
        best = best < 0 ? cpus : std::min(best, cpus);
    };
    // this process's cgroup path (v2: "0::/path"; v1: "N:cpu,cpuacct:/path")
    std::string v2_path, v1_path;
    if (FILE *f = std::fopen(proc_cgroup, "r")) {
        char line[512];
        while (std::fgets(line, sizeof line, f)) {
            std::string l(line);
            while (!l.empty() && (l.back() == '\n' || l.back() == '\r')) l.pop_back();
            const size_t c1 = l.find(':'), c2 = c1 == std::string::npos ? c1 : l.find(':', c1 + 1);
            if (c2 == std::string::npos) continue;
            const std::string ctrl = l.substr(c1 + 1, c2 - c1 - 1), path = l.substr(c2 + 1);
            if (ctrl.empty()) v2_path = path;
            else if (ctrl.find("cpu") != std::string::npos && ctrl.find("cpuset") == std::string::npos) v1_path = path;
        }
        std::fclose(f);
    }
    for (std::string p = v2_path;;) {  // the cgroup and every ancestor (inside a container the namespace root is "/")
        long long q = -1, per = 100000;
        if (read_pair(cg_root + p + (p.empty() || p.back() != '/' ? "/" : "") + "cpu.max", q, per)) take(q, per);
        if (p.empty() || p == "/") break;
        const size_t cut = p.find_last_of('/');
        p = cut == std::string::npos || cut == 0 ? "/" : p.substr(0, cut);
    }
    for (const char *ctrl : {"/cpu", "/cpu,cpuacct"}) {
        for (std::string p = v1_path.empty() ? "/" : v1_path;;) {
            long long q = -1, per = -1, dummy = 0;
            const std::string dir = cg_root + ctrl + p + (p.back() != '/' ? "/" : "");
            if (read_pair(dir + "cpu.cfs_quota_us", q, dummy) && read_pair(dir + "cpu.cfs_period_us", per, dummy)) take(q, per);
            if (p == "/") break;
            const size_t cut = p.find_last_of('/');
            p = cut == std::string::npos || cut == 0 ? "/" : p.substr(0, cut);
        }
    }
    return best < 0 ? 0 : (int)std::min<long long>(best, 1 << 20);
}

extern "C" int agx_debug_cgroup_cpu_quota(const char *cgroup_root, const char *proc_self_cgroup)
{
    try {
        if (!cgroup_root || !proc_self_cgroup) return AGX_ERR_ARG;
        return cgroup_cpu_quota(cgroup_root, proc_self_cgroup);
    } catch (...) {
        return AGX_ERR_NOMEM;
    }
}

extern "C" int agx_host_parallelism(void)
{
    try {
        static const int cached = [] {
            int n = (int)std::max(1u, std::thread::hardware_concurrency());
            cpu_set_t set;
            CPU_ZERO(&set);
            if (sched_getaffinity(0, sizeof set, &set) == 0 && CPU_COUNT(&set) > 0) n = std::min(n, CPU_COUNT(&set));
            const int quota = cgroup_cpu_quota();
            if (quota > 0) n = std::min(n, quota);
            return std::max(n, 1);
        }();
        return cached;
    } catch (...) {
        return 1;
    }
}

static int detect_batch_impl(agx_detector *det, const void *frames, const void *d_frames, int n_frames, int width, int height,
                             size_t row_stride_bytes, size_t frame_stride_bytes, int format, FrameResults &res, int n_threads);

extern "C" int agx_detect_batch(agx_detector *det, const void *frames, const void *d_frames, int n_frames, int width,
                                int height, size_t row_stride_bytes, size_t frame_stride_bytes, int format, agx_tag *out,
                                uint32_t cap_per_frame, uint32_t *counts, int *frame_status, int n_threads)
{
    int rc = AGX_ERR_ARG;
    try {
        FrameResults res(out, cap_per_frame, counts, frame_status);
        if (counts && (out || !cap_per_frame))
            rc = detect_batch_impl(det, frames, d_frames, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format, res, n_threads);
    } catch (...) {  // (the worker pool could not be created: nothing has run)
        rc = AGX_ERR_NOMEM;
    }
    // (AGX_ERR_CAPACITY is a frame's own status: the other frames' results stand)
    if (rc != AGX_OK && rc != AGX_ERR_CAPACITY && counts && n_frames > 0) FrameResults::fail_all(rc, counts, frame_status, n_frames);
    return rc;
}

// agx_detect_batch with option "device_tail": the board search and the decode run on the device behind the chain
// (tail_kernels.hip); per chunk one wait, and a few KB of tags come back instead of the saddle lists.  Frames the kernel
// hands back -- an angle comparison inside its guard band, a list beyond its fixed sizes -- take the host tail on the
// pool, as every frame does without the option: the results are the host tail's either way.
static int detect_batch_device_tail(agx_detector *det, const void *frames, const void *d_frames, int n_frames, int width, int height,
                                    size_t row_stride_bytes, size_t frame_stride_bytes, int format, FrameResults &res, WorkerPool *pool)
{
    const int device = det->device;
    constexpr int S = AGX_UPLOAD_STREAMS;
    // A frame's search occupies a workgroup of eight waves for two to five milliseconds (frames whose first seed does not
    // find the whole board cost twice the others), one workgroup per CU: a launch takes what its slowest frame takes, and
    // only launches of several times the CU count average that out.  So: chunks of up to 1024 frames; several per call only
    // so that the next one's upload runs under this one's kernels.
    const int chunk = std::max(1, std::min(n_frames, 1024));
    const int n_chunks = (n_frames + chunk - 1) / chunk;
    const size_t chunk_bytes = (size_t)chunk * frame_stride_bytes;
    uint8_t *d_stage = nullptr;
    const hipStream_t *up = nullptr;
    if (!d_frames) {
        d_stage = static_cast<uint8_t *>(side_ensure(det, SB_STAGE, (size_t)std::min(S, n_chunks) * chunk_bytes, 0));
        up = upload_streams(det);
        if (!d_stage || !up) return AGX_ERR_HIP;
    }
    std::mutex m;
    std::condition_variable cv;
    std::vector<int> uploaded;  // per chunk: 0 pending, 1 on the device, -1 failed   (guarded by m)
    std::deque<std::vector<agx_saddle>> handed_back;  // saddle lists of frames for the host tail (alive until the pool is drained)
    TailStats stats;
    int rc = AGX_OK;
    bool pending_batch = false;
    // A chunk goes up in P parts on P workers at once (a copy from pageable memory is staged by the calling thread at 10 .. 15 GB/s:
    // it takes four to six of them to fill the link), the chunks one after the other (three large chunks side by side would
    // share the link, and the first -- the one the device waits for -- would arrive with the third).  The parts form ONE
    // in-order list (index ci * P + part); up to P uploader tasks take the lowest part nobody has taken yet, copy it, and take
    // the next, until no released part is left -- then they end.  No task ever waits for another one: a pool of a single
    // thread uploads the parts one by one (a task that waited for "its" turn while lower-numbered parts were still queued
    // behind it deadlocked pools of <= 6 threads on calls of >= 4 chunks).  A chunk's parts are released when its staging
    // slot is free: the first S chunks at once, chunk ci + S when chunk ci's kernels are through.  (Measured on an 8 192-frame
    // stream, profiles/r6_upload_scheduling_ab.txt: 157.5 ms per call like round 5's gated tasks; with the uploaders waiting for
    // their stream instead of their own event 170 .. 194 ms.)
    const int P = std::max(1, std::min(6, pool->size()));
    int next_part = 0, released_parts = 0, live_uploaders = 0;  // (guarded by m)
    bool stop_uploads = false;                                   // an error ended the call: nothing more is taken (guarded by m)
    std::vector<int> parts_left;        // per chunk                                   (guarded by m)
    std::vector<char> chunk_failed;     //                                             (guarded by m)
    auto uploader = [&, device, P] {
        // An uploader waits for ITS copy (an event behind it), not for the stream to run empty: two uploaders share a stream,
        // and the other one -- and whoever takes the parts after it -- keeps enqueueing behind; waiting for the stream starved
        // single parts for tens of milliseconds and let later chunks overtake the one the device was waiting for.
        hipEvent_t mine = nullptr;
        if (hipSetDevice(device) != hipSuccess || hipEventCreateWithFlags(&mine, hipEventDisableTiming) != hipSuccess) mine = nullptr;  // (then: the stream)
        for (;;) {
            int idx = -1;
            {
                std::lock_guard<std::mutex> lk(m);
                if (stop_uploads || next_part >= released_parts) --live_uploaders;  // nothing left to take: this uploader ends
                else idx = next_part++;
            }
            if (idx < 0) break;
            const int ci = idx / P, part = idx % P;
            const int c0 = ci * chunk, nf = std::min(chunk, n_frames - c0), slot = ci % S;
            const int f0 = (int)((long long)nf * part / P), f1 = (int)((long long)nf * (part + 1) / P);
            const bool ok = f1 <= f0 ||
                            (hipSetDevice(device) == hipSuccess &&
                             hipMemcpyAsync(d_stage + (size_t)slot * chunk_bytes + (size_t)f0 * frame_stride_bytes,
                                            (const uint8_t *)frames + (size_t)(c0 + f0) * frame_stride_bytes, (size_t)(f1 - f0) * frame_stride_bytes,
                                            hipMemcpyHostToDevice, up[part % S]) == hipSuccess &&
                             (mine ? hipEventRecord(mine, up[part % S]) == hipSuccess && hipEventSynchronize(mine) == hipSuccess
                                   : hipStreamSynchronize(up[part % S]) == hipSuccess));
            {
                std::lock_guard<std::mutex> lk(m);
                if (!ok) chunk_failed[(size_t)ci] = 1;
                if (--parts_left[(size_t)ci] == 0) uploaded[(size_t)ci] = chunk_failed[(size_t)ci] ? -1 : 1;
            }
            cv.notify_all();
        }
        if (mine) (void)hipEventDestroy(mine);
    };
    // `n_more` chunks' parts may go up: tops the uploaders up to P (ahead of every queued host tail)
    auto release_chunks = [&, P](int n_more) {
        int spawn;
        {
            std::lock_guard<std::mutex> lk(m);
            released_parts += n_more * P;
            spawn = std::max(0, std::min(P - live_uploaders, released_parts - next_part));
            live_uploaders += spawn;
        }
        int started = 0;
        try {
            for (; started < spawn; ++started) pool->submit_front(uploader);
        } catch (...) {  // (a task could not be queued: the count must not include uploaders that will never run)
            std::lock_guard<std::mutex> lk(m);
            live_uploaders -= spawn - started;
            throw;
        }
    };
    try {
    uploaded.assign((size_t)n_chunks, 0);
    parts_left.assign((size_t)n_chunks, P);
    chunk_failed.assign((size_t)n_chunks, 0);
    if (!d_frames) release_chunks(std::min(S, n_chunks));
    const int tail_debug = tuning_env("AGX_TAIL_DEBUG", 0);  // (as read when the handle was created)
    std::vector<uint32_t> ns, offs;
    std::vector<int> fst, host_frames;
    std::vector<char> back;
    for (int ci = 0; ci < n_chunks; ++ci) {
        const int c0 = ci * chunk, nf = std::min(chunk, n_frames - c0);
        const uint8_t *h_chunk = (const uint8_t *)frames + (size_t)c0 * frame_stride_bytes;
        const void *d_chunk;
        if (!d_frames) {
            std::unique_lock<std::mutex> lk(m);
            cv.wait(lk, [&] { return uploaded[(size_t)ci] != 0; });
            if (uploaded[(size_t)ci] < 0) { rc = AGX_ERR_HIP; break; }
            d_chunk = d_stage + (size_t)(ci % S) * chunk_bytes;
        } else {
            d_chunk = (const uint8_t *)d_frames + (size_t)c0 * frame_stride_bytes;
        }
        rc = agx_saddles_batch_enqueue(det, d_chunk, nf, width, height, row_stride_bytes, frame_stride_bytes, format);
        if (rc) break;
        pending_batch = true;
        DeviceLuma luma;
        rc = device_luma(det, d_chunk, nf, width, height, row_stride_bytes, frame_stride_bytes, format, (size_t)chunk, luma);
        if (rc) break;
        rc = enqueue_tail(det, luma.d, luma.row, luma.frame, std::max(res.cap(), 1u), false);
        if (rc) break;
        const agx_tag *tags = nullptr;
        const uint32_t *table = nullptr;
        uint32_t tag_cap = 0;
        rc = fetch_tail(det, &tags, &table, &tag_cap);  // waits for the device
        if (rc) break;
        if (tail_debug) print_tail_table(table, nf, c0);
        back.resize((size_t)nf);
        if (read_tail_table(table, tags, tag_cap, c0, nf, res, back.data())) {
            // the saddle lists of the frames handed back (and the status of frames whose chain overflowed)
            ns.resize((size_t)nf);
            offs.resize((size_t)nf);
            fst.resize((size_t)nf);
            const agx_saddle *records = nullptr;
            rc = fetch_compact(det, &records, ns.data(), offs.data(), fst.data());
            pending_batch = false;
            if (rc) break;
            host_frames.clear();
            take_host_frames(back.data(), fst.data(), c0, nf, res, host_frames, &stats);
            for (const int f : host_frames) {  // (an L16 / colour frame: to_luma8 of the caller's frame, on the host this time)
                handed_back.emplace_back(records + offs[(size_t)f], records + offs[(size_t)f] + ns[(size_t)f]);
                const std::vector<agx_saddle> &list = handed_back.back();
                pool->submit(HostTail{&det->fam, det->params.max_num_of_boards, c0 + f, list.data(), (uint32_t)list.size(),
                                      h_chunk + (size_t)f * frame_stride_bytes, row_stride_bytes, width, height, format, &res, nullptr, 0});
            }
        } else {
            abandon_batch(det);  // (the stream is idle: the batch is done with)
            pending_batch = false;
        }
        // chain, luma and tail have read the staging slot: the chunk S ahead may go up
        if (!d_frames && ci + S < n_chunks) release_chunks(1);
    }
    } catch (...) {
        rc = AGX_ERR_NOMEM;
    }
    if (rc) {  // the call has failed: the uploaders stop at their next part instead of copying the rest of the caller's frames
        std::lock_guard<std::mutex> lk(m);
        stop_uploads = true;
    }
    (void)pool->wait();
    if (pending_batch) abandon_batch(det);
    set_tail_stats(det, n_frames, stats.fallback, stats.uncertain);
    return rc ? rc : res.first_recorded();
}

static int detect_batch_impl(agx_detector *det, const void *frames, const void *d_frames, int n_frames, int width, int height,
                             size_t row_stride_bytes, size_t frame_stride_bytes, int format, FrameResults &res, int n_threads)
{
    if (!det || !frames || n_frames <= 0) return AGX_ERR_ARG;  // (agx_detect_batch has looked at the result arrays)
    const size_t bpp = (size_t)format_px_bytes(format);
    if (!bpp || format == AGX_LF32) return AGX_ERR_FORMAT;  // the tail derives to_luma8 itself: every integer format
    if (width < 2 || height < 2) return AGX_ERR_ARG;
    const size_t frame_bytes = row_stride_bytes * format_rows(format, height);
    if (row_stride_bytes < (size_t)width * bpp || (n_frames > 1 && frame_stride_bytes < frame_bytes)) return AGX_ERR_ARG;
    // one frame: the stride between frames means nothing to the caller (0 is a natural value), but the staging
    // and the upload below are sized by it -- use the frame's own extent
    if (n_frames == 1 && frame_stride_bytes < frame_bytes) frame_stride_bytes = frame_bytes;
    // 0 = every CPU this process may keep busy: its affinity mask or its cgroup quota, whichever is smaller (threads beyond a
    // quota are not merely idle: the quota is spent sooner and EVERY thread of the process, the one driving the device
    // included, is frozen for the rest of the scheduler period -- profiles/r5_host_cpu_quota_and_tail_scaling.txt)
    if (n_threads <= 0) n_threads = agx_host_parallelism();
    WorkerPool *pool = worker_pool(det, n_threads);
    if (!pool) return AGX_ERR_ARG;
    if (hipSetDevice(det->device) != hipSuccess) return AGX_ERR_HIP;
    const int device = det->device;
    // The device tail costs a launch whose length is its slowest frame's (1.5 .. 3.5 ms) whatever the batch; the host tail costs
    // ~0.9 ms per frame and thread.  Measured on 16 threads the two meet at ~60 frames (1: 1.0 / 1.7 ms, 16: 2.1 / 3.6,
    // 48: 4.3 / 4.4, 64: 4.6 / 4.7, 96: 6.8 / 5.3, 128: 8.9 / 6.0, 256: 15.7 / 8.5): left to choose, a call of fewer than four
    // frames per host thread keeps the host tail.
    const int on_device = choose_tail(det, n_frames >= 4 * pool->size());
    if (on_device < 0) return on_device;
    if (on_device)
        return detect_batch_device_tail(det, frames, d_frames, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format, res, pool);
    set_tail_stats(det, 0, 0, 0);  // ("last_device_tail_frames" 0: this call's tails run on the host)

    // Chunks of about one frame per worker (8 .. 64): the chain of a chunk takes 0.1 ms on the device, a frame's board
    // search about a millisecond on a host thread, so small chunks cost nothing and the workers start after the first 8 .. 64 frames
    // instead of after a quarter of the batch.  Three kinds of work, none of which waits for another chunk's:
    //   uploads   (host frames only) pool tasks that jump the queue: a copy from pageable memory occupies the calling thread
    //             for its duration (0.3 ms per 16 MB chunk at the PCIe rate: profiles/r5_ubench_h2d_pageable.txt) -- it runs
    //             on the workers, up to AGX_UPLOAD_STREAMS chunks ahead, not on the thread that drives the device;
    //   chain     this thread: enqueue, luma (L16 / RGB8), one wait per chunk, the compact list into the chunk's slot;
    //   tails     pool tasks, one per frame, reading the slot; a slot is refilled when ITS tails are done (a counter per
    //             slot) -- no barrier over the pool between chunks.
    constexpr int S = AGX_UPLOAD_STREAMS, R = 4;
    const int chunk = std::max(1, std::min(n_frames, std::min(std::max(pool->size(), 8), 64)));
    const int n_chunks = (n_frames + chunk - 1) / chunk;
    const size_t chunk_bytes = (size_t)chunk * frame_stride_bytes;
    uint8_t *d_stage = nullptr;
    const hipStream_t *up = nullptr;
    if (!d_frames) {
        d_stage = static_cast<uint8_t *>(side_ensure(det, SB_STAGE, (size_t)std::min(S, n_chunks) * chunk_bytes, 0));
        up = upload_streams(det);
        if (!d_stage || !up) return AGX_ERR_HIP;
    }
    struct Slot {  // one chunk's results while its tails run
        std::vector<agx_saddle> saddles;  // compact
        std::vector<uint32_t> ns, offs;
        std::vector<int> fst;
    };
    static_assert(R <= SlotRing::kSlots, "a counter per slot");
    std::vector<Slot> slots((size_t)R);
    SlotRing ring;
    std::vector<int> host_frames;
    std::mutex m;
    std::condition_variable cv;
    std::vector<int> uploaded;   // per chunk: 0 pending, 1 on the device, -1 failed        (guarded by m)
    int rc = AGX_OK;
    bool pending_batch = false;  // a chunk is enqueued on the detector and not fetched yet
    auto upload_task = [&, device](int ci) {
        const int c0 = ci * chunk, nf = std::min(chunk, n_frames - c0), slot = ci % S;
        const bool ok = hipSetDevice(device) == hipSuccess &&
                        hipMemcpyAsync(d_stage + (size_t)slot * chunk_bytes, (const uint8_t *)frames + (size_t)c0 * frame_stride_bytes,
                                       (size_t)nf * frame_stride_bytes, hipMemcpyHostToDevice, up[slot]) == hipSuccess &&
                        hipStreamSynchronize(up[slot]) == hipSuccess;
        {
            std::lock_guard<std::mutex> lk(m);
            uploaded[(size_t)ci] = ok ? 1 : -1;
        }
        cv.notify_all();
    };
    // Nothing unwinds through the C boundary: an allocation failure on this thread (slot vectors, a task's
    // std::function) ends the loop like any other error, after the worker tasks -- which hold pointers into
    // the slots and references to the locals above -- have finished.
    try {
    uploaded.assign((size_t)n_chunks, 0);
    if (!d_frames)
        for (int ci = 0; ci < std::min(S, n_chunks); ++ci) pool->submit([&upload_task, ci] { upload_task(ci); });  // (empty queue: in order)
    for (int ci = 0; ci < n_chunks; ++ci) {
        const int c0 = ci * chunk, nf = std::min(chunk, n_frames - c0), r = ci % R;
        const uint8_t *h_chunk = (const uint8_t *)frames + (size_t)c0 * frame_stride_bytes;
        const void *d_chunk;
        ring.wait_free(r);
        if (!d_frames) {
            std::unique_lock<std::mutex> lk(m);
            cv.wait(lk, [&] { return uploaded[(size_t)ci] != 0; });
            if (uploaded[(size_t)ci] < 0) { rc = AGX_ERR_HIP; break; }
        }
        if (d_frames) d_chunk = (const uint8_t *)d_frames + (size_t)c0 * frame_stride_bytes;
        else d_chunk = d_stage + (size_t)(ci % S) * chunk_bytes;
        rc = agx_saddles_batch_enqueue(det, d_chunk, nf, width, height, row_stride_bytes, frame_stride_bytes, format);
        if (rc) break;
        pending_batch = true;
        // detector.rs:507: u8 luma for the decode.  L8 frames are their own; L16 / RGB8 chunks are converted on
        // the device behind the chain (the frames are there) and come back with the saddles
        const uint8_t *h_luma = nullptr;
        if (format != AGX_L8) {
            rc = chunk_luma8(det, d_chunk, nf, width, height, row_stride_bytes, frame_stride_bytes, format, r, R, (size_t)chunk, &h_luma, nullptr);
            if (rc) break;
        }
        Slot &sl = slots[(size_t)r];
        sl.ns.resize((size_t)nf);
        sl.offs.resize((size_t)nf);
        sl.fst.resize((size_t)nf);
        const agx_saddle *records = nullptr;
        rc = fetch_compact(det, &records, sl.ns.data(), sl.offs.data(), sl.fst.data());  // waits for the device
        pending_batch = false;
        if (rc) break;
        // chain and luma have read the staging slot: the chunk S ahead may go up (ahead of every queued tail)
        if (!d_frames && ci + S < n_chunks) pool->submit_front([&upload_task, ci] { upload_task(ci + S); });
        size_t total = 0;
        for (int f = 0; f < nf; ++f)
            if (sl.fst[(size_t)f] == AGX_OK) total = std::max(total, (size_t)sl.offs[(size_t)f] + sl.ns[(size_t)f]);
        sl.saddles.assign(records, records + total);  // (the detector's mirror is overwritten by the next chunk)
        host_frames.clear();
        take_host_frames(nullptr, sl.fst.data(), c0, nf, res, host_frames, nullptr);
        ring.submit(*pool, r, (int)host_frames.size(), [&](int i) {
            const int f = host_frames[(size_t)i];
            HostTail t{&det->fam, det->params.max_num_of_boards, c0 + f, sl.saddles.data() + sl.offs[(size_t)f], sl.ns[(size_t)f],
                       h_chunk + (size_t)f * frame_stride_bytes, row_stride_bytes, width, height, AGX_L8, &res, &ring, r};  // L8: the frame itself, at its own pitch
            if (h_luma) {
                t.px = h_luma + (size_t)f * (size_t)width * (size_t)height;
                t.pitch = (size_t)width;
            }
            return t;
        });
    }
    } catch (...) {
        rc = AGX_ERR_NOMEM;  // host memory exhausted on this thread
    }
    (void)pool->wait();  // every tail and every upload still queued (an upload may be reading the caller's frames)
    if (pending_batch) abandon_batch(det);  // an error between enqueue and fetch: no stale batch is left to be fetched later
    return rc ? rc : res.first_recorded();
}

// ---- agx_detect_batch_enqueue / _enqueue_to / agx_detect_batch_fetch: detect over a batch resident in device memory ---------
// The enqueue puts the chain, to_luma8 (L16 / RGB8: k_luma8) and, where this process may use it, the device tail on the
// detector's stream and returns without waiting.  The fetch waits, takes the device tail's tags, and runs the host tail on the
// pool for the frames the kernel handed back -- every frame without the device tail -- from the chain's compact saddle lists and
// the u8 luma of those frames only, copied down from the device.  No frame ever exists in host memory as the caller's pixels.
int agx::detect_enqueue_impl(agx_detector *det, const void *d_frames, int n_frames, int width, int height, size_t row_stride_bytes,
                             size_t frame_stride_bytes, int format, uint32_t cap_per_frame, int results, agx_tag *d_tags,
                             uint32_t *d_counts, int *d_status, uint32_t slab_records)
{
    const bool to_device = results != RESULTS_HOST;  // the tail's rows and table stay in device memory (SB_DTAGS + SB_DTABLE)
    // option "device_tail" -1 (default) or 1: the device tail wherever this process may use it (no batch-size rule: with the frames
    // on the device there is no upload for the host tail to hide behind); 0, or a tail this process may not use: the host tail
    const int on_device = choose_tail(det, true);
    if (on_device < 0) return on_device;
    int rc = agx_saddles_batch_enqueue(det, d_frames, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format);
    if (rc) return rc;
    DeviceLuma luma;
    rc = device_luma(det, d_frames, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format, (size_t)n_frames, luma);
    if (!rc && on_device) rc = enqueue_tail(det, luma.d, luma.row, luma.frame, std::max(cap_per_frame, 1u), to_device);
    if (!rc && results == RESULTS_GROUP) {
        // a group's batch: d_counts = the packed frame table [n_frames][4], d_tags = the slab (group.cpp owns both).  Without
        // the device tail no pack kernel runs: the group fills the table with "handed back" itself
        if (on_device) rc = pack_tags(det, cap_per_frame, d_counts, d_tags, slab_records);
    } else if (!rc && to_device) {
        if (on_device) {
            rc = publish_tags(det, cap_per_frame, d_tags, d_counts, d_status);
        } else {  // every frame is the fetch's: until then count 0, AGX_ERR_STATE
            if (hipMemsetD32Async(d_counts, 0, (size_t)n_frames, det->stream) != hipSuccess ||
                hipMemsetD32Async(d_status, AGX_ERR_STATE, (size_t)n_frames, det->stream) != hipSuccess)
                rc = AGX_ERR_HIP;
        }
    }
    if (rc) {
        abandon_batch(det);  // (nothing half-enqueued is left to be fetched)
        return rc;
    }
    det->batch = BATCH_DETECT;  // (over the chain's BATCH_SADDLES)
    DetectPending &p = det->detect;
    p.results = results;
    p.device_tail = on_device != 0;
    p.n_frames = n_frames;
    p.width = width;
    p.height = height;
    p.cap = cap_per_frame;
    p.d_luma = luma.d;
    p.luma_row = luma.row;
    p.luma_frame = luma.frame;
    p.d_tags = d_tags;
    p.d_counts = d_counts;
    p.d_status = d_status;
    return AGX_OK;
}

// ---- agx_decode_quads_enqueue / _fetch: try_decode_quad (src/detector.rs:448-476) of caller-given quads ----------------------
// to_luma8 of the frames (L8: the frames themselves; else k_luma8 / the front-end kernel into SB_LUMA_D, as
// agx_detect_batch_enqueue does) and k_decode_quads on the detector's stream.  The saddle chain is not run and the workspace
// is not touched.
int agx::decode_quads_enqueue_impl(agx_detector *det, const void *d_frames, int n_frames, int width, int height, size_t row_stride_bytes,
                                   size_t frame_stride_bytes, int format, const void *d_quads, size_t point_stride_bytes,
                                   uint32_t quads_per_frame, const uint32_t *d_counts, const uint32_t *d_point_status, agx_tag *d_tags,
                                   uint32_t *d_status, uint64_t *d_bits)
{
    if (!det) return AGX_ERR_ARG;
    if (!d_frames || !d_quads || n_frames <= 0) return fail(det, AGX_ERR_ARG, "null frames, null quads or n_frames <= 0");
    if (!quads_per_frame) return fail(det, AGX_ERR_ARG, "quads_per_frame must be > 0");
    if (point_stride_bytes < 8 || (point_stride_bytes & 3) || point_stride_bytes > 0x7fffffffu)
        return fail(det, AGX_ERR_ARG, "point_stride_bytes must be a multiple of 4 and at least 8");
    if ((d_tags == nullptr) != (d_status == nullptr)) return fail(det, AGX_ERR_ARG, "d_tags and d_status: both or neither");
    if (!d_tags && d_bits) return fail(det, AGX_ERR_ARG, "d_bits needs d_tags and d_status (internal results: the fetch's bits argument)");
    if ((((uintptr_t)d_quads | (uintptr_t)d_counts | (uintptr_t)d_point_status | (uintptr_t)d_tags | (uintptr_t)d_status) & 3) || ((uintptr_t)d_bits & 7))
        return fail(det, AGX_ERR_ARG, "quads, counts, point statuses, tags and statuses must be 4-byte aligned, bits 8-byte aligned");
    if (const int rc = check_frame_batch(det, {d_frames, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format},
                                         {/*min_side*/ 1, /*lf32*/ false, /*lone_frame_stride*/ false, /*align16*/ true, /*front_rows*/ true}))
        return rc;
    const size_t slots = (size_t)n_frames * quads_per_frame;
    if (slots >= ((size_t)1 << 29)) return fail(det, AGX_ERR_ARG, "at most 2^29 - 1 quads per batch");
    HIP_TRY(det, hipSetDevice(det->device));
    begin_batch(det);  // (SB_LUMA_D may grow below: nothing points into it any more)
    if (tail_prepare(det)) return fail(det, AGX_ERR_HIP, "hipMalloc / hipMemcpy: the family's code list");
    DeviceLuma luma;
    if (device_luma(det, d_frames, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format, (size_t)n_frames, luma))
        return fail(det, AGX_ERR_HIP, "to_luma8 of the frames on the device");
    int results = RESULTS_CALLER;
    if (!d_tags) {
        d_tags = static_cast<agx_tag *>(side_ensure(det, SB_DECODE_TAGS, slots * sizeof(agx_tag), 0));
        d_status = static_cast<uint32_t *>(side_ensure(det, SB_DECODE_STATUS, slots * sizeof(uint32_t), 0));
        d_bits = static_cast<uint64_t *>(side_ensure(det, SB_DECODE_BITS, slots * sizeof(uint64_t), 0));
        if (!d_tags || !d_status || !d_bits) return fail(det, AGX_ERR_HIP, "hipMalloc: decoded quads");
        results = RESULTS_HOST;
    }
    DecodeQuadsArgs q{};
    q.luma = luma.d;
    q.luma_frame_stride = (long long)luma.frame;
    q.luma_row_stride = (int)luma.row;
    q.W = width;
    q.H = height;
    q.n_frames = n_frames;
    q.edge = det->fam.edge;
    q.border = det->fam.border;
    q.hamming = det->fam.hamming;
    q.n_codes = det->fam.n_codes;
    q.codes = det->side[SB_CODES].ptr<uint64_t>();
    q.quads = static_cast<const uint8_t *>(d_quads);
    q.point_stride = (uint32_t)point_stride_bytes;
    q.quads_per_frame = quads_per_frame;
    q.counts = d_counts;
    q.point_status = d_point_status;
    q.tags = d_tags;
    q.status = d_status;
    q.bits = d_bits;
    const hipError_t e = (hipError_t)launch_decode_quads(q, det->stream);
    if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_decode_quads: ") + hipGetErrorString(e));
    det->batch = BATCH_DECODE;
    det->decode.results = results;
    det->decode.n_frames = n_frames;
    det->decode.quads_per_frame = quads_per_frame;
    det->decode.d_counts = d_counts;
    return AGX_OK;
}

int agx::decode_quads_fetch_impl(agx_detector *det, agx_tag *out, uint32_t *status, uint64_t *bits)
{
    if (!det) return AGX_ERR_ARG;
    if (const int other = refuse_other_batch(det, BATCH_DECODE)) return other;
    const DecodePending b = det->decode;
    const bool to_host = b.results == RESULTS_HOST;
    if (to_host && (!out || !status)) return fail(det, AGX_ERR_ARG, "null output");  // (the batch stays in flight)
    HIP_TRY(det, hipSetDevice(det->device));
    det->batch = BATCH_NONE;  // resolved by this call, whatever it returns
    const size_t slots = (size_t)b.n_frames * b.quads_per_frame;
    // host staging when counts were given (only the slots the kernel wrote reach the caller's arrays): in 8-byte words, the
    // bits, then the tags (9 x 4 bytes each), the statuses and the counts
    const size_t w_tags = slots, w_status = w_tags + (slots * sizeof(agx_tag) + 7) / 8, w_counts = w_status + (slots * 4 + 7) / 8;
    bool ok = true;
    if (to_host) {
        const agx_tag *d_tags = det->side[SB_DECODE_TAGS].ptr<agx_tag>();
        const uint32_t *d_status = det->side[SB_DECODE_STATUS].ptr<uint32_t>();
        const uint64_t *d_bits = det->side[SB_DECODE_BITS].ptr<uint64_t>();
        if (!b.d_counts) {
            ok = hipMemcpyAsync(out, d_tags, slots * sizeof(agx_tag), hipMemcpyDeviceToHost, det->stream) == hipSuccess &&
                 hipMemcpyAsync(status, d_status, slots * sizeof(uint32_t), hipMemcpyDeviceToHost, det->stream) == hipSuccess &&
                 (!bits || hipMemcpyAsync(bits, d_bits, slots * sizeof(uint64_t), hipMemcpyDeviceToHost, det->stream) == hipSuccess);
        } else {
            std::vector<uint64_t> &h = det->decode_host;
            h.resize(w_counts + ((size_t)b.n_frames * 4 + 7) / 8);
            ok = hipMemcpyAsync(h.data(), d_bits, slots * sizeof(uint64_t), hipMemcpyDeviceToHost, det->stream) == hipSuccess &&
                 hipMemcpyAsync(h.data() + w_tags, d_tags, slots * sizeof(agx_tag), hipMemcpyDeviceToHost, det->stream) == hipSuccess &&
                 hipMemcpyAsync(h.data() + w_status, d_status, slots * sizeof(uint32_t), hipMemcpyDeviceToHost, det->stream) == hipSuccess &&
                 hipMemcpyAsync(h.data() + w_counts, b.d_counts, (size_t)b.n_frames * sizeof(uint32_t), hipMemcpyDeviceToHost, det->stream) == hipSuccess;
        }
    }
    if (hipStreamSynchronize(det->stream) != hipSuccess || !ok) return fail(det, AGX_ERR_HIP, "agx_decode_quads_fetch: copy / wait");
    if (to_host && b.d_counts) {
        const std::vector<uint64_t> &h = det->decode_host;
        const char *h_tags = reinterpret_cast<const char *>(h.data() + w_tags);
        const uint32_t *h_status = reinterpret_cast<const uint32_t *>(h.data() + w_status), *h_counts = reinterpret_cast<const uint32_t *>(h.data() + w_counts);
        for (int f = 0; f < b.n_frames; ++f) {
            const size_t n = std::min(h_counts[f], b.quads_per_frame), s0 = (size_t)f * b.quads_per_frame;
            if (!n) continue;
            std::memcpy(out + s0, h_tags + s0 * sizeof(agx_tag), n * sizeof(agx_tag));
            std::memcpy(status + s0, h_status + s0, n * sizeof(uint32_t));
            if (bits) std::memcpy(bits + s0, h.data() + s0, n * sizeof(uint64_t));
        }
    }
    return AGX_OK;
}

// ---- the decode in three stages (decode_stages.hip): decode_positions (src/detector.rs:42-72), bit_code (:74-122), best_tag
// (:142-169) on caller-owned device arrays.  Like agx_filter_saddles_enqueue: every argument is checked before begin_batch, the
// launch replaces the batch in flight, and there is nothing to fetch.
static bool decode_stage_stride_ok(size_t point_stride_bytes)
{
    return point_stride_bytes >= 8 && !(point_stride_bytes & 3) && point_stride_bytes <= 0x7fffffffu;
}

bool agx::decode_square_ok(int border_bits, int edge_bits, float margin)
{
    if (edge_bits < 1 || edge_bits > 8 || border_bits < 0 || border_bits > 16 || !std::isfinite(margin)) return false;
    const float S = (float)(border_bits * 2 + edge_bits) - 1.0f + margin;  // image_util.rs:39-70: the square's far side ...
    return S != -margin;                                                   // ... and its near side: equal, the square is a point
}

int agx::decode_positions_enqueue_impl(agx_detector *det, const void *d_quads, size_t point_stride_bytes, int n_frames, uint32_t quads_per_frame,
                                       const uint32_t *d_counts, const uint32_t *d_point_status, uint32_t img_w, uint32_t img_h, int border_bits,
                                       int edge_bits, float margin, float *d_points, uint32_t *d_status, int model)
{
    if (!det) return AGX_ERR_ARG;
    if (model != AGX_TAG_MAP_AFFINE && model != AGX_TAG_MAP_HOMOGRAPHY) return fail(det, AGX_ERR_ARG, "model must be AGX_TAG_MAP_AFFINE or AGX_TAG_MAP_HOMOGRAPHY");
    if (!d_quads || !d_points || !d_status || n_frames <= 0) return fail(det, AGX_ERR_ARG, "null quads, points or status, or n_frames <= 0");
    if (!quads_per_frame) return fail(det, AGX_ERR_ARG, "quads_per_frame must be > 0");
    if (!decode_stage_stride_ok(point_stride_bytes)) return fail(det, AGX_ERR_ARG, "point_stride_bytes must be a multiple of 4 and at least 8");
    if (((uintptr_t)d_quads | (uintptr_t)d_counts | (uintptr_t)d_point_status | (uintptr_t)d_points | (uintptr_t)d_status) & 3)
        return fail(det, AGX_ERR_ARG, "quads, counts, point statuses, points and statuses must be 4-byte aligned");
    if (!decode_square_ok(border_bits, edge_bits, margin))
        return fail(det, AGX_ERR_ARG, "edge_bits 1 .. 8, border_bits 0 .. 16, a finite margin and a source square that is not a point");
    if ((size_t)n_frames * quads_per_frame >= ((size_t)1 << 29)) return fail(det, AGX_ERR_ARG, "at most 2^29 - 1 quads per batch");
    HIP_TRY(det, hipSetDevice(det->device));
    begin_batch(det);  // and there is nothing of this one to be fetched
    DecodePositionsArgs p{};
    p.quads = static_cast<const uint8_t *>(d_quads);
    p.point_stride = (uint32_t)point_stride_bytes;
    p.n_frames = n_frames;
    p.quads_per_frame = quads_per_frame;
    p.counts = d_counts;
    p.point_status = d_point_status;
    p.W = img_w;
    p.H = img_h;
    p.border = border_bits;
    p.edge = edge_bits;
    p.margin = margin;
    p.points = d_points;
    p.status = d_status;
    const hipError_t e = (hipError_t)(model == AGX_TAG_MAP_HOMOGRAPHY ? launch_positions_homography(p, det->stream) : launch_decode_positions(p, det->stream));
    if (e != hipSuccess)
        return fail(det, AGX_ERR_HIP, std::string(model == AGX_TAG_MAP_HOMOGRAPHY ? "k_positions_homography: " : "k_decode_positions: ") + hipGetErrorString(e));
    return AGX_OK;
}

bool agx::tag_square_ok(int side_bits, float margin)
{
    if (side_bits < 1 || side_bits > 40 || !std::isfinite(margin)) return false;
    return (float)side_bits - 1.0f + margin != -margin;  // (decode_square_ok's rule: the square is not a point)
}

int agx::tag_maps_enqueue_impl(agx_detector *det, const void *d_quads, size_t point_stride_bytes, int n_frames, uint32_t quads_per_frame,
                               const uint32_t *d_counts, const uint32_t *d_point_status, int side_bits, float margin, int model, float *d_maps,
                               uint32_t *d_status)
{
    if (!det) return AGX_ERR_ARG;
    if (model != AGX_TAG_MAP_AFFINE && model != AGX_TAG_MAP_HOMOGRAPHY) return fail(det, AGX_ERR_ARG, "model must be AGX_TAG_MAP_AFFINE or AGX_TAG_MAP_HOMOGRAPHY");
    if (!d_quads || !d_maps || !d_status || n_frames <= 0) return fail(det, AGX_ERR_ARG, "null quads, maps or status, or n_frames <= 0");
    if (!quads_per_frame) return fail(det, AGX_ERR_ARG, "quads_per_frame must be > 0");
    if (!decode_stage_stride_ok(point_stride_bytes)) return fail(det, AGX_ERR_ARG, "point_stride_bytes must be a multiple of 4 and at least 8");
    if (((uintptr_t)d_quads | (uintptr_t)d_counts | (uintptr_t)d_point_status | (uintptr_t)d_maps | (uintptr_t)d_status) & 3)
        return fail(det, AGX_ERR_ARG, "quads, counts, point statuses, maps and statuses must be 4-byte aligned");
    if (!tag_square_ok(side_bits, margin)) return fail(det, AGX_ERR_ARG, "side_bits 1 .. 40, a finite margin and a source square that is not a point");
    if ((size_t)n_frames * quads_per_frame >= ((size_t)1 << 29)) return fail(det, AGX_ERR_ARG, "at most 2^29 - 1 quads per batch");
    HIP_TRY(det, hipSetDevice(det->device));
    begin_batch(det);  // and there is nothing of this one to be fetched
    TagMapsArgs p{};
    p.quads = static_cast<const uint8_t *>(d_quads);
    p.point_stride = (uint32_t)point_stride_bytes;
    p.n_frames = n_frames;
    p.quads_per_frame = quads_per_frame;
    p.counts = d_counts;
    p.point_status = d_point_status;
    p.side_bits = side_bits;
    p.margin = margin;
    p.model = model;
    p.maps = d_maps;
    p.status = d_status;
    const hipError_t e = (hipError_t)launch_tag_maps(p, det->stream);
    if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_tag_maps: ") + hipGetErrorString(e));
    return AGX_OK;
}

int agx::bit_code_enqueue_impl(agx_detector *det, const void *d_frames, int n_frames, int width, int height, size_t row_stride_bytes,
                               size_t frame_stride_bytes, int format, const float *d_points, uint32_t points_per_slot, uint32_t quads_per_frame,
                               const uint32_t *d_counts, const uint32_t *d_status_in, int valid_brightness_threshold, uint32_t max_invalid_bit,
                               uint64_t *d_bits, uint32_t *d_status)
{
    if (!det) return AGX_ERR_ARG;
    if (!d_frames || !d_points || !d_bits || !d_status || n_frames <= 0) return fail(det, AGX_ERR_ARG, "null frames, points, bits or status, or n_frames <= 0");
    if (!quads_per_frame) return fail(det, AGX_ERR_ARG, "quads_per_frame must be > 0");
    if (points_per_slot < 1 || points_per_slot > 64) return fail(det, AGX_ERR_ARG, "points_per_slot must be 1 .. 64");
    if (valid_brightness_threshold < 0 || valid_brightness_threshold > 255) return fail(det, AGX_ERR_ARG, "valid_brightness_threshold must be 0 .. 255");
    if ((((uintptr_t)d_points | (uintptr_t)d_counts | (uintptr_t)d_status_in | (uintptr_t)d_status) & 3) || ((uintptr_t)d_bits & 7))
        return fail(det, AGX_ERR_ARG, "points, counts and statuses must be 4-byte aligned, bits 8-byte aligned");
    if (const int rc = check_frame_batch(det, {d_frames, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format},
                                         {/*min_side*/ 1, /*lf32*/ false, /*lone_frame_stride*/ false, /*align16*/ true, /*front_rows*/ true}))
        return rc;
    if ((size_t)n_frames * quads_per_frame >= ((size_t)1 << 29)) return fail(det, AGX_ERR_ARG, "at most 2^29 - 1 slots per batch");
    HIP_TRY(det, hipSetDevice(det->device));
    begin_batch(det);  // (SB_LUMA_D may grow below: nothing points into it any more)
    DeviceLuma luma;
    if (device_luma(det, d_frames, n_frames, width, height, row_stride_bytes, frame_stride_bytes, format, (size_t)n_frames, luma))
        return fail(det, AGX_ERR_HIP, "to_luma8 of the frames on the device");
    BitCodeArgs b{};
    b.luma = luma.d;
    b.luma_frame_stride = (long long)luma.frame;
    b.luma_row_stride = (int)luma.row;
    b.W = width;
    b.H = height;
    b.n_frames = n_frames;
    b.points = d_points;
    b.points_per_slot = points_per_slot;
    b.quads_per_frame = quads_per_frame;
    b.counts = d_counts;
    b.status_in = d_status_in;
    b.threshold = valid_brightness_threshold;
    b.max_invalid = max_invalid_bit;
    b.bits = d_bits;
    b.status = d_status;
    const hipError_t e = (hipError_t)launch_bit_code(b, det->stream);
    if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_bit_code: ") + hipGetErrorString(e));
    return AGX_OK;
}

int agx::best_tag_enqueue_impl(agx_detector *det, const uint64_t *d_bits, uint32_t n_slots, uint32_t quads_per_frame, const uint32_t *d_counts,
                               const uint32_t *d_status_in, int thres, const uint64_t *d_codes, uint32_t n_codes, int edge_bits, const void *d_quads,
                               size_t point_stride_bytes, uint32_t *d_ids, uint32_t *d_rotations, uint32_t *d_status, agx_tag *d_tags)
{
    if (!det) return AGX_ERR_ARG;
    if (!d_bits || !d_ids || !d_rotations || !d_status) return fail(det, AGX_ERR_ARG, "null bits, ids, rotations or status");
    if (!n_slots || n_slots >= (1u << 31)) return fail(det, AGX_ERR_ARG, "n_slots must be 1 .. 2^31 - 1");
    if (d_counts && (!quads_per_frame || n_slots % quads_per_frame)) return fail(det, AGX_ERR_ARG, "d_counts: n_slots must be a multiple of quads_per_frame");
    if (thres < 0 || thres > 255) return fail(det, AGX_ERR_ARG, "thres must be 0 .. 255");
    if (d_codes ? (n_codes < 1 || n_codes > 65535) : n_codes != 0)
        return fail(det, AGX_ERR_ARG, "d_codes with n_codes 1 .. 65535, or NULL with 0 (the handle's family list)");
    if (edge_bits < 1 || edge_bits > 8) return fail(det, AGX_ERR_ARG, "edge_bits must be 1 .. 8");
    if ((d_quads == nullptr) != (d_tags == nullptr)) return fail(det, AGX_ERR_ARG, "d_quads and d_tags: both or neither");
    if (d_quads && !decode_stage_stride_ok(point_stride_bytes)) return fail(det, AGX_ERR_ARG, "point_stride_bytes must be a multiple of 4 and at least 8");
    if ((((uintptr_t)d_counts | (uintptr_t)d_status_in | (uintptr_t)d_quads | (uintptr_t)d_ids | (uintptr_t)d_rotations | (uintptr_t)d_status | (uintptr_t)d_tags) & 3) ||
        (((uintptr_t)d_bits | (uintptr_t)d_codes) & 7))
        return fail(det, AGX_ERR_ARG, "counts, statuses, quads, ids, rotations and tags must be 4-byte aligned, bits and codes 8-byte aligned");
    HIP_TRY(det, hipSetDevice(det->device));
    begin_batch(det);  // and there is nothing of this one to be fetched
    if (!d_codes) {
        if (tail_prepare(det)) return fail(det, AGX_ERR_HIP, "hipMalloc / hipMemcpy: the family's code list");
        d_codes = det->side[SB_CODES].ptr<uint64_t>();
        n_codes = (uint32_t)det->fam.n_codes;
    }
    BestTagArgs t{};
    t.bits = d_bits;
    t.n_slots = n_slots;
    t.quads_per_frame = quads_per_frame;
    t.counts = d_counts;
    t.status_in = d_status_in;
    t.thres = (uint32_t)thres;
    t.codes = d_codes;
    t.n_codes = n_codes;
    t.edge = edge_bits;
    t.quads = static_cast<const uint8_t *>(d_quads);
    t.point_stride = (uint32_t)point_stride_bytes;
    t.ids = d_ids;
    t.rotations = d_rotations;
    t.status = d_status;
    t.tags = d_tags;
    const hipError_t e = (hipError_t)launch_best_tag(t, det->stream);
    if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_best_tag: ") + hipGetErrorString(e));
    return AGX_OK;
}

// ---- the three stages over caller-given saddle lists: agx_find_boards_*, agx_grow_boards_*, agx_init_quads_* ---------------------
// One kernel each on the detector's stream, one workgroup per frame.  No pixels, no chain, no workspace.  Without the device tail
// (option "device_tail" 0, or this process's atan2f is not the routine the kernel restates) the kernel only marks every frame
// AGX_BOARD_PENDING, and the fetch's host form answers them all.
namespace {
// What the three enqueues are handed alike: the lists and the result arrays
struct ListArgs {
    const void *d_saddles;
    size_t saddle_stride_bytes;
    int n_frames;
    uint32_t saddles_per_frame;
    const uint32_t *d_counts;
    const void *d_frame_table;
    const uint32_t *d_point_status;
    uint32_t quads_per_frame;
    uint32_t *d_quads;
    float *d_quad_points;
    uint32_t *d_n_quads, *d_status;
};

// The checks of the list arguments, in the one order all three refuse them in.  seeds_per_frame: null where the stage has no
// seeds; own(): the stage's own checks, between the lists' and the alignment's; own_ptrs: its own device pointers, or'ed.
// (All of it ahead of begin_batch: refused arguments leave the batch in flight.)
template <class Own>
int check_list_args(agx_detector *det, const ListArgs &l, const uint32_t *seeds_per_frame, uintptr_t own_ptrs, Own own)
{
    if (!l.d_saddles || l.n_frames <= 0) return fail(det, AGX_ERR_ARG, "null saddles or n_frames <= 0");
    if (l.saddle_stride_bytes < 20 || (l.saddle_stride_bytes & 3) || l.saddle_stride_bytes > 0x7fffffffu)
        return fail(det, AGX_ERR_ARG, "saddle_stride_bytes must be a multiple of 4 and at least 20");
    if (!l.saddles_per_frame || !l.quads_per_frame || (seeds_per_frame && !*seeds_per_frame))
        return fail(det, AGX_ERR_ARG, seeds_per_frame ? "saddles_per_frame, seeds_per_frame and quads_per_frame must be > 0"
                                                      : "saddles_per_frame and quads_per_frame must be > 0");
    if (l.d_counts && l.d_frame_table) return fail(det, AGX_ERR_ARG, "d_counts and d_frame_table: at most one of them");
    if (const int rc = own()) return rc;
    if (((uintptr_t)l.d_saddles | (uintptr_t)l.d_counts | (uintptr_t)l.d_frame_table | (uintptr_t)l.d_point_status | (uintptr_t)l.d_quads |
         (uintptr_t)l.d_quad_points | (uintptr_t)l.d_n_quads | (uintptr_t)l.d_status | own_ptrs) & 3)
        return fail(det, AGX_ERR_ARG, seeds_per_frame ? "saddles, counts, frame table, point statuses, seeds and the results must be 4-byte aligned"
                                                      : "saddles, counts, frame table, point statuses and the results must be 4-byte aligned");
    if (l.n_frames > 65535) return fail(det, AGX_ERR_ARG, "at most 65535 frames per batch");
    if ((size_t)l.n_frames * l.quads_per_frame >= ((size_t)1 << 27)) return fail(det, AGX_ERR_ARG, "at most 2^27 - 1 quad rows per batch");
    if (seeds_per_frame && (size_t)l.n_frames * *seeds_per_frame >= ((size_t)1 << 27))
        return fail(det, AGX_ERR_ARG, "at most 2^27 - 1 seed rows per batch");
    return AGX_OK;
}

// Behind the checks: this batch replaces the one in flight; host_only = the kernel will only mark the frames
int begin_list_batch(agx_detector *det, bool &host_only)
{
    HIP_TRY(det, hipSetDevice(det->device));
    begin_batch(det);
    host_only = device_tail_mode(det) == 0;
    if (!host_only && tail_prepare(det)) return fail(det, AGX_ERR_HIP, "the device tail's set-up (code list, kernel attributes)");
    return AGX_OK;
}

void fill_list_args(FindBoardsArgs &q, const agx_detector *det, const ListArgs &l, bool host_only)
{
    q.saddles = static_cast<const uint8_t *>(l.d_saddles);
    q.stride = (uint32_t)l.saddle_stride_bytes;
    q.n_frames = l.n_frames;
    q.saddles_per_frame = l.saddles_per_frame;
    q.counts = l.d_counts;
    q.frame_table = static_cast<const uint32_t *>(l.d_frame_table);
    q.point_status = l.d_point_status;
    q.quads_per_frame = l.quads_per_frame;
    q.quads = l.d_quads;
    q.quad_points = l.d_quad_points;
    q.n_quads = l.d_n_quads;
    q.status = l.d_status;
    q.debug_band = (float)det->tail_debug_band_mdeg * 1e-3f;
    q.host_only = host_only ? 1 : 0;
}

void fill_list_pending(FindPending &p, const ListArgs &l, int results, const uint32_t *d_seed_counts, uint32_t seeds_per_frame)
{
    p.results = results;
    p.n_frames = l.n_frames;
    p.saddles_per_frame = l.saddles_per_frame;
    p.quads_per_frame = l.quads_per_frame;
    p.stride = l.saddle_stride_bytes;
    p.d_saddles = static_cast<const uint8_t *>(l.d_saddles);
    p.d_counts = l.d_counts;
    p.d_frame_table = static_cast<const uint32_t *>(l.d_frame_table);
    p.d_point_status = l.d_point_status;
    p.d_quads = l.d_quads;
    p.d_n_quads = l.d_n_quads;
    p.d_status = l.d_status;
    p.d_quad_points = l.d_quad_points;
    p.d_seed_counts = d_seed_counts;
    p.seeds_per_frame = seeds_per_frame;
}

bool to_host(void *dst, const void *src, size_t bytes, hipStream_t stream)
{
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream) == hipSuccess;
}
bool to_device(void *dst, const void *src, size_t bytes, hipStream_t stream)
{
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream) == hipSuccess;
}

// What differs between the three fetches.  Per stage: its batch record (Pending), where its counters are (WHICH) and its name
// in messages; a handed-back frame's extra inputs and outputs on the host (Frame); and three pieces --
//   inputs_down(b, f, n_seeds, x, stream): the frame's extra inputs down (n_seeds: the frame's seeds by the batch's counts);
//   run(b, slots, stride, count, words, rows, x): its *_in_slots, on the pool;
//   outputs_up(b, f, status, x, stream): the extra outputs up, and when.  What it copies from lives in x.
struct FindStage {
    using Pending = FindPending;
    static constexpr int WHICH = LIST_FIND;
    static constexpr const char *NAME = "agx_find_boards_fetch";
    struct Frame {};
    static bool inputs_down(const Pending &, size_t, size_t, Frame &, hipStream_t) { return true; }
    static int run(const Pending &, const void *slots, size_t stride, uint32_t count, const uint32_t *words, std::vector<uint32_t> &rows, Frame &)
    {
        return find_board_in_slots(slots, stride, count, words, rows);
    }
    static bool outputs_up(const Pending &, size_t, uint32_t, const Frame &, hipStream_t) { return true; }
};

struct GrowStage {
    using Pending = GrowPending;
    static constexpr int WHICH = LIST_GROW;
    static constexpr const char *NAME = "agx_grow_boards_fetch";
    struct Frame {
        std::vector<uint32_t> seeds, scores;  // [4 * n_seeds]; the seeds' scores
        uint32_t best = 0;
    };
    static bool inputs_down(const Pending &b, size_t f, size_t n_seeds, Frame &x, hipStream_t stream)
    {
        x.seeds.resize(4 * n_seeds);
        return !n_seeds || to_host(x.seeds.data(), b.d_seed_quads + f * b.seeds_per_frame * 4, 4 * n_seeds * sizeof(uint32_t), stream);
    }
    static int run(const Pending &b, const void *slots, size_t stride, uint32_t count, const uint32_t *words, std::vector<uint32_t> &rows, Frame &x)
    {
        const int st = grow_boards_in_slots(slots, stride, count, words, x.seeds.data(), (uint32_t)(x.seeds.size() / 4), b.spacing_ratio,
                                            b.stop_score, b.flags, rows, x.scores, x.best);
        if (st != AGX_BOARD_FOUND) x.scores.clear();  // (written for frames that have a board only)
        return st;
    }
    static bool outputs_up(const Pending &b, size_t f, uint32_t status, const Frame &x, hipStream_t stream)
    {
        if (status != AGX_BOARD_FOUND && status != AGX_BOARD_CAPACITY) return true;
        return (!b.d_seed_scores || x.scores.empty() ||
                to_device(b.d_seed_scores + f * b.seeds_per_frame, x.scores.data(), x.scores.size() * sizeof(uint32_t), stream)) &&
               (!b.d_best_seed || to_device(b.d_best_seed + f, &x.best, sizeof(uint32_t), stream));
    }
};

struct InitStage {
    using Pending = InitPending;
    static constexpr int WHICH = LIST_INIT;
    static constexpr const char *NAME = "agx_init_quads_fetch";
    struct Frame {
        std::vector<uint32_t> seeds, counts, taken;  // the caller's seeds; the quads of each seed; the seeds taken
        uint32_t n_taken = 0;
    };
    static bool inputs_down(const Pending &b, size_t f, size_t n_seeds, Frame &x, hipStream_t stream)
    {
        if (!b.d_seed_saddles) return true;
        x.seeds.resize(n_seeds);
        return !n_seeds || to_host(x.seeds.data(), b.d_seed_saddles + f * b.seeds_per_frame, n_seeds * sizeof(uint32_t), stream);
    }
    static int run(const Pending &b, const void *slots, size_t stride, uint32_t count, const uint32_t *words, std::vector<uint32_t> &rows, Frame &x)
    {
        static const uint32_t no_seed = 0;  // (a non-null pointer for a frame without seeds: null asks for the reference's)
        const uint32_t *sd = b.d_seed_saddles ? (x.seeds.empty() ? &no_seed : x.seeds.data()) : nullptr;
        const int st = init_quads_in_slots(slots, stride, count, words, sd, (uint32_t)x.seeds.size(), b.seeds_per_frame, b.n_nearest, rows, x.counts,
                                           x.taken);
        x.n_taken = (uint32_t)x.taken.size();
        return st;
    }
    // (an AGX_BOARD_INPUT frame has neither counts nor seeds taken; its n_seeds_out is 0 like every frame's without a list)
    static bool outputs_up(const Pending &b, size_t f, uint32_t, const Frame &x, hipStream_t stream)
    {
        return (!b.d_seed_quad_counts || x.counts.empty() ||
                to_device(b.d_seed_quad_counts + f * b.seeds_per_frame, x.counts.data(), x.counts.size() * sizeof(uint32_t), stream)) &&
               (!b.d_seeds_out || x.taken.empty() ||
                to_device(b.d_seeds_out + f * b.seeds_per_frame, x.taken.data(), x.taken.size() * sizeof(uint32_t), stream)) &&
               (!b.d_n_seeds_out || to_device(b.d_n_seeds_out + f, &x.n_taken, sizeof(uint32_t), stream));
    }
};

// The fetch of any of the three, behind its own checks: the statuses down; for the frames the kernel handed back
// (AGX_BOARD_PENDING) their slots, status words and the stage's extra inputs down, the host form on the pool, the answers up --
// rows, corner points, count and status, and the stage's extra outputs.  The batch is resolved by this call, whatever it returns.
template <class Stage>
int resolve_handed_back(agx_detector *det, const typename Stage::Pending b, int n_threads)
{
    const std::string name = Stage::NAME;
    HIP_TRY(det, hipSetDevice(det->device));
    det->batch = BATCH_NONE;  // resolved by this call, whatever it returns
    det->last_list_frames[Stage::WHICH] = b.n_frames;
    det->last_list_handed_back[Stage::WHICH] = 0;
    if (n_threads <= 0) n_threads = agx_host_parallelism();
    hipStream_t stream = det->stream;
    const size_t n = (size_t)b.n_frames, qpf = b.quads_per_frame, spf = b.seeds_per_frame, stride = b.stride;
    try {
        std::vector<uint32_t> h_status(n), h_count(n, 0u);
        if (!to_host(h_status.data(), b.d_status, n * sizeof(uint32_t), stream) || hipStreamSynchronize(stream) != hipSuccess)
            return fail(det, AGX_ERR_HIP, name + ": copy / wait");
        std::vector<int> pending;
        for (size_t f = 0; f < n; ++f)
            if (h_status[f] == AGX_BOARD_PENDING) pending.push_back((int)f);
        det->last_list_handed_back[Stage::WHICH] = (int)pending.size();
        if (pending.empty()) return AGX_OK;
        WorkerPool *pool = worker_pool(det, n_threads);
        if (!pool) return fail(det, AGX_ERR_ARG, "n_threads");
        const size_t np = pending.size();
        std::vector<std::vector<uint8_t>> slots(np);
        std::vector<std::vector<uint32_t>> words(np), rows(np);
        std::vector<std::vector<float>> pts(np);
        std::vector<typename Stage::Frame> extra(np);
        // the frames' own slots (table entries or counts) and seed counts
        std::vector<uint32_t> own(b.d_frame_table ? 4 * n : (b.d_counts ? n : 0)), seed_counts(b.d_seed_counts ? n : 0);
        bool ok = own.empty() || to_host(own.data(), b.d_frame_table ? b.d_frame_table : b.d_counts, own.size() * sizeof(uint32_t), stream);
        if (ok && !seed_counts.empty()) ok = to_host(seed_counts.data(), b.d_seed_counts, n * sizeof(uint32_t), stream);
        if (!ok || hipStreamSynchronize(stream) != hipSuccess) return fail(det, AGX_ERR_HIP, name + ": the frames' counts");
        std::vector<char> no_list(np, 0);
        for (size_t k = 0; k < np && ok; ++k) {
            const size_t f = (size_t)pending[k];
            size_t first = f * b.saddles_per_frame, count = b.saddles_per_frame;
            if (b.d_frame_table) {
                count = own[4 * f];
                first = own[4 * f + 1];
                if (own[4 * f + 2] & 7u) {  // an overflow bit: there is no list (the kernel says so itself unless it read nothing)
                    no_list[k] = 1;
                    continue;
                }
            } else if (b.d_counts) {
                count = std::min<size_t>(own[f], b.saddles_per_frame);
            }
            ok = Stage::inputs_down(b, f, b.d_seed_counts ? std::min<size_t>(seed_counts[f], spf) : spf, extra[k], stream);
            if (!count) continue;
            slots[k].resize((count - 1) * stride + sizeof(agx_saddle));
            ok = ok && to_host(slots[k].data(), b.d_saddles + first * stride, slots[k].size(), stream);
            if (ok && b.d_point_status) {
                words[k].resize(count);
                ok = to_host(words[k].data(), b.d_point_status + first, count * sizeof(uint32_t), stream);
            }
        }
        if (!ok || hipStreamSynchronize(stream) != hipSuccess) return fail(det, AGX_ERR_HIP, name + ": the handed-back frames' lists");
        std::atomic<bool> nomem{false};
        const bool want_pts = b.d_quad_points != nullptr;
        try {
            for (size_t k = 0; k < np; ++k) {
                const size_t f = (size_t)pending[k];
                if (no_list[k]) {
                    h_status[f] = AGX_BOARD_INPUT;
                    continue;
                }
                pool->submit([&, k, f] {
                    try {
                        const uint32_t count = slots[k].empty() ? 0u : (uint32_t)((slots[k].size() - sizeof(agx_saddle)) / stride + 1);
                        const int st = Stage::run(b, slots[k].data(), stride, count, words[k].empty() ? nullptr : words[k].data(), rows[k], extra[k]);
                        const uint32_t nq = (uint32_t)(rows[k].size() / 4);
                        h_status[f] = (uint32_t)st;
                        if (st == AGX_BOARD_FOUND && nq > qpf) {
                            h_status[f] = AGX_BOARD_CAPACITY;
                            rows[k].clear();
                        }
                        h_count[f] = st == AGX_BOARD_FOUND ? nq : 0u;
                        if (want_pts)
                            for (uint32_t s : rows[k]) {
                                float xy[2];
                                std::memcpy(xy, slots[k].data() + (size_t)s * stride, sizeof xy);
                                pts[k].push_back(xy[0]);
                                pts[k].push_back(xy[1]);
                            }
                    } catch (...) {
                        nomem.store(true);
                    }
                });
            }
        } catch (...) {  // a task could not be queued: the ones that were read this call's vectors
            (void)pool->wait();
            throw;
        }
        if (!pool->wait() || nomem.load()) return fail(det, AGX_ERR_NOMEM, name + ": the host form");
        for (size_t k = 0; k < np && ok; ++k) {
            const size_t f = (size_t)pending[k];
            if (!rows[k].empty())
                ok = to_device(b.d_quads + f * qpf * 4, rows[k].data(), rows[k].size() * sizeof(uint32_t), stream) &&
                     (!want_pts || to_device(b.d_quad_points + f * qpf * 8, pts[k].data(), pts[k].size() * sizeof(float), stream));
            ok = ok && Stage::outputs_up(b, f, h_status[f], extra[k], stream) && to_device(b.d_n_quads + f, &h_count[f], sizeof(uint32_t), stream) &&
                 to_device(b.d_status + f, &h_status[f], sizeof(uint32_t), stream);
        }
        if (!ok || hipStreamSynchronize(stream) != hipSuccess) return fail(det, AGX_ERR_HIP, name + ": the host form's answers to the device");
    } catch (...) {
        return fail(det, AGX_ERR_NOMEM, name + ": host memory");
    }
    return AGX_OK;
}
}  // namespace

// ---- agx_find_boards_enqueue / _fetch: try_find_best_board (src/detector.rs:588-639) of caller-given saddle lists: k_find_boards ----
int agx::find_boards_enqueue_impl(agx_detector *det, const void *d_saddles, size_t saddle_stride_bytes, int n_frames, uint32_t saddles_per_frame,
                                  const uint32_t *d_counts, const void *d_frame_table, const uint32_t *d_point_status,
                                  uint32_t quads_per_frame, uint32_t *d_quads, float *d_quad_points, uint32_t *d_n_quads, uint32_t *d_status)
{
    if (!det) return AGX_ERR_ARG;
    ListArgs l{d_saddles, saddle_stride_bytes, n_frames, saddles_per_frame, d_counts, d_frame_table, d_point_status,
               quads_per_frame, d_quads, d_quad_points, d_n_quads, d_status};
    if (const int rc = check_list_args(det, l, nullptr, 0, [&] {
            if ((d_quads == nullptr) != (d_n_quads == nullptr) || (d_quads == nullptr) != (d_status == nullptr))
                return fail(det, AGX_ERR_ARG, "d_quads, d_n_quads and d_status: all or none");
            return (int)AGX_OK;
        }))
        return rc;
    bool host_only;
    if (const int rc = begin_list_batch(det, host_only)) return rc;
    int results = RESULTS_CALLER;
    if (!d_quads) {
        const size_t rows = (size_t)n_frames * quads_per_frame;
        l.d_quads = static_cast<uint32_t *>(side_ensure(det, SB_FIND_QUADS, rows * 4 * sizeof(uint32_t), 0));
        l.d_n_quads = static_cast<uint32_t *>(side_ensure(det, SB_FIND_COUNTS, (size_t)n_frames * sizeof(uint32_t), 0));
        l.d_status = static_cast<uint32_t *>(side_ensure(det, SB_FIND_STATUS, (size_t)n_frames * sizeof(uint32_t), 0));
        if (!d_quad_points) l.d_quad_points = static_cast<float *>(side_ensure(det, SB_FIND_POINTS, rows * 8 * sizeof(float), 0));
        if (!l.d_quads || !l.d_n_quads || !l.d_status || !l.d_quad_points) return fail(det, AGX_ERR_HIP, "hipMalloc: board quads");
        results = RESULTS_HOST;
    }
    FindBoardsArgs q{};
    fill_list_args(q, det, l, host_only);
    const hipError_t e = (hipError_t)launch_find_boards(q, det->stream);
    if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_find_boards: ") + hipGetErrorString(e));
    det->batch = BATCH_FIND;
    fill_list_pending(det->find, l, results, nullptr, 0);
    return AGX_OK;
}

int agx::find_boards_fetch_impl(agx_detector *det, uint32_t *quads, float *quad_points, uint32_t *n_quads, uint32_t *status, int n_threads)
{
    if (!det) return AGX_ERR_ARG;
    if (const int other = refuse_other_batch(det, BATCH_FIND)) return other;
    const FindPending b = det->find;
    if (b.results == RESULTS_HOST && (!quads || !n_quads || !status)) return fail(det, AGX_ERR_ARG, "null output");  // (the batch stays in flight)
    if (const int rc = resolve_handed_back<FindStage>(det, b, n_threads)) return rc;
    // the caller's host arrays (also where no frame was handed back): counts and statuses, and the rows below each frame's count
    if (!(quads || quad_points || n_quads || status)) return AGX_OK;
    if (quad_points && !b.d_quad_points) return fail(det, AGX_ERR_ARG, "quad_points: the batch was enqueued without d_quad_points");
    hipStream_t stream = det->stream;
    const size_t n = (size_t)b.n_frames, qpf = b.quads_per_frame;
    try {
        std::vector<uint32_t> h_status(n), h_count(n), h_quads(quads ? n * qpf * 4 : 0);
        std::vector<float> h_pts(quad_points ? n * qpf * 8 : 0);
        bool ok = to_host(h_count.data(), b.d_n_quads, n * sizeof(uint32_t), stream) && to_host(h_status.data(), b.d_status, n * sizeof(uint32_t), stream);
        if (ok && quads) ok = to_host(h_quads.data(), b.d_quads, h_quads.size() * sizeof(uint32_t), stream);
        if (ok && quad_points) ok = to_host(h_pts.data(), b.d_quad_points, h_pts.size() * sizeof(float), stream);
        if (!ok || hipStreamSynchronize(stream) != hipSuccess) return fail(det, AGX_ERR_HIP, "agx_find_boards_fetch: copy / wait");
        for (size_t f = 0; f < n; ++f) {
            if (n_quads) n_quads[f] = h_count[f];
            if (status) status[f] = h_status[f];
            if (h_status[f] != AGX_BOARD_FOUND || !h_count[f]) continue;
            const size_t nq = std::min<size_t>(h_count[f], qpf);
            if (quads) std::memcpy(quads + f * qpf * 4, h_quads.data() + f * qpf * 4, nq * 4 * sizeof(uint32_t));
            if (quad_points) std::memcpy(quad_points + f * qpf * 8, h_pts.data() + f * qpf * 8, nq * 8 * sizeof(float));
        }
    } catch (...) {
        return fail(det, AGX_ERR_NOMEM, "agx_find_boards_fetch: host memory");
    }
    return AGX_OK;
}

// ---- agx_grow_boards_enqueue / _fetch: boards from caller-given seed quads (src/board.rs:26-112) over the same lists: k_grow_boards ----
// Everything in the caller's device arrays.
int agx::grow_boards_enqueue_impl(agx_detector *det, const void *d_saddles, size_t saddle_stride_bytes, int n_frames, uint32_t saddles_per_frame,
                                  const uint32_t *d_counts, const void *d_frame_table, const uint32_t *d_point_status, const uint32_t *d_seed_quads,
                                  uint32_t seeds_per_frame, const uint32_t *d_seed_counts, float spacing_ratio, uint32_t stop_score, int flags,
                                  uint32_t quads_per_frame, uint32_t *d_quads, float *d_quad_points, uint32_t *d_n_quads, uint32_t *d_status,
                                  uint32_t *d_seed_scores, uint32_t *d_best_seed)
{
    if (!det) return AGX_ERR_ARG;
    const ListArgs l{d_saddles, saddle_stride_bytes, n_frames, saddles_per_frame, d_counts, d_frame_table, d_point_status,
                     quads_per_frame, d_quads, d_quad_points, d_n_quads, d_status};
    const uintptr_t own_ptrs = (uintptr_t)d_seed_quads | (uintptr_t)d_seed_counts | (uintptr_t)d_seed_scores | (uintptr_t)d_best_seed;
    if (const int rc = check_list_args(det, l, &seeds_per_frame, own_ptrs, [&] {
            if (!d_quads || !d_n_quads || !d_status || !d_seed_quads)
                return fail(det, AGX_ERR_ARG, "d_seed_quads, d_quads, d_n_quads and d_status are required");
            if (!std::isfinite(spacing_ratio) || !(1.0f + spacing_ratio > 0.0f))
                return fail(det, AGX_ERR_ARG, "spacing_ratio must be finite with 1 + spacing_ratio > 0");
            if (flags & ~AGX_GROW_FIX_MISSING) return fail(det, AGX_ERR_ARG, "flags: AGX_GROW_FIX_MISSING or 0");
            return (int)AGX_OK;
        }))
        return rc;
    bool host_only;
    if (const int rc = begin_list_batch(det, host_only)) return rc;
    GrowBoardsArgs q{};
    fill_list_args(q, det, l, host_only);
    q.seed_quads = d_seed_quads;
    q.seeds_per_frame = seeds_per_frame;
    q.seed_counts = d_seed_counts;
    q.spacing_ratio = spacing_ratio;
    q.stop_score = stop_score;
    q.flags = flags;
    q.seed_scores = d_seed_scores;
    q.best_seed = d_best_seed;
    const hipError_t e = (hipError_t)launch_grow_boards(q, det->stream);
    if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_grow_boards: ") + hipGetErrorString(e));
    det->batch = BATCH_GROW;
    GrowPending &p = det->grow;
    fill_list_pending(p, l, RESULTS_CALLER, d_seed_counts, seeds_per_frame);
    p.d_seed_quads = d_seed_quads;
    p.stop_score = stop_score;
    p.spacing_ratio = spacing_ratio;
    p.flags = flags;
    p.d_seed_scores = d_seed_scores;
    p.d_best_seed = d_best_seed;
    return AGX_OK;
}

int agx::grow_boards_fetch_impl(agx_detector *det, int n_threads)
{
    if (!det) return AGX_ERR_ARG;
    if (const int other = refuse_other_batch(det, BATCH_GROW)) return other;
    return resolve_handed_back<GrowStage>(det, det->grow, n_threads);
}

// ---- agx_init_quads_enqueue / _fetch: init_quads (src/detector.rs:543-586) of caller-given seed saddles over the same lists: k_init_quads ----
// Everything in the caller's device arrays.
int agx::init_quads_enqueue_impl(agx_detector *det, const void *d_saddles, size_t saddle_stride_bytes, int n_frames, uint32_t saddles_per_frame,
                                 const uint32_t *d_counts, const void *d_frame_table, const uint32_t *d_point_status, const uint32_t *d_seed_saddles,
                                 uint32_t seeds_per_frame, const uint32_t *d_seed_counts, uint32_t n_nearest, uint32_t quads_per_frame,
                                 uint32_t *d_quads, float *d_quad_points, uint32_t *d_n_quads, uint32_t *d_status, uint32_t *d_seed_quad_counts,
                                 uint32_t *d_seeds_out, uint32_t *d_n_seeds_out)
{
    if (!det) return AGX_ERR_ARG;
    const ListArgs l{d_saddles, saddle_stride_bytes, n_frames, saddles_per_frame, d_counts, d_frame_table, d_point_status,
                     quads_per_frame, d_quads, d_quad_points, d_n_quads, d_status};
    const uintptr_t own_ptrs = (uintptr_t)d_seed_saddles | (uintptr_t)d_seed_counts | (uintptr_t)d_seed_quad_counts | (uintptr_t)d_seeds_out |
                               (uintptr_t)d_n_seeds_out;
    if (const int rc = check_list_args(det, l, &seeds_per_frame, own_ptrs, [&] {
            if (!d_quads || !d_n_quads || !d_status) return fail(det, AGX_ERR_ARG, "d_quads, d_n_quads and d_status are required");
            if (d_seed_counts && !d_seed_saddles) return fail(det, AGX_ERR_ARG, "d_seed_counts without d_seed_saddles");
            if (n_nearest < 2 || n_nearest > 64) return fail(det, AGX_ERR_ARG, "n_nearest must be 2 .. 64");
            return (int)AGX_OK;
        }))
        return rc;
    bool host_only;
    if (const int rc = begin_list_batch(det, host_only)) return rc;
    InitQuadsArgs q{};
    fill_list_args(q, det, l, host_only);
    q.seed_saddles = d_seed_saddles;
    q.seeds_per_frame = seeds_per_frame;
    q.seed_counts = d_seed_counts;
    q.n_nearest = n_nearest;
    q.seed_quad_counts = d_seed_quad_counts;
    q.seeds_out = d_seeds_out;
    q.n_seeds_out = d_n_seeds_out;
    const hipError_t e = (hipError_t)launch_init_quads(q, det->stream);
    if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_init_quads: ") + hipGetErrorString(e));
    det->batch = BATCH_INIT;
    InitPending &p = det->init;
    fill_list_pending(p, l, RESULTS_CALLER, d_seed_counts, seeds_per_frame);
    p.d_seed_saddles = d_seed_saddles;
    p.n_nearest = n_nearest;
    p.d_seed_quad_counts = d_seed_quad_counts;
    p.d_seeds_out = d_seeds_out;
    p.d_n_seeds_out = d_n_seeds_out;
    return AGX_OK;
}

int agx::init_quads_fetch_impl(agx_detector *det, int n_threads)
{
    if (!det) return AGX_ERR_ARG;
    if (const int other = refuse_other_batch(det, BATCH_INIT)) return other;
    return resolve_handed_back<InitStage>(det, det->init, n_threads);
}

// ---- agx_snap_points_enqueue: caller points to the nearest listed saddle over the same lists: k_snap_points ----------------------
// Everything in the caller's device arrays; nothing is handed back, so there is no batch record and no fetch.
bool agx::snap_point_args_ok(size_t row_stride_bytes, size_t point_stride_bytes, uint32_t points_per_row, float max_dist_sq, int flags)
{
    if (points_per_row < 1 || points_per_row > 4) return false;
    if ((row_stride_bytes & 3) || (point_stride_bytes & 3) || point_stride_bytes < 8 || point_stride_bytes > 0x7fffffffu) return false;
    if (row_stride_bytes < (size_t)(points_per_row - 1) * point_stride_bytes + 8) return false;
    return max_dist_sq >= 0.0f && !(flags & ~AGX_SNAP_REVERSE);  // (a NaN fails the comparison)
}

int agx::snap_points_enqueue_impl(agx_detector *det, const void *d_saddles, size_t saddle_stride_bytes, int n_frames, uint32_t saddles_per_frame,
                                  const uint32_t *d_counts, const void *d_frame_table, const uint32_t *d_point_status, const void *d_points,
                                  size_t row_stride_bytes, size_t point_stride_bytes, uint32_t rows_per_frame, uint32_t points_per_row,
                                  const uint32_t *d_row_counts, float max_dist_sq, int flags, uint32_t *d_slots, float *d_dist_sq, uint32_t *d_rows,
                                  uint32_t *d_n_rows, uint32_t *d_row_index, uint32_t *d_status)
{
    if (!det) return AGX_ERR_ARG;
    // the lists' checks with the rows in the seeds' place (this stage has no quads: 1 passes that check)
    const ListArgs l{d_saddles, saddle_stride_bytes, n_frames, saddles_per_frame, d_counts, d_frame_table, d_point_status, 1u, nullptr, nullptr,
                     nullptr, nullptr};
    const uintptr_t own_ptrs = (uintptr_t)d_points | (uintptr_t)d_row_counts | (uintptr_t)d_slots | (uintptr_t)d_dist_sq | (uintptr_t)d_rows |
                               (uintptr_t)d_n_rows | (uintptr_t)d_row_index | (uintptr_t)d_status;
    if (const int rc = check_list_args(det, l, &rows_per_frame, own_ptrs, [&] {
            if (!d_points || !d_slots || !d_rows || !d_n_rows || !d_status)
                return fail(det, AGX_ERR_ARG, "d_points, d_slots, d_rows, d_n_rows and d_status are required");
            if (!snap_point_args_ok(row_stride_bytes, point_stride_bytes, points_per_row, max_dist_sq, flags))
                return fail(det, AGX_ERR_ARG, "points_per_row 1 .. 4, strides multiples of 4 that cover a point and a row, max_dist_sq >= 0, flags AGX_SNAP_REVERSE or 0");
            return (int)AGX_OK;
        }))
        return rc;
    HIP_TRY(det, hipSetDevice(det->device));
    begin_batch(det);  // and there is nothing of this one to be fetched
    SnapPointsArgs s{};
    s.saddles = static_cast<const uint8_t *>(d_saddles);
    s.stride = (uint32_t)saddle_stride_bytes;
    s.n_frames = n_frames;
    s.saddles_per_frame = saddles_per_frame;
    s.counts = d_counts;
    s.frame_table = static_cast<const uint32_t *>(d_frame_table);
    s.point_status = d_point_status;
    s.points = static_cast<const uint8_t *>(d_points);
    s.row_stride = row_stride_bytes;
    s.point_stride = (uint32_t)point_stride_bytes;
    s.rows_per_frame = rows_per_frame;
    s.points_per_row = points_per_row;
    s.row_counts = d_row_counts;
    s.max_dist_sq = max_dist_sq;
    s.flags = flags;
    s.slots = d_slots;
    s.dist_sq = d_dist_sq;
    s.rows = d_rows;
    s.n_rows = d_n_rows;
    s.row_index = d_row_index;
    s.status = d_status;
    const hipError_t e = (hipError_t)launch_snap_points(s, det->stream);
    if (e != hipSuccess) return fail(det, AGX_ERR_HIP, std::string("k_snap_points: ") + hipGetErrorString(e));
    return AGX_OK;
}

// The host tail of the frames `back` marks (1 handed back, 2 handed back as uncertain; without the device tail: every frame) of
// the batch `b` in flight on `det`, on the pool: from the chain's compact saddle lists and those frames' u8 luma, copied down
// from the device a group at a time.  `res` gets those frames' results (a list of the chain overflowed: reported, never truncated
// -- _enqueue_to: k_publish_tags has said so already), host_frames the frames whose tail ran here.  Every tail has finished when
// this returns, whatever it returns.
static int resolve_on_host(agx_detector *det, const DetectPending &b, const std::vector<char> &back, WorkerPool *pool, FrameResults &res,
                           std::vector<int> &host_frames, TailStats &stats)
{
    const int n = b.n_frames, W = b.width, H = b.height;
    const size_t plane = (size_t)W * (size_t)H;
    hipStream_t stream = det->stream;
    SlotRing ring;  // (two slots of luma)
    int rc = AGX_OK;
    try {
        do {
            if (std::none_of(back.begin(), back.end(), [](char c) { return c != 0; })) break;
            // the saddle lists of the frames handed back (and the status of frames whose chain overflowed)
            std::vector<uint32_t> ns((size_t)n), offs((size_t)n);
            std::vector<int> fst((size_t)n);
            const agx_saddle *records = nullptr;
            rc = fetch_compact(det, &records, ns.data(), offs.data(), fst.data());
            if (rc) break;
            take_host_frames(back.data(), fst.data(), 0, n, res, host_frames, b.device_tail ? &stats : nullptr);
            const int n_host = (int)host_frames.size();
            if (!n_host) break;
            // their u8 luma, copied down a group at a time into one of two pinned slots while the previous group's tails run
            const int G = std::min(n_host, std::max(8, std::min(32, 2 * pool->size())));
            const int n_slots = n_host > G ? 2 : 1;
            // (pinned, guarded like every side buffer; fetch_compact has waited for the stream, so side_ensure's own wait costs nothing)
            uint8_t *h_luma = static_cast<uint8_t *>(side_ensure(det, SB_FETCH_LUMA, (size_t)n_slots * (size_t)G * plane, 1));
            if (!h_luma) { rc = AGX_ERR_HIP; break; }
            for (int c0 = 0, ci = 0; c0 < n_host && !rc; c0 += G, ++ci) {
                const int nc = std::min(G, n_host - c0), r = ci % n_slots;
                ring.wait_free(r);
                uint8_t *slot = h_luma + (size_t)r * (size_t)G * plane;
                bool ok = true;
                for (int i = 0; i < nc && ok; ++i)
                    ok = hipMemcpy2DAsync(slot + (size_t)i * plane, (size_t)W, b.d_luma + (size_t)host_frames[(size_t)(c0 + i)] * b.luma_frame,
                                          b.luma_row, (size_t)W, (size_t)H, hipMemcpyDeviceToHost, stream) == hipSuccess;
                if (!ok || hipStreamSynchronize(stream) != hipSuccess) { rc = AGX_ERR_HIP; break; }
                ring.submit(*pool, r, nc, [&](int i) {
                    const int f = host_frames[(size_t)(c0 + i)];
                    return HostTail{&det->fam, det->params.max_num_of_boards, f, records + offs[(size_t)f], ns[(size_t)f], slot + (size_t)i * plane,
                                    (size_t)W, W, H, AGX_L8, &res, &ring, r};
                });
            }
        } while (false);
    } catch (...) {
        rc = AGX_ERR_NOMEM;
    }
    (void)pool->wait();  // every tail (they read the luma slots and the compact list, and write to res)
    if (!rc && res.out_of_memory()) rc = AGX_ERR_NOMEM;
    return rc;
}

int agx::detect_fetch_impl(agx_detector *det, agx_tag *out, uint32_t *counts, int *frame_status, int n_threads)
{
    const DetectPending b = det->detect;
    if ((b.results == RESULTS_HOST && !counts) || (out && b.cap && !counts)) return AGX_ERR_ARG;  // (the batch stays in flight)
    if (b.results == RESULTS_HOST && !out && b.cap) return AGX_ERR_ARG;
    det->batch = BATCH_SADDLES;  // resolved by this call, whatever happens below; fetch_compact reads the chain's results under it
    const int n = b.n_frames;
    const uint32_t cap = b.cap;
    const bool to_dev = b.results == RESULTS_CALLER;
    hipStream_t stream = det->stream;
    if (n_threads <= 0) n_threads = agx_host_parallelism();
    // every frame's result as the host knows it (the device arrays of _enqueue_to get the same) and (_enqueue_to) the host tail's
    // tag rows until they are copied to the caller's device arrays; the frames the host tail takes
    FrameResults res(out, cap, nullptr, nullptr);
    std::vector<int> host_frames;
    TailStats stats;
    int rc = AGX_OK;
    try {
        do {
            if (hipSetDevice(det->device) != hipSuccess) { rc = AGX_ERR_HIP; break; }
            WorkerPool *pool = worker_pool(det, n_threads);
            if (!pool) { rc = AGX_ERR_ARG; break; }
            res.hold(n, to_dev);
            std::vector<char> back((size_t)n, b.device_tail ? 0 : 1);  // 1 handed back, 2 handed back as uncertain
            if (b.device_tail) {
                const uint32_t *table = nullptr;
                const agx_tag *tags = nullptr;
                uint32_t tag_stride = 0;
                std::vector<uint32_t> dtab;
                if (to_dev) {  // the 16-byte table entry per frame, not the rows: those are in the caller's arrays already
                    dtab.resize((size_t)n * 4);
                    if (hipMemcpyAsync(dtab.data(), det->side[SB_DTABLE].payload, dtab.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
                        hipStreamSynchronize(stream) != hipSuccess) { rc = AGX_ERR_HIP; break; }
                    table = dtab.data();
                } else {
                    rc = fetch_tail(det, &tags, &table, &tag_stride);  // waits for the device
                    if (rc) break;
                }
                (void)read_tail_table(table, tags, tag_stride, 0, n, res, back.data());
            }
            rc = resolve_on_host(det, b, back, pool, res, host_frames, stats);
        } while (false);
    } catch (...) {
        rc = AGX_ERR_NOMEM;
    }
    const uint32_t *cnt = res.counts();
    const int *st = res.statuses();
    if (!rc && to_dev) {
        // the host tail's frames into the caller's device arrays, on the detector's stream: rows, count, status (all frames at once
        // where the host tail took every frame)
        bool ok = true;
        for (size_t k = 0; k < host_frames.size() && ok; ++k) {
            const int f = host_frames[k];
            if (st[(size_t)f] == AGX_OK && cnt[(size_t)f])
                ok = hipMemcpyAsync(b.d_tags + (size_t)f * cap, res.held_rows(f).data(), (size_t)cnt[(size_t)f] * sizeof(agx_tag),
                                    hipMemcpyHostToDevice, stream) == hipSuccess;
            if (ok && b.device_tail)
                ok = hipMemcpyAsync(b.d_counts + f, &cnt[(size_t)f], sizeof(uint32_t), hipMemcpyHostToDevice, stream) == hipSuccess &&
                     hipMemcpyAsync(b.d_status + f, &st[(size_t)f], sizeof(int), hipMemcpyHostToDevice, stream) == hipSuccess;
        }
        if (ok && !b.device_tail)
            ok = hipMemcpyAsync(b.d_counts, cnt, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, stream) == hipSuccess &&
                 hipMemcpyAsync(b.d_status, st, (size_t)n * sizeof(int), hipMemcpyHostToDevice, stream) == hipSuccess;
        // the caller's host arrays as well, if it passed any: the rows from the device arrays, counts and status as known here
        if (ok && out && cap)
            ok = hipMemcpyAsync(out, b.d_tags, (size_t)n * cap * sizeof(agx_tag), hipMemcpyDeviceToHost, stream) == hipSuccess;
        if (!ok || hipStreamSynchronize(stream) != hipSuccess) rc = AGX_ERR_HIP;
    }
    abandon_batch(det);  // (waits for the stream; nothing of the batch is left to be fetched)
    set_tail_stats(det, b.device_tail ? n : 0, stats.fallback, stats.uncertain);
    if (rc) {
        FrameResults::fail_all(rc, counts, frame_status, n);
        return rc;
    }
    return res.hand_over(counts, frame_status, n, nullptr);
}

// agx_group_detect_fetch, rank by rank: the group has read this rank's packed frame table; back[f] != 0 marks the frames the
// host tail takes (1, or 2: handed back as uncertain; without the device tail every frame).  Only THEIR rows (out + f * cap),
// counts and statuses are written: the other frames' are the group's, from the gathered table and slab.  Resolves the batch.
int agx::group_detect_fetch_impl(agx_detector *det, const char *back_in, agx_tag *out, uint32_t *counts, int *frame_status, int n_threads)
{
    const DetectPending b = det->detect;
    if (det->batch != BATCH_DETECT || b.results != RESULTS_GROUP) return AGX_ERR_STATE;  // (something else was enqueued on the borrowed detector since)
    det->batch = BATCH_SADDLES;  // (as detect_fetch_impl)
    const int n = b.n_frames;
    if (n_threads <= 0) n_threads = agx_host_parallelism();
    FrameResults res(out, b.cap, nullptr, nullptr);
    std::vector<int> host_frames;
    TailStats stats;
    int rc = AGX_OK;
    try {
        const std::vector<char> back(back_in, back_in + n);
        res.hold(n, false);
        if (std::any_of(back.begin(), back.end(), [](char c) { return c != 0; })) {
            WorkerPool *pool = hipSetDevice(det->device) == hipSuccess ? worker_pool(det, n_threads) : nullptr;
            rc = pool ? resolve_on_host(det, b, back, pool, res, host_frames, stats) : AGX_ERR_HIP;
        }
        if (!rc) (void)res.hand_over(counts, frame_status, n, back.data());  // (a frame's own status is not the rank's)
    } catch (...) {
        rc = AGX_ERR_NOMEM;
    }
    abandon_batch(det);
    set_tail_stats(det, b.device_tail ? n : 0, stats.fallback, stats.uncertain);
    return rc;
}
