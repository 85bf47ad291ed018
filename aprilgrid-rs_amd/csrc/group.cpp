// group.cpp -- several GPUs of one node driven from ONE process through the C ABI
// (include/aprilgrid_amd.h, "detector groups"): frame sharding and the result gather of
// SURVEY.md 8(e) without torch.  Frames are independent (reference: detect(&self) only reads
// immutable fields, src/detector.rs:17-23,505), so rank r runs the whole saddle chain for its own
// frames on its own device and stream; the one exchange step is the gather of the per-rank result
// slabs (frame table + packed saddle records; for detect, src/detector.rs:505-540: frame table + packed tag records -- the
// device tail's results through k_pack_tags, tail_kernels.hip) to the root device.
//
// Transports of the gather:
//   AGX_GATHER_RCCL   ncclSend / ncclRecv in one ncclGroup over xGMI, enqueued on the detectors'
//                     streams behind their chains.  librccl is opened with dlopen when a group of MORE
//                     THAN ONE rank is created, so a single-GPU host (a group of one, or a process that
//                     never builds a group) does not need it: a group of one moves its slabs with two
//                     device-to-device copies whatever the transport.  AGX_GROUP_RCCL_SELF=1 (environment,
//                     read at agx_group_create; a test switch) makes a group of one bind the library and
//                     send its slabs to itself through it -- what a one-GPU box can exercise of librccl.
//   AGX_GATHER_PEER   hipMemcpyPeerAsync on the producer's stream + an event the root stream waits
//                     on.  Same data path over xGMI, no communicator; also the only transport that
//                     accepts the same device twice (a test configuration for one-GPU boxes).
#include <hip/hip_runtime_api.h>

#include <dlfcn.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/aprilgrid_amd.h"
#include "detector_internal.h"
#include "tail_kernels.h"

namespace {

// The handful of RCCL entry points the gather needs (rccl.h is not included: the library is
// optional at run time and its handle types are opaque pointers).
struct Rccl {
    void *lib = nullptr;
    int (*CommInitAll)(void **comms, int ndev, const int *devlist) = nullptr;
    int (*CommDestroy)(void *comm) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void *buf, size_t count, int dtype, int peer, void *comm, hipStream_t st) = nullptr;
    int (*Recv)(void *buf, size_t count, int dtype, int peer, void *comm, hipStream_t st) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};
constexpr int kNcclUint8 = 1;  // ncclUint8 / ncclChar family: 0 = int8, 1 = uint8

// AGX_RCCL_LIBRARY (environment): the library to bind instead of librccl.  The test suite points it at a stand-in
// (tests/stub_rccl) that moves the bytes with peer copies, so that this file's RCCL branch runs on a one-GPU box --
// several ranks on one device, which the real library refuses.
const char *rccl_override()
{
    const char *p = getenv("AGX_RCCL_LIBRARY");
    return (p && *p) ? p : nullptr;
}

bool load_rccl(Rccl &r, std::string &err)
{
    if (r.lib) return true;
    if (const char *over = rccl_override()) {
        r.lib = dlopen(over, RTLD_NOW | RTLD_LOCAL);
    } else {
        // the soname first: a process that already holds an RCCL (e.g. the one bundled with PyTorch)
        // gets that copy back instead of a second runtime
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            r.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (r.lib) break;
        }
    }
    if (!r.lib) {
        const char *why = dlerror();  // (a second call would return NULL: the message is consumed by the first)
        err = std::string("dlopen librccl: ") + (why ? why : "not found");
        return false;
    }
    auto sym = [&](const char *n) { return dlsym(r.lib, n); };
    r.CommInitAll = (decltype(r.CommInitAll))sym("ncclCommInitAll");
    r.CommDestroy = (decltype(r.CommDestroy))sym("ncclCommDestroy");
    r.GroupStart = (decltype(r.GroupStart))sym("ncclGroupStart");
    r.GroupEnd = (decltype(r.GroupEnd))sym("ncclGroupEnd");
    r.Send = (decltype(r.Send))sym("ncclSend");
    r.Recv = (decltype(r.Recv))sym("ncclRecv");
    r.GetErrorString = (decltype(r.GetErrorString))sym("ncclGetErrorString");
    if (!r.CommInitAll || !r.CommDestroy || !r.GroupStart || !r.GroupEnd || !r.Send || !r.Recv) {
        err = "librccl lacks ncclCommInitAll / ncclSend / ncclRecv";
        dlclose(r.lib);
        r.lib = nullptr;
        return false;
    }
    return true;
}

}  // namespace

struct agx_group {
    int n = 0;
    int transport = AGX_GATHER_PEER;
    std::vector<int> devices;
    std::vector<agx_detector *> dets;
    Rccl rccl;
    std::vector<void *> comms;
    bool rccl_bound = false;  // the library is loaded and a communicator exists (n > 1, or n == 1 with AGX_GROUP_RCCL_SELF=1)
    // per rank, on its own device: result slabs of the last batch
    std::vector<float *> d_saddles;
    std::vector<uint32_t *> d_table;
    std::vector<hipEvent_t> done;  // PEER: rank r's copy to the root has been enqueued up to here
    // on the root device: every rank's slabs, rank-major
    float *d_all_saddles = nullptr;
    uint32_t *d_all_table = nullptr;
    // pinned host mirrors
    float *h_saddles = nullptr;
    uint32_t *h_table = nullptr;
    int frames_per_rank = 0;
    uint32_t slab_records = 0;  // records per rank slab
    size_t cap_frames = 0, cap_records = 0;
    // agx_group_detect_*: the same for tags.  Each buffer is the group's alone (allocated in ensure_tag_slabs, freed in
    // free_tag_slabs; the detectors get a rank's pair as the destination of ONE batch and keep no pointer past its fetch).
    std::vector<agx_tag *> d_tags;         // per rank, on its own device: the slab k_pack_tags fills ...
    std::vector<uint32_t *> d_tag_table;   // ... and the packed frame table [frames][4]: count, offset, status, flags
    uint8_t *d_all_tags = nullptr;         // root device: every rank's table, rank-major, then every rank's slab -- one allocation,
    uint8_t *h_tags = nullptr;             // ... so that ONE copy brings both into this pinned mirror
    uint32_t *h_handed_back = nullptr;     // pinned [frames][4], every entry "handed back": the table of a rank without the device tail
    size_t cap_tag_frames = 0, cap_tag_records = 0;
    uint32_t tag_cap = 0, tag_slab_records = 0;  // of the detect batch in flight: the caller's cap_per_frame, records per rank slab
    bool tag_slabs_sent = false;                 // the gather carried the slabs (some rank ran the device tail), not the tables only
    int pending = 0;  // the batch in flight: 0 none, 1 agx_group_saddles_enqueue's, 2 agx_group_detect_enqueue's
    std::string last_error;
};

namespace {

thread_local std::string g_group_error;

int gfail(agx_group *g, int status, const std::string &msg)
{
    if (g) g->last_error = msg;
    else g_group_error = msg;
    return status;
}

// nothing unwinds across the C boundary (see agx_guard in detector.cpp)
void set_group_error_noexcept(agx_group *g, const char *msg) noexcept;

template <typename F>
int agx_group_guard(agx_group *g, F &&body) noexcept
{
    try {
        return body();
    } catch (const std::bad_alloc &) {
        set_group_error_noexcept(g, "out of host memory");
        return AGX_ERR_NOMEM;
    } catch (const std::exception &e) {
        set_group_error_noexcept(g, e.what());
        return AGX_ERR_STATE;
    } catch (...) {
        set_group_error_noexcept(g, "unknown exception");
        return AGX_ERR_STATE;
    }
}

#define GHIP(g, expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return gfail((g), AGX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

void set_group_error_noexcept(agx_group *g, const char *msg) noexcept
{
    try {
        if (g) g->last_error = msg;
        else g_group_error = msg;
    } catch (...) {
    }
}

// The two kinds of slabs are freed and grown apart: a group that alternates saddle and detect batches keeps both.
void free_saddle_slabs(agx_group *g)
{
    for (int r = 0; r < g->n; ++r) {
        (void)hipSetDevice(g->devices[r]);
        if (r < (int)g->d_saddles.size() && g->d_saddles[r]) (void)hipFree(g->d_saddles[r]);
        if (r < (int)g->d_table.size() && g->d_table[r]) (void)hipFree(g->d_table[r]);
    }
    g->d_saddles.assign(g->n, nullptr);
    g->d_table.assign(g->n, nullptr);
    if (g->n) (void)hipSetDevice(g->devices[0]);
    if (g->d_all_saddles) (void)hipFree(g->d_all_saddles);
    if (g->d_all_table) (void)hipFree(g->d_all_table);
    if (g->h_saddles) (void)hipHostFree(g->h_saddles);
    if (g->h_table) (void)hipHostFree(g->h_table);
    g->d_all_saddles = nullptr;
    g->d_all_table = nullptr;
    g->h_saddles = nullptr;
    g->h_table = nullptr;
    g->cap_frames = g->cap_records = 0;
}

void free_tag_slabs(agx_group *g)
{
    for (int r = 0; r < g->n; ++r) {
        (void)hipSetDevice(g->devices[r]);
        if (r < (int)g->d_tags.size() && g->d_tags[r]) (void)hipFree(g->d_tags[r]);
        if (r < (int)g->d_tag_table.size() && g->d_tag_table[r]) (void)hipFree(g->d_tag_table[r]);
    }
    g->d_tags.assign(g->n, nullptr);
    g->d_tag_table.assign(g->n, nullptr);
    if (g->n) (void)hipSetDevice(g->devices[0]);
    if (g->d_all_tags) (void)hipFree(g->d_all_tags);
    if (g->h_tags) (void)hipHostFree(g->h_tags);
    if (g->h_handed_back) (void)hipHostFree(g->h_handed_back);
    g->d_all_tags = nullptr;
    g->h_tags = nullptr;
    g->h_handed_back = nullptr;
    g->cap_tag_frames = g->cap_tag_records = 0;
}

void free_slabs(agx_group *g)
{
    free_saddle_slabs(g);
    free_tag_slabs(g);
}

int ensure_slabs(agx_group *g, int frames_per_rank, uint32_t slab_records)
{
    if ((size_t)frames_per_rank <= g->cap_frames && slab_records <= g->cap_records) return AGX_OK;
    for (agx_detector *d : g->dets) (void)agx_detector_sync(d);
    free_saddle_slabs(g);
    const size_t F = (size_t)frames_per_rank, R = slab_records;
    for (int r = 0; r < g->n; ++r) {
        GHIP(g, hipSetDevice(g->devices[r]));
        GHIP(g, hipMalloc((void **)&g->d_saddles[r], std::max<size_t>(R, 1) * 5 * sizeof(float)));
        GHIP(g, hipMalloc((void **)&g->d_table[r], F * 4 * sizeof(uint32_t)));
    }
    GHIP(g, hipSetDevice(g->devices[0]));
    GHIP(g, hipMalloc((void **)&g->d_all_saddles, (size_t)g->n * std::max<size_t>(R, 1) * 5 * sizeof(float)));
    GHIP(g, hipMalloc((void **)&g->d_all_table, (size_t)g->n * F * 4 * sizeof(uint32_t)));
    GHIP(g, hipHostMalloc((void **)&g->h_saddles, (size_t)g->n * std::max<size_t>(R, 1) * 5 * sizeof(float), hipHostMallocDefault));
    GHIP(g, hipHostMalloc((void **)&g->h_table, (size_t)g->n * F * 4 * sizeof(uint32_t), hipHostMallocDefault));
    g->cap_frames = F;
    g->cap_records = R;
    return AGX_OK;
}

// the tag slabs, grown the same way
int ensure_tag_slabs(agx_group *g, int frames_per_rank, uint32_t slab_records)
{
    if ((size_t)frames_per_rank <= g->cap_tag_frames && slab_records <= g->cap_tag_records) return AGX_OK;
    for (agx_detector *d : g->dets) (void)agx_detector_sync(d);
    free_tag_slabs(g);
    const size_t F = (size_t)frames_per_rank, R = std::max<size_t>(slab_records, 1);
    const size_t tab_bytes = F * 4 * sizeof(uint32_t), slab_bytes = R * sizeof(agx_tag);
    for (int r = 0; r < g->n; ++r) {
        GHIP(g, hipSetDevice(g->devices[r]));
        GHIP(g, hipMalloc((void **)&g->d_tags[r], slab_bytes));
        GHIP(g, hipMalloc((void **)&g->d_tag_table[r], tab_bytes));
    }
    GHIP(g, hipSetDevice(g->devices[0]));
    GHIP(g, hipMalloc((void **)&g->d_all_tags, (size_t)g->n * (tab_bytes + slab_bytes)));
    GHIP(g, hipHostMalloc((void **)&g->h_tags, (size_t)g->n * (tab_bytes + slab_bytes), hipHostMallocDefault));
    GHIP(g, hipHostMalloc((void **)&g->h_handed_back, tab_bytes, hipHostMallocDefault));
    for (size_t f = 0; f < F; ++f) {
        uint32_t *e = g->h_handed_back + 4 * f;
        e[0] = e[1] = 0;
        e[2] = (uint32_t)AGX_ERR_STATE;
        e[3] = agx::PACK_HANDED_BACK;
    }
    g->cap_tag_frames = F;
    g->cap_tag_records = slab_records;
    return AGX_OK;
}

// One payload of a gather: rank r's `bytes` at src[r] on its own device -> dst + r * bytes on the root device (0 bytes: not sent)
struct Payload {
    std::vector<const void *> src;
    char *dst;
    size_t bytes;
};

// The one exchange step: every rank's payloads to the root device, stream-ordered behind what the ranks' streams hold.
int enqueue_gather(agx_group *g, const Payload *pl, int n_pl)
{
    auto rccl_error = [&](const char *what, int e) {
        return gfail(g, AGX_ERR_HIP, std::string(what) + (g->rccl.GetErrorString ? g->rccl.GetErrorString(e) : "error"));
    };
    hipStream_t root = g->dets[0]->stream;
    GHIP(g, hipSetDevice(g->devices[0]));
    if (g->n == 1 && g->rccl_bound) {
        // A group of one under AGX_GROUP_RCCL_SELF=1 (test switch): the root's own slabs take the library's path -- a send
        // to itself and the matching receive in one ncclGroup on the root's stream.  (What a one-GPU box can exercise of
        // the real librccl: the binding, the communicator, the datatype constant, the ordering behind the chain on a
        // non-blocking stream.)  Without the switch a group of one never touches the library: two copies, below.
        int e = g->rccl.GroupStart();
        for (int k = 0; k < n_pl && e == 0; ++k) {
            if (!pl[k].bytes) continue;
            e = g->rccl.Send(pl[k].src[0], pl[k].bytes, kNcclUint8, 0, g->comms[0], root);
            if (e == 0) e = g->rccl.Recv(pl[k].dst, pl[k].bytes, kNcclUint8, 0, g->comms[0], root);
        }
        const int e2 = g->rccl.GroupEnd();
        if (e != 0 || e2 != 0) return rccl_error("RCCL self gather: ", e ? e : e2);
        return AGX_OK;
    }
    for (int k = 0; k < n_pl; ++k)
        if (pl[k].bytes) GHIP(g, hipMemcpyAsync(pl[k].dst, pl[k].src[0], pl[k].bytes, hipMemcpyDeviceToDevice, root));
    if (g->n > 1 && g->rccl_bound) {
        int e = g->rccl.GroupStart();
        for (int r = 1; r < g->n && e == 0; ++r) {
            hipStream_t st = g->dets[r]->stream;
            for (int k = 0; k < n_pl && e == 0; ++k)
                if (pl[k].bytes) e = g->rccl.Send(pl[k].src[r], pl[k].bytes, kNcclUint8, 0, g->comms[r], st);
            for (int k = 0; k < n_pl && e == 0; ++k)
                if (pl[k].bytes) e = g->rccl.Recv(pl[k].dst + (size_t)r * pl[k].bytes, pl[k].bytes, kNcclUint8, r, g->comms[0], root);
        }
        const int e2 = g->rccl.GroupEnd();
        if (e != 0 || e2 != 0) return rccl_error("RCCL gather: ", e ? e : e2);
    } else {
        for (int r = 1; r < g->n; ++r) {
            hipStream_t st = g->dets[r]->stream;
            GHIP(g, hipSetDevice(g->devices[r]));
            for (int k = 0; k < n_pl; ++k)
                if (pl[k].bytes)
                    GHIP(g, hipMemcpyPeerAsync(pl[k].dst + (size_t)r * pl[k].bytes, g->devices[0], pl[k].src[r], g->devices[r], pl[k].bytes, st));
            GHIP(g, hipEventRecord(g->done[r], st));
            GHIP(g, hipSetDevice(g->devices[0]));
            GHIP(g, hipStreamWaitEvent(root, g->done[r], 0));
        }
    }
    return AGX_OK;
}

// a detect batch that will not be fetched (an error after some ranks were enqueued): no detector keeps a batch only the group
// could resolve
void drop_detect_batch(agx_group *g)
{
    for (agx_detector *d : g->dets)
        if (d->batch == agx::BATCH_DETECT && d->detect.results == agx::RESULTS_GROUP) agx::abandon_batch(d);
    g->pending = 0;
}

}  // namespace

extern "C" {

const char *agx_group_last_error(const agx_group *g) { return g ? g->last_error.c_str() : g_group_error.c_str(); }

int agx_group_create(int family, const agx_params *params, const int *devices, int n_devices, int transport,
                     agx_group **out)
{
    return agx_group_guard(nullptr, [&]() -> int {
    if (!out) return AGX_ERR_ARG;
    *out = nullptr;
    if (n_devices < 1 || n_devices > 64) return gfail(nullptr, AGX_ERR_ARG, "n_devices must be 1..64");
    if (transport != AGX_GATHER_RCCL && transport != AGX_GATHER_PEER) return gfail(nullptr, AGX_ERR_ARG, "unknown gather transport");
    std::unique_ptr<agx_group> g(new agx_group());
    g->n = n_devices;
    g->transport = transport;
    for (int r = 0; r < n_devices; ++r) g->devices.push_back(devices ? devices[r] : r);
    const char *self_env = getenv("AGX_GROUP_RCCL_SELF");
    const bool use_rccl = transport == AGX_GATHER_RCCL && (n_devices > 1 || (self_env && self_env[0] == '1'));
    if (use_rccl) {
        // the library first: only the test suite's stand-in (it exports stub_rccl_stats) may take several ranks on one
        // device -- the real ncclCommInitAll would hang on them, whatever AGX_RCCL_LIBRARY says
        std::string err;
        if (!load_rccl(g->rccl, err)) return gfail(nullptr, AGX_ERR_HIP, err);
        const bool stand_in = dlsym(g->rccl.lib, "stub_rccl_stats") != nullptr;
        if (!stand_in)
            for (int r = 0; r < n_devices; ++r)
                for (int q = 0; q < r; ++q)
                    if (g->devices[q] == g->devices[r])
                        return gfail(nullptr, AGX_ERR_ARG, "the RCCL transport needs distinct devices (use AGX_GATHER_PEER to test on one GPU)");
    }
    g->d_saddles.assign(n_devices, nullptr);
    g->d_table.assign(n_devices, nullptr);
    g->d_tags.assign(n_devices, nullptr);
    g->d_tag_table.assign(n_devices, nullptr);
    auto cleanup = [&]() {
        for (agx_detector *d : g->dets) agx_detector_destroy(d);
        for (hipEvent_t e : g->done) (void)hipEventDestroy(e);
    };
    for (int r = 0; r < n_devices; ++r) {
        agx_detector *d = nullptr;
        const int st = agx_detector_create(family, params, g->devices[r], &d);
        if (st != AGX_OK) {
            g_group_error = std::string("rank ") + std::to_string(r) + ": " + agx_last_error(nullptr);
            cleanup();
            return st;
        }
        g->dets.push_back(d);
        hipEvent_t e = nullptr;
        if (hipSetDevice(g->devices[r]) != hipSuccess || hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
            cleanup();
            return gfail(nullptr, AGX_ERR_HIP, "hipEventCreate");
        }
        g->done.push_back(e);
    }
    if (transport == AGX_GATHER_PEER) {
        // direct xGMI access root <- rank (already-enabled is fine)
        for (int r = 1; r < n_devices; ++r)
            if (g->devices[r] != g->devices[0]) {
                (void)hipSetDevice(g->devices[r]);
                (void)hipDeviceEnablePeerAccess(g->devices[0], 0);
                (void)hipSetDevice(g->devices[0]);
                (void)hipDeviceEnablePeerAccess(g->devices[r], 0);
            }
        (void)hipGetLastError();
    } else if (use_rccl) {  // (one rank only with AGX_GROUP_RCCL_SELF=1: its slabs then go through the library as a send to itself)
        g->comms.assign(n_devices, nullptr);
        const int rc = g->rccl.CommInitAll(g->comms.data(), n_devices, g->devices.data());
        if (rc != 0) {
            cleanup();
            return gfail(nullptr, AGX_ERR_HIP, std::string("ncclCommInitAll: ") + (g->rccl.GetErrorString ? g->rccl.GetErrorString(rc) : "error"));
        }
        g->rccl_bound = true;
    }
    *out = g.release();
    return AGX_OK;
    });
}

void agx_group_destroy(agx_group *g)
{
    if (!g) return;
    try {
    for (agx_detector *d : g->dets) (void)agx_detector_sync(d);
    free_slabs(g);
    for (size_t r = 0; r < g->comms.size(); ++r)
        if (g->comms[r]) (void)g->rccl.CommDestroy(g->comms[r]);
    for (hipEvent_t e : g->done) (void)hipEventDestroy(e);
    for (agx_detector *d : g->dets) agx_detector_destroy(d);
    } catch (...) {
    }
    delete g;
}

int agx_group_size(const agx_group *g) { return g ? g->n : 0; }

agx_detector *agx_group_detector(agx_group *g, int rank) { return (g && rank >= 0 && rank < g->n) ? g->dets[rank] : nullptr; }

int agx_group_saddles_enqueue(agx_group *g, const void *const *d_frames, int frames_per_rank, int width, int height,
                              size_t row_stride_bytes, size_t frame_stride_bytes, int format, uint32_t records_per_frame)
{
    return agx_group_guard(g, [&]() -> int {
    if (!g || !d_frames || frames_per_rank <= 0) return gfail(g, AGX_ERR_ARG, "null frames or frames_per_rank <= 0");
    if (!records_per_frame) records_per_frame = 512;
    const unsigned long long slab64 = (unsigned long long)frames_per_rank * records_per_frame;
    if (slab64 > 0x7fffffffull) return gfail(g, AGX_ERR_ARG, "result slab too large");
    const uint32_t slab = (uint32_t)slab64;
    int rc = ensure_slabs(g, frames_per_rank, slab);
    if (rc) return rc;
    g->frames_per_rank = frames_per_rank;
    g->slab_records = slab;
    const size_t sad_bytes = (size_t)slab * 5 * sizeof(float), tab_bytes = (size_t)frames_per_rank * 4 * sizeof(uint32_t);
    // every rank's chain on its own device and stream, results in its own slabs
    for (int r = 0; r < g->n; ++r) {
        if (!d_frames[r]) return gfail(g, AGX_ERR_ARG, "null frame pointer for rank " + std::to_string(r));
        rc = agx_saddles_batch_enqueue_to(g->dets[r], d_frames[r], frames_per_rank, width, height, row_stride_bytes,
                                          frame_stride_bytes, format, g->d_saddles[r], slab, g->d_table[r]);
        if (rc) return gfail(g, rc, std::string("rank ") + std::to_string(r) + ": " + agx_last_error(g->dets[r]));
    }
    // the one exchange step: gather the slabs on the root device, stream-ordered behind the chains
    g->pending = 0;
    Payload pl[2] = {{{}, (char *)g->d_all_table, tab_bytes}, {{}, (char *)g->d_all_saddles, sad_bytes}};
    pl[0].src.assign(g->d_table.begin(), g->d_table.end());
    pl[1].src.assign(g->d_saddles.begin(), g->d_saddles.end());
    rc = enqueue_gather(g, pl, 2);
    if (rc) return rc;
    g->pending = 1;
    return AGX_OK;
    });
}

int agx_group_saddles_fetch(agx_group *g, agx_saddle *out, uint32_t cap_per_frame, uint32_t *counts, int *frame_status)
{
    return agx_group_guard(g, [&]() -> int {
    if (!g || !counts || (!out && cap_per_frame)) return gfail(g, AGX_ERR_ARG, "null output");
    if (g->pending == 2) return gfail(g, AGX_ERR_STATE, "the batch in flight is agx_group_detect_enqueue's: fetch it with agx_group_detect_fetch");
    if (!g->pending) return gfail(g, AGX_ERR_STATE, "no batch enqueued");
    const size_t F = (size_t)g->frames_per_rank;
    const size_t sad_bytes = (size_t)g->slab_records * 5 * sizeof(float), tab_bytes = F * 4 * sizeof(uint32_t);
    hipStream_t root = g->dets[0]->stream;
    GHIP(g, hipSetDevice(g->devices[0]));
    GHIP(g, hipMemcpyAsync(g->h_table, g->d_all_table, (size_t)g->n * tab_bytes, hipMemcpyDeviceToHost, root));
    GHIP(g, hipMemcpyAsync(g->h_saddles, g->d_all_saddles, (size_t)g->n * sad_bytes, hipMemcpyDeviceToHost, root));
    GHIP(g, hipStreamSynchronize(root));
    for (int r = 1; r < g->n; ++r) {  // the senders' streams have nothing left either
        const int rc = agx_detector_sync(g->dets[r]);
        if (rc) return gfail(g, rc, agx_last_error(g->dets[r]));
    }
    int first_bad = AGX_OK;
    for (int r = 0; r < g->n; ++r) {
        const uint32_t *tab = g->h_table + (size_t)r * F * 4;
        const float *sad = g->h_saddles + (size_t)r * g->slab_records * 5;
        for (size_t f = 0; f < F; ++f) {
            const size_t gf = (size_t)r * F + f;  // global frame index: rank-major, as the frames were sharded
            const uint32_t cnt = tab[f * 4 + 0], off = tab[f * 4 + 1], status = tab[f * 4 + 2];
            int st = AGX_OK;
            if ((status & (AGX_FRAME_CANDIDATE_OVERFLOW | AGX_FRAME_CLUSTER_OVERFLOW | AGX_FRAME_SADDLE_OVERFLOW)) || cnt > cap_per_frame ||
                (unsigned long long)off + cnt > g->slab_records)
                st = AGX_ERR_CAPACITY;
            // as agx_saddles_batch_fetch: a list that is merely longer than the caller's room reports its
            // length (so the caller can size a retry); a frame whose device-side lists overflowed reports 0
            const bool device_overflow = (status & (AGX_FRAME_CANDIDATE_OVERFLOW | AGX_FRAME_CLUSTER_OVERFLOW | AGX_FRAME_SADDLE_OVERFLOW)) ||
                                         (unsigned long long)off + cnt > g->slab_records;
            counts[gf] = device_overflow ? 0 : cnt;
            if (frame_status) frame_status[gf] = st;
            if (st != AGX_OK) {
                if (first_bad == AGX_OK) {
                    first_bad = st;
                    char buf[160];
                    std::snprintf(buf, sizeof buf, "rank %d frame %zu: capacity exceeded (status 0x%x, %u saddles)", r, f, status, cnt);
                    g->last_error = buf;
                }
                continue;
            }
            std::memcpy(out + gf * (size_t)cap_per_frame, sad + (size_t)off * 5, (size_t)cnt * sizeof(agx_saddle));
        }
    }
    return first_bad;
    });
}

int agx_group_detect_enqueue(agx_group *g, const void *const *d_frames, int frames_per_rank, int width, int height,
                             size_t row_stride_bytes, size_t frame_stride_bytes, int format, uint32_t cap_per_frame,
                             uint32_t tags_per_frame)
{
    return agx_group_guard(g, [&]() -> int {
    if (!g || !d_frames || frames_per_rank <= 0) return gfail(g, AGX_ERR_ARG, "null frames or frames_per_rank <= 0");
    for (int r = 0; r < g->n; ++r)
        if (!d_frames[r]) return gfail(g, AGX_ERR_ARG, "null frame pointer for rank " + std::to_string(r));
    if (frames_per_rank > 65535) return gfail(g, AGX_ERR_ARG, "at most 65535 frames per rank and batch");
    if (!agx::format_px_bytes(format) || format == AGX_LF32)
        return gfail(g, AGX_ERR_FORMAT, "format must be an integer agx_format (AGX_LF32: agx_detect_planes)");
    if (!tags_per_frame) tags_per_frame = 128;
    const unsigned long long slab64 = (unsigned long long)frames_per_rank * tags_per_frame;
    if (slab64 > 0x7fffffffull / sizeof(agx_tag)) return gfail(g, AGX_ERR_ARG, "tag slab too large");
    const uint32_t slab = (uint32_t)slab64;
    int rc = ensure_tag_slabs(g, frames_per_rank, slab);
    if (rc) return rc;
    g->pending = 0;  // (this batch replaces whatever was in flight)
    g->frames_per_rank = frames_per_rank;
    g->tag_cap = cap_per_frame;
    g->tag_slab_records = slab;
    const size_t tab_bytes = (size_t)frames_per_rank * 4 * sizeof(uint32_t), slab_bytes = (size_t)slab * sizeof(agx_tag);
    rc = [&]() -> int {
        // every rank's chain, to_luma8, device tail and k_pack_tags on its own device and stream, results in its own table + slab
        bool any_packed = false;
        for (int r = 0; r < g->n; ++r) {
            agx_detector *d = g->dets[r];
            const int e = agx::group_detect_enqueue(d, d_frames[r], frames_per_rank, width, height, row_stride_bytes, frame_stride_bytes,
                                                    format, cap_per_frame, g->d_tag_table[r], g->d_tags[r], slab);
            if (e) return gfail(g, e, std::string("rank ") + std::to_string(r) + ": " + agx_last_error(d));
            if (d->detect.device_tail) any_packed = true;
            else  // the host tail takes every frame of this rank (option "device_tail" 0, or refused): no pack kernel, a fill
                GHIP(g, hipMemcpyAsync(g->d_tag_table[r], g->h_handed_back, tab_bytes, hipMemcpyHostToDevice, d->stream));
        }
        // the one exchange step; where no rank has packed anything it carries the tables only
        g->tag_slabs_sent = any_packed;
        Payload pl[2] = {{{}, (char *)g->d_all_tags, tab_bytes}, {{}, (char *)g->d_all_tags + (size_t)g->n * tab_bytes, any_packed ? slab_bytes : 0}};
        pl[0].src.assign(g->d_tag_table.begin(), g->d_tag_table.end());
        pl[1].src.assign(g->d_tags.begin(), g->d_tags.end());
        return enqueue_gather(g, pl, 2);
    }();
    if (rc) {
        drop_detect_batch(g);
        return rc;
    }
    g->pending = 2;
    return AGX_OK;
    });
}

int agx_group_detect_fetch(agx_group *g, agx_tag *out, uint32_t *counts, int *frame_status, int n_threads)
{
    return agx_group_guard(g, [&]() -> int {
    if (!g || !counts) return gfail(g, AGX_ERR_ARG, "null group or counts");
    if (g->pending == 1) return gfail(g, AGX_ERR_STATE, "the batch in flight is agx_group_saddles_enqueue's: fetch it with agx_group_saddles_fetch");
    if (g->pending != 2) return gfail(g, AGX_ERR_STATE, "no agx_group_detect_enqueue batch in flight");
    if (!out && g->tag_cap) return gfail(g, AGX_ERR_ARG, "null output");  // (the cap of THIS batch; it stays in flight)
    const size_t F = (size_t)g->frames_per_rank, N = (size_t)g->n * F;
    const uint32_t cap = g->tag_cap, slab = g->tag_slab_records;
    const size_t tab_bytes = F * 4 * sizeof(uint32_t), slab_bytes = (size_t)slab * sizeof(agx_tag);
    g->last_error.clear();
    std::vector<int> st(N, AGX_OK);
    std::vector<char> back(F);
    int rc = [&]() -> int {
        // one copy: the gathered tables and, where any rank packed tags, the slabs behind them
        hipStream_t root = g->dets[0]->stream;
        GHIP(g, hipSetDevice(g->devices[0]));
        GHIP(g, hipMemcpyAsync(g->h_tags, g->d_all_tags, (size_t)g->n * (tab_bytes + (g->tag_slabs_sent ? slab_bytes : 0)), hipMemcpyDeviceToHost, root));
        GHIP(g, hipStreamSynchronize(root));
        for (int r = 1; r < g->n; ++r) {  // the senders' streams have nothing left either
            const int e = agx_detector_sync(g->dets[r]);
            if (e) return gfail(g, e, agx_last_error(g->dets[r]));
        }
        for (int r = 0; r < g->n; ++r) {
            const uint32_t *tab = reinterpret_cast<const uint32_t *>(g->h_tags + (size_t)r * tab_bytes);
            const agx_tag *rows = reinterpret_cast<const agx_tag *>(g->h_tags + (size_t)g->n * tab_bytes + (size_t)r * slab_bytes);
            for (size_t f = 0; f < F; ++f) {
                const size_t gf = (size_t)r * F + f;  // global frame index: rank-major, as the frames were sharded
                const uint32_t cnt = tab[f * 4 + 0], off = tab[f * 4 + 1], flags = tab[f * 4 + 3];
                const int status = (int)tab[f * 4 + 2];
                back[f] = (flags & agx::PACK_HANDED_BACK) ? ((flags & agx::PACK_UNCERTAIN) ? 2 : 1) : 0;
                if (back[f]) continue;  // the host tail's, below
                counts[gf] = cnt;
                st[gf] = status;
                if (status == AGX_OK) {
                    if (cnt > cap || (unsigned long long)off + cnt > slab || !g->tag_slabs_sent)
                        return gfail(g, AGX_ERR_HIP, "rank " + std::to_string(r) + " frame " + std::to_string(f) + ": packed frame table out of range");
                    if (cnt) std::memcpy(out + gf * (size_t)cap, rows + off, (size_t)cnt * sizeof(agx_tag));
                } else if ((flags & agx::PACK_SLAB_FULL) && g->last_error.empty()) {
                    char buf[200];
                    std::snprintf(buf, sizeof buf, "rank %d frame %zu: the rank's tag slab is full (%u records; this frame has %u tags from record %u): a larger tags_per_frame is needed",
                                  r, f, slab, cnt, off);
                    g->last_error = buf;
                }
            }
            // the frames the device tail handed back (without it: every frame) on this rank's own device data
            const int e = agx::group_detect_fetch(g->dets[r], back.data(), out ? out + (size_t)r * F * cap : nullptr, counts + (size_t)r * F,
                                                  st.data() + (size_t)r * F, n_threads);
            if (e) return gfail(g, e, std::string("rank ") + std::to_string(r) + ": " + agx_last_error(g->dets[r]));
        }
        return AGX_OK;
    }();
    drop_detect_batch(g);  // resolved by this call, whatever happened (a rank not reached after a failure included)
    if (rc) {  // the call failed as a whole: no frame's result is valid (as agx_detect_batch)
        for (size_t i = 0; i < N; ++i) {
            counts[i] = 0;
            if (frame_status) frame_status[i] = rc;
        }
        return rc;
    }
    int first_bad = AGX_OK;
    std::string slab_msg;
    slab_msg.swap(g->last_error);
    for (size_t i = 0; i < N; ++i) {
        if (frame_status) frame_status[i] = st[i];
        if (st[i] != AGX_OK && first_bad == AGX_OK) {
            first_bad = st[i];
            char buf[160];
            std::snprintf(buf, sizeof buf, "rank %zu frame %zu: capacity exceeded (%u tags, room for %u per frame)", i / F, i % F, counts[i], cap);
            g->last_error = buf;
        }
    }
    if (!slab_msg.empty()) g->last_error = slab_msg;  // (the one a retry can act on: it names the rank, the frame and the slab)
    return first_bad;
    });
}

}  // extern "C"
