// abi_internal.hpp -- what the C ABI's translation units (abi_*.cpp) share:
// the context, device and slot structs, the error and buffer helpers, slot
// acquisition and the wait helpers.  Everything is in nice::abi, which has
// hidden visibility: none of it reaches the library's dynamic symbol table.
//
// The C ABI (include/nice_hip.h) replaces the reference's CUDA host pipeline
// (common/src/client_process_gpu.rs): no NVRTC (kernels are AOT code objects),
// one HIP stream per device, fields sharded across devices as contiguous
// n-ranges, histograms summed and near-miss / nice lists merged on the host,
// the MSD recursion on the device (or a multi-threaded host producer streaming
// range descriptors).
//
// Fields are processed asynchronously: every device owns kSlots result slots
// per mode (device state block, mapped result words, output lists, events), so
// a caller can submit field i+1 before collecting field i and the GPU never
// waits for the host between fields (nice_*_submit / nice_*_collect).  The
// synchronous reference-shaped entry points are submit + collect.
//
//   abi_context.cpp    context and device / slot lifetime, errors, queries
//   abi_detailed.cpp   detailed fields: enqueue, wait, gather + self-check
//   abi_niceonly.cpp   niceonly fields: device MSD or host MSD producer
//   abi_ranges.cpp     batched detailed ranges
//   abi_ranges_niceonly.cpp  batched niceonly ranges
//   abi_map.cpp        the per-number unique-count map
//   abi_msd_ranges.cpp the device MSD recursion's range list
//   abi_hooks.cpp      debug and check hooks
//   host_parallel.cpp  host thread count and the adaptive MSD floor (no HIP)
#pragma once

#include <hip/hip_runtime.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/nice_hip.h"
#include "host_math.hpp"
#include "host_parallel.hpp"
#include "kernels.h"
#include "probe.hpp"

namespace nice {
namespace abi __attribute__((visibility("hidden"))) {

// Per-slot state block: kHistCopies histograms of kHistBins u64 bins (kernels
// spread their end-of-launch atomics over the copies: hundreds of workgroups
// adding to ONE address serialise in L2), then the detailed list count and
// the fd2 finish's arrival counters.
constexpr size_t kStateBytes = (size_t)kHistCopies * kHistBins * 8 + (1 + kDoneWords) * 4;
constexpr int kSlots = 3;  // fields in flight per mode and context

constexpr uint32_t kInitialListCap = 1u << 20;  // NEAR_MISS_CAPACITY (client_process_gpu.rs:74)
constexpr uint32_t kNiceCap = 1u << 16;         // NICE_OUT_CAPACITY (:71)

// Slots a context rotates through (probe build: NICE_SLOTS limits it, for
// pipeline-depth experiments).
inline int slots_used() { return std::max(1, std::min(kSlots, (int)probe_knob("NICE_SLOTS", kSlots))); }

// Sets the calling thread's nice_last_error() message; returns code.
int fail(int code, const std::string &msg);

#define HIPCHK(expr)                                                                    \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return fail(NICE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

inline u128 mk(uint64_t lo, uint64_t hi) { return ((u128)hi << 64) | lo; }
inline uint64_t lo64(u128 v) { return (uint64_t)v; }
inline uint64_t hi64(u128 v) { return (uint64_t)(v >> 64); }

struct LeafBuf {
    // host pinned staging + device copy of one launch's leaf descriptors
    Leaf *h = nullptr, *d = nullptr;
    uint32_t cap = 0;
    hipEvent_t done = nullptr;
    bool pending = false;
};

struct MsdBuf {
    // device MSD: ping-pong level queues (or the fused kernel's per-workgroup
    // queues), leaf list, counters (layout.h).
    MsdNode *q[2] = {nullptr, nullptr};
    ChunkNode *scratch = nullptr;
    void *wscratch = nullptr;  // msd_wave_kernel work stacks
    size_t wscratch_bytes = 0;
    Leaf *leaves = nullptr;
    LeafMask *leaf_masks = nullptr;  // sound filter: parallel to leaves (allocated on first use)
    uint32_t *counters = nullptr;    // kMsdCounterWords
    uint32_t q_cap = 0, leaf_cap = 0, mask_cap = 0;
    uint64_t scratch_nodes = 0;
    // counters / nice count not known to be zero (first use, or a field that
    // did not end in the candidate kernel's epilogue)
    bool dirty = true;
};

struct ListBuf {
    uint64_t *n = nullptr;  // (lo, hi) pairs
    uint32_t *u = nullptr;  // num_uniques (detailed only)
    uint32_t cap = 0;
};

// One field in flight on one device: its own stream (consecutive fields run
// on alternate streams, so field i+1's first workgroups fill the CUs that
// field i's last ones leave idle), state block, results and MSD buffers.
struct Slot {
    hipStream_t stream = nullptr;   // detailed
    bool own_stream = false, own_nstream = false;  // false: shared with slot 0 (shared_streams)
    hipStream_t nstream = nullptr;  // niceonly: high priority, so its chain of short,
                                    // dependent MSD launches is not queued behind the
                                    // detailed kernels' workgroups
    uint64_t *d_state = nullptr;  // kHistCopies x kHistBins bins, then d_count
    uint32_t *d_count = nullptr;  // detailed list count
    uint32_t *d_done = nullptr;   // workgroups retired (fd2's in-kernel finish)
    uint32_t *d_nice_count = nullptr;  // niceonly list count
    uint64_t *h_fin = nullptr;    // mapped pinned: the kFinWords detailed result words (layout.h)
    uint64_t *d_fin = nullptr;    // device view of h_fin
    ListBuf det, nice;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_done = nullptr, nice_done = nullptr;
    hipEvent_t nt0 = nullptr, nt1 = nullptr;  // niceonly field span on the GPU (adaptive floor)
    uint32_t *h_msd = nullptr;    // mapped: MSD counters at the end of a niceonly field
    uint32_t *h_nice = nullptr;   // mapped: niceonly list count
    uint32_t *d_msd_mapped = nullptr, *d_nice_mapped = nullptr;  // device views
    uint32_t *d_nice_done = nullptr;  // workgroups retired (niceonly in-kernel finish)
    bool dirty = true;            // state block not known to be zero
    bool inflight = false;        // a detailed field enqueued and not yet gathered
    bool timed = false;           // the detailed field records ev0 / ev1 (kernel timing)
    bool marked = false;          // ... or an untimed end marker (ev_done) on a shared stream
    uint64_t seq = 0;             // last detailed field's sequence number
    uint32_t launches = 0;        // ... and its kernel launches (the finish kernel not counted)
    uint32_t sib[3] = {0, 0, 0};  // ... and its last sibling-lane launch: lanes M, stride L, persistent grid
    bool fin_seq = false;         // ... and whether its fd2 finish publishes it
    uint32_t tag = 0;             // ... as tagged words (FieldFinish::tag; 0: bins + sequence word)
    uint32_t tag_words = 0;       // ... bins 0..tag_words-1 (and kFinCount) carry the tag
    MsdBuf msd;
};

struct Device {
    int id = 0;
    int num_cus = 0;
    hipStream_t aux = nullptr;    // self-check recomputes (never behind a queued field); lazily created
    uint64_t *chk_n = nullptr;    // self-check recompute buffers, grown on demand (a hipFree per
    uint32_t *chk_u = nullptr;    // collect would synchronise the whole device)
    size_t chk_cap = 0;
    Slot slot[kSlots];
    std::map<uint32_t, uint32_t *> residues;  // base*8+k -> device residue table
    std::map<uint32_t, uint32_t *> ranks;     // base*8+k -> lower_bound(residues, r), r in [0, M]
    // sound filter: base*8+k -> StrideTable::residues_flagged followed by ::lowmask
    std::map<uint32_t, uint32_t *> lowtabs;
    LeafBuf desc[2];
    int desc_next = 0;
    nice_kernel_stats last{};
    int stats_slot = -1;  // slot whose events last.kernel_ms is still to be read from
};

struct Entry {
    u128 n;
    uint32_t u;
};

// A submitted field, until its results have been handed to the caller.
struct DetJob {
    bool active = false, collected = false;
    bool waiting = false;          // a collect is waiting for it outside the context lock
    std::thread::id owner;         // the submitting thread (acquire_slot's deadlock test)
    u128 s = 0, e = 0;
    uint32_t base = 0;
    std::vector<u128> bounds;      // per-device shard bounds
    std::vector<uint64_t> total;   // merged histogram (after collection)
    std::vector<Entry> all;        // merged near-miss list (after collection)
};
struct NiceJob {
    bool active = false, collected = false;
    bool waiting = false;          // a collect is waiting for it outside the context lock
    std::thread::id owner;         // the submitting thread (acquire_slot's deadlock test)
    // the submitted field, kept so that collect can re-run it (list overflow)
    u128 s = 0, e = 0;
    uint32_t base = 0;
    nice_niceonly_opts opts{};
    bool has_opts = false;
    bool on_device = false;
    bool empty = false;            // nothing enqueued (residue-empty base, no chunk dealt)
    std::vector<char> used;        // devices that ran part of the field
    nice_niceonly_stats st{};
    std::chrono::steady_clock::time_point t0;
    std::vector<Entry> all;
    bool adapt = false;            // host-MSD field on the adaptive floor: update it at collect
    uint32_t reruns = 0;           // times the field was re-run with grown device lists
    uint64_t rejected = 0;         // sound filter: candidates the prefix test rejected
    uint32_t nice_min = 0;         // nice_debug_set_nice_min's value for the base when the field was
                                   // submitted (0: production); a re-run keeps it
};

// The calls beside the field slots (batched detailed ranges, batched niceonly
// ranges, the map) each keep, under a lock of their own (not ctx->mu: fields
// in flight go on), per device a SideStream and the buffers below, and where
// the caller may retry with a longer list the last call's results (KeptList).

// A call's non-blocking stream on one device and the events around its launches.
struct SideStream {
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int init(const Device &d);  // on first use; leaves d current
    // Wait for what was enqueued.
    hipError_t drain(const Device &d) const { return (void)hipSetDevice(d.id), hipStreamSynchronize(stream); }
    hipError_t elapsed(float *ms) const { return hipEventElapsedTime(ms, ev0, ev1); }
    void destroy(const Device &d);  // after drain and the owner's buffers
};

// Pinned host staging and its device copy, of one capacity in units.
struct StagePair {
    void *h = nullptr, *d = nullptr;
    size_t cap = 0;
    // Room for `units` units (4096 at least), on the current device; `busy`:
    // a stream whose queued work may still read the pair.
    int ensure(size_t units, size_t unit_bytes, hipStream_t busy = nullptr);
    void free() {
        if (h) (void)hipHostFree(h);
        if (d) (void)hipFree(d);
    }
};

// What a batched call keeps after NICE_ERR_CAPACITY, for the same call with
// room: the call (`key`: its flags or stride k) and its list; the owners add
// their payload.
struct KeptList {
    bool kept = false;
    uint32_t base = 0, key = 0;
    std::vector<uint64_t> bounds;
    std::vector<Entry> list;
    bool holds(uint32_t b, uint32_t k, const uint64_t *bnd, size_t n_ranges) const {
        return kept && base == b && key == k && bounds.size() == 4 * n_ranges &&
               std::equal(bounds.begin(), bounds.end(), bnd);
    }
    void begin(uint32_t b, uint32_t k, const uint64_t *bnd, size_t n_ranges) {
        kept = false, base = b, key = k, bounds.assign(bnd, bnd + 4 * n_ranges);
    }
    // *n_out = the list's length; NICE_ERR_CAPACITY, and the results kept,
    // when it passes `cap`; else the caller copies the list out and drops it.
    int fits(size_t cap, size_t *n_out);
    void drop() { kept = false, bounds = {}, list = {}; }
};

struct RangesDev {
    SideStream side;
    StagePair desc;              // descriptors (kBatchDescBytes each)
    uint64_t *d_rows = nullptr;  // histogram rows, then the list count
    size_t rows_cap = 0;
    uint32_t *d_count = nullptr;
    ListBuf list;
    uint32_t *chk_u = nullptr;  // self-check recompute of the listed numbers
    uint32_t chk_cap = 0;
};
struct RangesState : KeptList {  // key: the flags
    std::vector<RangesDev> dev;
    nice_ranges_stats stats{};
    std::vector<uint64_t> hist;
    std::vector<uint32_t> list_range;
};

// Its own copies of the residue tables included (Device::residues belongs to
// fields, under ctx->mu).
struct RangesNiceDev {
    SideStream side;
    StagePair leaves;          // RangeLeaf records
    uint32_t *d_sq = nullptr;  // square_ok, one counter per range
    size_t sq_cap = 0;
    uint32_t *d_ctl = nullptr;  // [0] the list count, then kDoneWords arrival counters
    uint32_t *h_count = nullptr, *d_count_mapped = nullptr;  // mapped: the list count at a launch's end
    ListBuf list;               // list.u: the entries' range indices
    std::map<uint32_t, uint32_t *> residues;  // base*8+k -> device residue table
    // the prefix test (nice_process_ranges_niceonly_ex), allocated on its first use
    std::map<uint32_t, uint32_t *> lowtabs;  // base*8+k -> residues_flagged followed by lowmask
    StagePair spans;                         // RangeSpan records, one per fast range of the share
    LeafMask *d_masks = nullptr;             // ... and their masks (range_mask_kernel)
    size_t masks_cap = 0;
    unsigned long long *d_rej = nullptr;     // prefix_rejected, one counter per range
    size_t rej_cap = 0;
    hipEvent_t ev_mask = nullptr;            // after the mask launch (side.ev0 before it)
};
// key: the stride k, plus kRangesPrefixKey with the prefix test on; Entry::u: the range index
constexpr uint32_t kRangesPrefixKey = 1u << 8;
struct RangesNiceState : KeptList {
    std::vector<RangesNiceDev> dev;
    nice_ranges_niceonly_stats stats{};
    nice_ranges_niceonly_prefix_stats prefix{};
    uint32_t nice_min = 0;
    std::vector<uint64_t> candidates;
    std::vector<uint32_t> square_ok;
    std::vector<uint64_t> prefix_rejected;
};

struct MapDev {
    SideStream side;
    StagePair desc;             // FD records (kMapDescBytes each)
    uint8_t *d_out = nullptr;   // host mode: the device's shard of the map
    size_t out_cap = 0;
};
struct MapState {
    std::vector<MapDev> dev;
    nice_map_stats stats{};
};

struct MsdRangesDev {
    SideStream side;              // ev0 / ev1: around a batch's recursion
    hipEvent_t so0 = nullptr, so1 = nullptr;  // ... and around its sort
    StagePair roots;              // MsdRangeRoot records of a batch
    StagePair lists;              // its groups' root indices (u32)
    MsdNode *q[2] = {nullptr, nullptr};  // level queues
    size_t q_cap = 0;
    uint64_t *rec = nullptr;      // 4 x rec_cap u64: keys, sizes, and the sort's output of both
    size_t rec_cap = 0;
    ChunkNode *scratch = nullptr; // the workgroup-per-root form's queues
    size_t scratch_nodes = 0;
    void *sort_tmp = nullptr;
    size_t sort_bytes = 0;
    uint32_t *d_ctl = nullptr;    // level sizes, record count, overflow flag (layout.h's indices)
    uint32_t *h_ctl = nullptr;    // pinned: the last two after a batch
    uint64_t *h_rec = nullptr;    // pinned, 2 x h_rec_cap u64: a batch's ordered keys, then its sizes
    size_t h_rec_cap = 0;
};
struct MsdRangesState : KeptList {  // key: the filter; Entry: a range's start and its root index
    std::vector<MsdRangesDev> dev;
    nice_msd_ranges_stats stats{};
    uint64_t floor_size = 0;
    std::vector<uint64_t> sizes;   // parallel to the list
    std::vector<uint64_t> counts;  // ranges per root
};

}  // namespace abi
}  // namespace nice

struct nice_ctx {
    std::mutex msd_ranges_mu;  // serialises nice_msd_ranges
    nice::abi::MsdRangesState msd_ranges;
    std::mutex map_mu;  // serialises nice_unique_map
    nice::abi::MapState map;
    std::mutex ranges_mu;  // ... nice_process_ranges_detailed
    nice::abi::RangesState ranges;
    std::mutex ranges_nice_mu;  // ... and nice_process_ranges_niceonly
    nice::abi::RangesNiceState ranges_nice;
    std::vector<nice::abi::Device> devs;
    std::mutex mu;  // serialises calls on one context (client_process_gpu.rs:196-201)
    std::condition_variable freed;  // a collect released a slot (synchronous submits wait on it)
    bool timing = true;  // record HIP events around each detailed field (nice_ctx_set_kernel_timing)
    nice::abi::DetJob det[nice::abi::kSlots];
    nice::abi::NiceJob nice[nice::abi::kSlots];
    int det_next = 0, nice_next = 0;
    // threads blocked in acquire_slot (either mode): they collect nothing
    // until they get a slot, so their fields do not count as freeable
    std::vector<std::thread::id> blocked;
};

namespace nice {
namespace abi __attribute__((visibility("hidden"))) {

// The slot a new field takes: the round-robin position if it is free (so
// consecutive fields alternate slots), else the next free one after it
// (tickets may be collected in any order).  -1 if every slot is in flight.
template <class Job>
int free_slot(const Job *jobs, int next) {
    const int n = slots_used();
    for (int i = 0; i < n; i++) {
        const int t = (next + i) % n;
        if (!jobs[t].active) return t;
    }
    return -1;
}

// A free slot for a new field, under ctx->mu (held by `lock`).  Without
// `wait`, NICE_ERR_BUSY when every slot is in flight (the asynchronous
// submits: the caller collects one first).  With `wait` (the synchronous
// reference-shaped calls, which the reference serves behind the context's
// Mutex, client_process_gpu.rs:199-200), block until another thread's
// collect frees one -- unless no other thread can: a field in flight can be
// freed only while a collect is waiting for it, or while its submitter is a
// thread that is not itself blocked here (a blocked thread collects nothing:
// two threads each holding tickets and each waiting for the other's slot
// would otherwise wait forever, so one of them gets NICE_ERR_BUSY).
template <class Job>
int acquire_slot(nice_ctx *ctx, std::unique_lock<std::mutex> &lock, const Job *jobs, int next, bool wait,
                 const char *mode, int *slot) {
    const std::thread::id me = std::this_thread::get_id();
    auto blocked = [&](std::thread::id id) {
        return id == me || std::find(ctx->blocked.begin(), ctx->blocked.end(), id) != ctx->blocked.end();
    };
    auto unblock = [&] {
        auto it = std::find(ctx->blocked.begin(), ctx->blocked.end(), me);
        if (it != ctx->blocked.end()) {
            ctx->blocked.erase(it);
            ctx->freed.notify_all();
        }
    };
    for (;;) {
        const int t = free_slot(jobs, next);
        if (t >= 0) {
            unblock();
            *slot = t;
            return NICE_OK;
        }
        bool freeable = false;
        for (int i = 0; i < slots_used(); i++)
            freeable |= jobs[i].active && (jobs[i].waiting || !blocked(jobs[i].owner));
        if (!wait || !freeable) {
            unblock();
            return fail(NICE_ERR_BUSY, std::string("three ") + mode +
                                           " fields already in flight on this context; collect one first");
        }
        if (std::find(ctx->blocked.begin(), ctx->blocked.end(), me) == ctx->blocked.end()) {
            ctx->blocked.push_back(me);
            // waiters that counted on this thread's fields re-check
            ctx->freed.notify_all();
        }
        ctx->freed.wait(lock);
    }
}

// Replace a device buffer by one of `bytes` bytes holding `new_cap` units: the
// old one freed first (after `drain`, the stream whose queued work may still
// use it, has been synchronised), `cap` zero until the new one exists.  The
// current device is the buffer's.
template <class T, class C>
int grow_device(T *&p, C &cap, C new_cap, size_t bytes, hipStream_t drain = nullptr) {
    if (drain) HIPCHK(hipStreamSynchronize(drain));
    if (p) HIPCHK(hipFree(p));
    p = nullptr;
    cap = 0;
    HIPCHK(hipMalloc(&p, bytes));
    cap = new_cap;
    return NICE_OK;
}
// ... and a pinned host buffer.
template <class T, class C>
int grow_pinned(T *&p, C &cap, C new_cap, size_t bytes) {
    if (p) HIPCHK(hipHostFree(p));
    p = nullptr;
    cap = 0;
    HIPCHK(hipHostMalloc(&p, bytes, hipHostMallocDefault));
    cap = new_cap;
    return NICE_OK;
}

// After an error of a call beside the slots: wait for what it enqueued, on
// every device (`dev`: its per-device blocks, one per device of the context).
template <class Dev>
void drain_all(const nice_ctx *ctx, const std::vector<Dev> &dev) {
    for (size_t q = 0; q < dev.size(); q++)
        if (dev[q].side.stream) (void)dev[q].side.drain(ctx->devs[q]);
}

int ensure_listbuf(Device &d, ListBuf &l, uint32_t cap, bool with_u);

// Entries [0, cnt) of a device list into host vectors (n: (lo, hi) pairs),
// async on `s`.
int read_list(const ListBuf &l, uint32_t cnt, std::vector<uint64_t> &n, std::vector<uint32_t> &u, hipStream_t s);

inline void put_entry(nice_number &o, const Entry &e) {
    o.number_lo = lo64(e.n);
    o.number_hi = hi64(e.n);
    o.num_uniques = e.u;
    o.reserved = 0;
}

// NICE_ERR_CAPACITY for a list of n entries offered room for cap.
int capacity_error(size_t n, size_t cap);

// NICE_ERR_INVALID for the first range of `bounds` that is not range_proper.
int check_ranges(const uint64_t *bounds, size_t n_ranges);

// Sort `all` by n and hand it to the caller (NICE_ERR_CAPACITY: *n_out says
// how many entries it needs).
int emit_list(std::vector<Entry> &all, nice_number *out, size_t cap, size_t *n_out);

// nice_debug_set_near_miss_cutoff: per base, the cutoff the GPU detailed paths
// use instead of near_miss_cutoff(base) (0: production).
inline std::atomic<uint32_t> g_cutoff_override[129];

inline uint32_t effective_cutoff(uint32_t base) {
    const uint32_t c = base <= 128 ? g_cutoff_override[base].load(std::memory_order_relaxed) : 0u;
    return c ? c : near_miss_cutoff(base);
}

// nice_debug_set_nice_min: per base, the union count from which the compile-time
// niceonly kernels list a square survivor of an in-range field (0: production,
// the base).  Read once per field, at submit (NiceJob::nice_min).
inline std::atomic<uint32_t> g_nice_min_override[129];

// The server's submit invariants for a detailed result (api/src/main.rs:
// 309-359): the distribution sums to the field size; for every bin above the
// near-miss cutoff the count equals the number of listed numbers with that
// unique count; the list holds exactly the numbers above the cutoff.  (The
// server's last check, recomputing each listed number, runs on the device in
// nice_process_range_detailed.)  get(i) -> {n, u} of list entry i.  cutoff:
// the one the result was computed with (effective_cutoff for a GPU result).
template <class Get>
int validate_detailed(uint32_t base, uint32_t cutoff, u128 size, const uint64_t *hist, size_t n, Get get) {
    u128 sum = 0;
    for (uint32_t b = 0; b <= base; b++) sum += hist[b];
    if (sum != size)
        return fail(NICE_ERR_HIP, "self-check: distribution total does not equal the field size");
    std::vector<uint64_t> per(base + 1, 0);
    for (size_t i = 0; i < n; i++) {
        const uint32_t u = get(i).u;
        if (u <= cutoff || u > base)
            return fail(NICE_ERR_HIP, "self-check: listed number " + std::to_string(i) +
                                          " has num_uniques " + std::to_string(u) +
                                          " at or below the cutoff");
        per[u]++;
    }
    u128 above = 0;
    for (uint32_t u = cutoff + 1; u <= base; u++) {
        if (per[u] != hist[u])
            return fail(NICE_ERR_HIP, "self-check: " + std::to_string(per[u]) +
                                          " listed numbers with " + std::to_string(u) +
                                          " uniques, distribution claims " + std::to_string(hist[u]));
        above += hist[u];
    }
    if (above != (u128)n) return fail(NICE_ERR_HIP, "self-check: list length does not match the distribution");
    return NICE_OK;
}

// Stride tables by (base, k), built once per process.
struct StrideCache {
    std::mutex mu;
    std::map<std::pair<uint32_t, uint32_t>, std::shared_ptr<StrideTable>> tables;
    std::shared_ptr<StrideTable> get(uint32_t base, uint32_t k) {
        std::lock_guard<std::mutex> g(mu);
        auto key = std::make_pair(base, k);
        auto it = tables.find(key);
        if (it != tables.end()) return it->second;
        auto t = std::make_shared<StrideTable>(base, k);
        tables[key] = t;
        return t;
    }
};
inline StrideCache g_stride;

// Polls spin for the first kSpinPolls (a small field ends within tens of
// microseconds, and a sleeping waiter would add its wake-up latency), then
// yield the core between polls for kYieldPolls more, then sleep between
// polls, 20 us doubling to 200 us: a multi-second field (a split-launch
// detailed field, the massive niceonly field) must not keep a core busy per
// waiting thread beside the host MSD pool.  The sleep adds at most 200 us to
// fields that run for milliseconds.
constexpr uint32_t kSpinPolls = 1u << 14, kYieldPolls = 1u << 11;

inline void backoff(uint32_t i) {
    if (i < kSpinPolls) {
        __builtin_ia32_pause();
    } else if (i < kSpinPolls + kYieldPolls) {
        sched_yield();
    } else {
        const uint32_t k = std::min<uint32_t>((i - kSpinPolls - kYieldPolls) / 8, 3);
        std::this_thread::sleep_for(std::chrono::microseconds(std::min(200u, 20u << (2 * k))));
    }
}

// Wait for an event by polling it (see backoff).
inline hipError_t sync_event(hipEvent_t ev) {
    for (uint32_t i = 0;; i++) {
        const hipError_t q = hipEventQuery(ev);
        if (q != hipErrorNotReady) return q;
        backoff(i);
    }
}

// The event after a detailed field's last launch: the finish kernel's
// (ev_done) when the field needed one; else the kernel end (ev1) of a timed
// field, the end marker (ev_done) of an untimed one on a shared stream, or
// none: an untimed field that fd2 finishes in-kernel on its slot's own stream
// records no event at all (two fewer runtime calls per field), and the stream
// itself reports its completion.
inline hipEvent_t done_event(const Slot &sl) {
    if (!sl.fin_seq) return sl.ev_done;
    return sl.timed ? sl.ev1 : (sl.marked ? sl.ev_done : nullptr);
}

// A detailed field's completion: its end event, or its slot's own stream
// when it recorded none (done_event).
inline hipError_t field_query(const Slot &sl) {
    const hipEvent_t ev = done_event(sl);
    return ev ? hipEventQuery(ev) : hipStreamQuery(sl.stream);
}

inline hipError_t field_sync(const Slot &sl) {
    for (uint32_t i = 0;; i++) {
        const hipError_t q = field_query(sl);
        if (q != hipErrorNotReady) return q;
        backoff(i);
    }
}

// The kernel time of the device's last collected field, read from its slot's
// events on demand (collect returns as soon as the results are published,
// possibly before the end-of-kernel event has completed).
int resolve_stats(Device &d);

// A device's side stream and buffers (nice_ctx_destroy), each in its call's file.
void ranges_dev_free(Device &d, RangesDev &r);
void ranges_nice_dev_free(Device &d, RangesNiceDev &r);
void map_dev_free(Device &d, MapDev &r);
void msd_ranges_dev_free(Device &d, MsdRangesDev &r);

}  // namespace abi
}  // namespace nice
