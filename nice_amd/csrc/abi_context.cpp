// abi_context.cpp -- the C ABI's contexts: device and slot lifetime, the
// calling thread's error message, the shared buffer helpers, and the constant
// and query functions.
#include <cstring>

#include "abi_internal.hpp"
#include "niceonly_bases.h"

namespace {

thread_local std::string g_err;

// Streams of a device's slots: bit 0 = the slots share ONE detailed stream
// (consecutive detailed fields run back to back instead of overlapping at
// their edges), bit 1 = they share one niceonly stream.
inline int shared_streams() { return (int)nice::probe_knob("NICE_SHARED_STREAMS", 0); }

}  // namespace

namespace nice {

// The CPU path (cpu_path.cpp) reports through the same thread-local message.
void set_last_error(const char *msg) { g_err = msg; }

namespace abi {

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

int ensure_listbuf(Device &d, ListBuf &l, uint32_t cap, bool with_u) {
    if (l.cap >= cap) return NICE_OK;
    HIPCHK(hipSetDevice(d.id));
    if (int rc = grow_device(l.n, l.cap, cap, (size_t)cap * 16)) return rc;
    return with_u ? grow_device(l.u, l.cap, cap, (size_t)cap * 4) : NICE_OK;
}

int read_list(const ListBuf &l, uint32_t cnt, std::vector<uint64_t> &n, std::vector<uint32_t> &u, hipStream_t s) {
    n.resize((size_t)cnt * 2);
    u.resize(cnt);
    if (!cnt) return NICE_OK;
    HIPCHK(hipMemcpyAsync(n.data(), l.n, (size_t)cnt * 16, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(u.data(), l.u, (size_t)cnt * 4, hipMemcpyDeviceToHost, s));
    return NICE_OK;
}

int capacity_error(size_t n, size_t cap) {
    return fail(NICE_ERR_CAPACITY,
                "output list needs " + std::to_string(n) + " entries, capacity " + std::to_string(cap));
}

int check_ranges(const uint64_t *bounds, size_t n_ranges) {
    for (size_t i = 0; i < n_ranges; i++)
        if (!range_proper(bounds, i)) return fail(NICE_ERR_INVALID, range_refusal(i));
    return NICE_OK;
}

int emit_list(std::vector<Entry> &all, nice_number *out, size_t cap, size_t *n_out) {
    std::sort(all.begin(), all.end(), [](const Entry &a, const Entry &b) { return a.n < b.n; });
    if (n_out) *n_out = all.size();
    const size_t c = std::min(cap, all.size());
    for (size_t i = 0; i < c; i++) put_entry(out[i], all[i]);
    return all.size() > cap ? capacity_error(all.size(), cap) : NICE_OK;
}

int SideStream::init(const Device &d) {
    if (stream) return NICE_OK;
    HIPCHK(hipSetDevice(d.id));
    HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&ev0));
    HIPCHK(hipEventCreate(&ev1));
    return NICE_OK;
}

void SideStream::destroy(const Device &d) {
    (void)hipSetDevice(d.id);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    (void)hipStreamDestroy(stream);
}

int StagePair::ensure(size_t units, size_t unit_bytes, hipStream_t busy) {
    if (cap >= units) return NICE_OK;
    const size_t c = std::max<size_t>(units, 4096);
    if (busy) HIPCHK(hipStreamSynchronize(busy));
    if (int rc = grow_pinned(h, cap, c, c * unit_bytes)) return rc;
    return grow_device(d, cap, c, c * unit_bytes);
}

int KeptList::fits(size_t cap, size_t *n_out) {
    if (n_out) *n_out = list.size();
    kept = list.size() > cap;
    return kept ? capacity_error(list.size(), cap) : NICE_OK;
}

int resolve_stats(Device &d) {
    if (d.stats_slot < 0) return NICE_OK;
    Slot &sl = d.slot[d.stats_slot];
    d.stats_slot = -1;
    HIPCHK(hipSetDevice(d.id));
    HIPCHK(field_sync(sl));
    float ms = 0;
    if (sl.timed) HIPCHK(hipEventElapsedTime(&ms, sl.ev0, sl.ev1));
    d.last.kernel_ms = ms;
    return NICE_OK;
}

}  // namespace abi
}  // namespace nice

using namespace nice::abi;

namespace {

int slot_init(Device &d, Slot &sl, const Slot *share) {
    if (share && (shared_streams() & 1)) {
        sl.stream = share->stream;
    } else {
        HIPCHK(hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
        sl.own_stream = true;
    }
    int least = 0, greatest = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    if (nice::probe_set("NICE_NICE_PRIO") && nice::probe_knob("NICE_NICE_PRIO", 1) == 0) greatest = least;
    if (share && (shared_streams() & 2)) {
        sl.nstream = share->nstream;
    } else {
        HIPCHK(hipStreamCreateWithPriority(&sl.nstream, hipStreamNonBlocking, greatest));
        sl.own_nstream = true;
    }
    HIPCHK(hipMalloc(&sl.d_nice_count, 4));
    // hist bins and list counters in one block: one memset per field at most.
    HIPCHK(hipMalloc(&sl.d_state, kStateBytes));
    sl.d_count = (uint32_t *)(sl.d_state + (size_t)nice::kHistCopies * nice::kHistBins);
    sl.d_done = sl.d_count + 1;
    HIPCHK(hipHostMalloc(&sl.h_fin, nice::kFinWords * 8, hipHostMallocMapped | hipHostMallocCoherent));
    memset(sl.h_fin, 0, nice::kFinWords * 8);
    HIPCHK(hipHostGetDevicePointer((void **)&sl.d_fin, sl.h_fin, 0));
    HIPCHK(hipHostMalloc(&sl.h_msd, nice::kMsdMappedWords * 4, hipHostMallocMapped | hipHostMallocCoherent));
    memset(sl.h_msd, 0, nice::kMsdMappedWords * 4);
    HIPCHK(hipHostGetDevicePointer((void **)&sl.d_msd_mapped, sl.h_msd, 0));
    HIPCHK(hipHostMalloc(&sl.h_nice, 4, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(hipHostGetDevicePointer((void **)&sl.d_nice_mapped, sl.h_nice, 0));
    HIPCHK(hipMalloc(&sl.d_nice_done, nice::kDoneWords * 4));
    HIPCHK(hipMemset(sl.d_nice_done, 0, nice::kDoneWords * 4));
    HIPCHK(hipEventCreate(&sl.ev0));
    HIPCHK(hipEventCreate(&sl.ev1));
    HIPCHK(hipEventCreateWithFlags(&sl.ev_done, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&sl.nice_done, hipEventDisableTiming));
    HIPCHK(hipEventCreate(&sl.nt0));
    HIPCHK(hipEventCreate(&sl.nt1));
    int rc = ensure_listbuf(d, sl.det, kInitialListCap, true);
    if (!rc) rc = ensure_listbuf(d, sl.nice, kNiceCap, false);
    return rc;
}

int device_init(Device &d, int id) {
    d.id = id;
    HIPCHK(hipSetDevice(id));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, id));
    d.num_cus = prop.multiProcessorCount;
    for (int i = 0; i < kSlots; i++) {
        int rc = slot_init(d, d.slot[i], i ? &d.slot[0] : nullptr);
        if (rc) return rc;
    }
    return NICE_OK;
}

void device_free(Device &d) {
    if (!d.slot[0].stream) return;
    (void)hipSetDevice(d.id);
    if (d.aux) (void)hipStreamSynchronize(d.aux);
    for (auto &sl : d.slot) {
        if (sl.stream) (void)hipStreamSynchronize(sl.stream);
        if (sl.nstream) (void)hipStreamSynchronize(sl.nstream);
    }
    for (auto &kv : d.residues) (void)hipFree(kv.second);
    for (auto &kv : d.ranks) (void)hipFree(kv.second);
    for (auto &kv : d.lowtabs) (void)hipFree(kv.second);
    for (auto &b : d.desc) {
        if (b.h) (void)hipHostFree(b.h);
        if (b.d) (void)hipFree(b.d);
        if (b.done) (void)hipEventDestroy(b.done);
    }
    for (auto &sl : d.slot) {
        for (auto &q : sl.msd.q)
            if (q) (void)hipFree(q);
        if (sl.msd.leaves) (void)hipFree(sl.msd.leaves);
        if (sl.msd.leaf_masks) (void)hipFree(sl.msd.leaf_masks);
        if (sl.msd.counters) (void)hipFree(sl.msd.counters);
        if (sl.msd.scratch) (void)hipFree(sl.msd.scratch);
        if (sl.stream && sl.own_stream) (void)hipStreamDestroy(sl.stream);
        if (sl.nstream && sl.own_nstream) (void)hipStreamDestroy(sl.nstream);
        if (sl.d_nice_count) (void)hipFree(sl.d_nice_count);
        if (sl.d_nice_done) (void)hipFree(sl.d_nice_done);
        if (sl.d_state) (void)hipFree(sl.d_state);
        for (ListBuf *l : {&sl.det, &sl.nice}) {
            if (l->n) (void)hipFree(l->n);
            if (l->u) (void)hipFree(l->u);
        }
        if (sl.h_fin) (void)hipHostFree(sl.h_fin);
        if (sl.h_msd) (void)hipHostFree(sl.h_msd);
        if (sl.h_nice) (void)hipHostFree(sl.h_nice);
        for (hipEvent_t ev : {sl.ev0, sl.ev1, sl.ev_done, sl.nice_done, sl.nt0, sl.nt1})
            if (ev) (void)hipEventDestroy(ev);
    }
    if (d.chk_n) (void)hipFree(d.chk_n);
    if (d.chk_u) (void)hipFree(d.chk_u);
    if (d.aux) (void)hipStreamDestroy(d.aux);
    for (auto &sl : d.slot) sl.stream = nullptr;
}

}  // namespace

extern "C" {

const char *nice_last_error(void) { return g_err.c_str(); }

int nice_device_count(int *out) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    *out = n;
    return NICE_OK;
}

int nice_ctx_create(const int *devices, int n_devices, nice_ctx **out) {
    if (!out) return fail(NICE_ERR_INVALID, "null out");
    int have = 0;
    if (hipGetDeviceCount(&have) != hipSuccess || have < 1)
        return fail(NICE_ERR_NO_DEVICE, "no HIP device visible");
    std::unique_ptr<nice_ctx> ctx(new nice_ctx());
    std::vector<int> ids;
    if (!devices || n_devices <= 0) ids.push_back(0);
    else ids.assign(devices, devices + n_devices);
    ctx->devs.resize(ids.size());
    for (size_t i = 0; i < ids.size(); i++) {
        if (ids[i] < 0 || ids[i] >= have)
            return fail(NICE_ERR_INVALID, "device ordinal " + std::to_string(ids[i]) + " out of range");
        int rc = device_init(ctx->devs[i], ids[i]);
        if (rc) {
            for (auto &d : ctx->devs) device_free(d);
            return rc;
        }
    }
    *out = ctx.release();
    return NICE_OK;
}

int nice_ctx_synchronize(nice_ctx *ctx) {
    if (!ctx) return fail(NICE_ERR_INVALID, "null ctx");
    std::lock_guard<std::mutex> lock(ctx->mu);
    for (auto &d : ctx->devs) {
        HIPCHK(hipSetDevice(d.id));
        for (auto &sl : d.slot) {
            HIPCHK(hipStreamSynchronize(sl.stream));
            HIPCHK(hipStreamSynchronize(sl.nstream));
        }
        if (d.aux) HIPCHK(hipStreamSynchronize(d.aux));
    }
    return NICE_OK;
}

void nice_ctx_destroy(nice_ctx *ctx) {
    if (!ctx) return;
    for (size_t i = 0; i < ctx->ranges.dev.size() && i < ctx->devs.size(); i++)
        ranges_dev_free(ctx->devs[i], ctx->ranges.dev[i]);
    for (size_t i = 0; i < ctx->ranges_nice.dev.size() && i < ctx->devs.size(); i++)
        ranges_nice_dev_free(ctx->devs[i], ctx->ranges_nice.dev[i]);
    for (size_t i = 0; i < ctx->map.dev.size() && i < ctx->devs.size(); i++)
        map_dev_free(ctx->devs[i], ctx->map.dev[i]);
    for (size_t i = 0; i < ctx->msd_ranges.dev.size() && i < ctx->devs.size(); i++)
        msd_ranges_dev_free(ctx->devs[i], ctx->msd_ranges.dev[i]);
    for (auto &d : ctx->devs) device_free(d);
    delete ctx;
}

int nice_ctx_set_kernel_timing(nice_ctx *ctx, int enable) {
    if (!ctx) return fail(NICE_ERR_INVALID, "null ctx");
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->timing = enable != 0;
    return NICE_OK;
}

int nice_last_kernel_stats(nice_ctx *ctx, int i, nice_kernel_stats *out) {
    if (!ctx || i < 0 || i >= (int)ctx->devs.size() || !out) return fail(NICE_ERR_INVALID, "bad args");
    // (under the context lock: a collect on another thread updates the
    // device's last-field record)
    std::lock_guard<std::mutex> lock(ctx->mu);
    int rc = resolve_stats(ctx->devs[i]);
    if (rc) return rc;
    *out = ctx->devs[i].last;
    return NICE_OK;
}

int nice_base_range(uint32_t base, uint64_t *slo, uint64_t *shi, uint64_t *elo, uint64_t *ehi) {
    nice::u128 s = 0, e = 0;
    int rc = nice::base_range_cached(base, s, e);
    if (rc == 1) {
        *slo = lo64(s);
        *shi = hi64(s);
        *elo = lo64(e);
        *ehi = hi64(e);
    }
    return rc;
}

uint32_t nice_near_miss_cutoff(uint32_t base) { return nice::near_miss_cutoff(base); }
uint64_t nice_gpu_batch_size(void) { return 50000000ull; }
uint64_t nice_processing_chunk_size(void) { return 1000000ull; }
int nice_gpu_supports_base(uint32_t base) { return base >= 2 && base <= 128; }
int nice_fd_kernel_base(uint32_t base) { return nice::fd2_supported(base) ? 1 : 0; }
int nice_niceonly_fast_base(uint32_t base) { return nice::niceonly_fast_base(base) ? 1 : 0; }

}  // extern "C"
