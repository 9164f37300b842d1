// abi_detailed.cpp -- detailed fields: enqueue on every device, wait for the
// published result words, gather and self-check, submit / collect.
#include <cstring>

#include "abi_internal.hpp"

using namespace nice::abi;
using nice::u128;

namespace {

// How collect waits for a detailed field that ends in fd2's in-kernel finish:
// by polling the sequence word it publishes in mapped memory (default), or
// (probe build: NICE_SPIN=0) by the stream's completion event.
inline bool spin_wait() { return nice::probe_knob("NICE_SPIN", 1) != 0; }

// Enqueue the detailed kernels for [s, e) on one device (async): generic
// kernel outside the base's valid range, FD kernel inside.  Returns in
// *finished whether the last launch also finished the field (fd2's in-kernel
// finish into the slot's mapped result words); otherwise the caller enqueues
// the epilogue kernel.
int enqueue_detailed(Device &d, Slot &sl, u128 s, u128 e, uint32_t base, bool *finished) {
    nice::DetailedLaunch p{};
    p.base = base;
    p.cutoff = effective_cutoff(base);
    p.hist = sl.d_state;
    p.out = nice::NumOut{sl.det.n, sl.det.u, sl.d_count, sl.det.cap};
    p.launches = &sl.launches;
    p.sib = sl.sib;
    // Another detailed field of this device submitted and not yet collected:
    // the caller pipelines, so this field's launches are shaped for throughput
    // (fd2_plan.hpp plan_sib).  Whether that field is still running does not matter --
    // fields on the slot streams progress together and often finish
    // together, and a pick that followed their completion flipped every third
    // 2.5e8 field to the lone-field stride (8 % slower per step,
    // profiles/r06/stride/probe_pick.log).
    for (const Slot &o : d.slot)
        if (&o != &sl && o.inflight) p.overlapped = 1;
    *finished = false;
    // Small fields run wholly by fd2 publish tagged result words
    // (FieldFinish::tag): one fewer round trip to host memory at their end.
    uint32_t tag = 0;
    auto launch = [&](u128 a, u128 b, bool fd) -> int {
        if (a >= b) return NICE_OK;
        u128 cnt = b - a;
        while (cnt) {  // segments longer than 2^63 are split (count is u64)
            uint64_t c = cnt > ((u128)1 << 62) ? (1ull << 62) : (uint64_t)cnt;
            p.start_lo = lo64(a);
            p.start_hi = hi64(a);
            p.count = c;
            // the field's last launch finishes it when it is an fd2 launch
            const bool last = a + c == e;
            p.fin = last && fd ? nice::FieldFinish{sl.d_fin, sl.d_done, sl.seq, tag}
                               : nice::FieldFinish{nullptr, nullptr, 0, 0};
            if (nice::probe_set("NICE_FD2_NOFIN")) p.fin = nice::FieldFinish{nullptr, nullptr, 0, 0};  // probe: finish kernel
            hipError_t err = fd ? nice::launch_detailed_fd2(p, d.num_cus, sl.stream)
                                : nice::launch_detailed_generic(p, d.num_cus, sl.stream);
            if (!fd) sl.launches++;
            if (err != hipSuccess)
                return fail(NICE_ERR_HIP, std::string("detailed launch: ") + hipGetErrorString(err));
            if (last) {
                *finished = fd && p.fin.out_mapped;
                sl.tag = *finished ? p.fin.tag : 0u;
                sl.tag_words = base + 1;
            }
            a += c;
            cnt -= c;
        }
        return NICE_OK;
    };
    u128 rs = 0, re = 0;
    const bool fd_base = nice::fd2_supported(base);
    const bool fd = fd_base && nice::base_range_cached(base, rs, re) == 1;
    // Histogram copies the field's launches flush into: a small field run
    // wholly by fd2 keeps 16 (its whole grid flushes at once, and the
    // in-kernel finish reads every copy in use); anything else all 64 (the
    // generic kernel and the finish kernel use all of them).
    const bool small_fd = fd && s >= rs && e <= re && e - s < 20000000;
    p.hist_copies = small_fd ? 16 : nice::kHistCopies;
    // (probe: NICE_FD2_UNTAGGED publishes bins + sequence word as large fields do)
    if (small_fd && !nice::probe_set("NICE_FD2_UNTAGGED")) tag = (uint32_t)sl.seq | 0x80000000u;
    sl.tag = 0;
    if (!fd) return launch(s, e, false);
    int rc;
    if ((rc = launch(s, std::min(e, rs), false))) return rc;
    if ((rc = launch(std::max(s, rs), std::min(e, re), true))) return rc;
    return launch(std::max(s, re), e, false);
}

// A field's published result words: its sequence word, or (tagged fields)
// every bin word and the near-miss count carrying the field's tag.
bool published(const Slot &sl) {
    if (!sl.tag) return __atomic_load_n(&sl.h_fin[nice::kFinSeq], __ATOMIC_ACQUIRE) == sl.seq;
    if ((uint32_t)(__atomic_load_n(&sl.h_fin[nice::kFinCount], __ATOMIC_ACQUIRE) >> 32) != sl.tag) return false;
    for (uint32_t b = 0; b < sl.tag_words; b++)
        if ((uint32_t)(__atomic_load_n(&sl.h_fin[b], __ATOMIC_ACQUIRE) >> 32) != sl.tag) return false;
    return true;
}

// Wait until the detailed field in slot `sl` is finished.  A field ending in
// fd2's in-kernel finish is waited for by polling the result words that
// finish publishes in mapped memory -- microseconds sooner than the kernel's
// completion signal (which still follows: the last workgroup retires after
// publishing).  The completion event is queried every 4096 polls, so a failed
// launch or a finish that never publishes is reported, not spun on.
int wait_field(Slot &sl) {
    if (!sl.fin_seq || !spin_wait()) {
        const hipError_t q = field_sync(sl);
        if (q != hipSuccess) return fail(NICE_ERR_HIP, std::string("detailed field: ") + hipGetErrorString(q));
        return NICE_OK;
    }
    for (uint32_t i = 1;; i++) {
        if (published(sl)) return NICE_OK;
        if ((i & 4095) == 0 || i > kSpinPolls) {
            const hipError_t q = field_query(sl);
            if (q == hipSuccess) {
                if (published(sl)) return NICE_OK;
                return fail(NICE_ERR_HIP, "detailed field completed without publishing its results");
            }
            if (q != hipErrorNotReady) return fail(NICE_ERR_HIP, std::string("detailed field: ") + hipGetErrorString(q));
        }
        backoff(i);
    }
}

// Enqueue one device's shard of a detailed field into slot `sl` (async).
int enqueue_detailed_shard(Device &d, Slot &sl, u128 s, u128 e, uint32_t base, bool timing) {
    HIPCHK(hipSetDevice(d.id));
    // this slot's events are about to be re-recorded
    if (d.stats_slot == (int)(&sl - d.slot)) {
        int rc = resolve_stats(d);
        if (rc) return rc;
    }
    sl.seq++;
    sl.launches = 0;
    sl.sib[0] = sl.sib[1] = sl.sib[2] = 0;
    // The state block is zeroed by the previous field's finish; a memset
    // only after an interrupted field (or the first one).
    if (sl.dirty) HIPCHK(hipMemsetAsync(sl.d_state, 0, kStateBytes, sl.stream));
    sl.dirty = true;
    sl.timed = timing;
    sl.marked = false;
    if (timing) HIPCHK(hipEventRecord(sl.ev0, sl.stream));
    bool finished = false;
    int rc = enqueue_detailed(d, sl, s, e, base, &finished);
    if (rc) return rc;
    sl.inflight = true;
    if (timing) HIPCHK(hipEventRecord(sl.ev1, sl.stream));
    sl.fin_seq = finished;
    if (!finished) {
        HIPCHK(nice::launch_detailed_finish(sl.d_state, sl.d_count, sl.d_fin, sl.stream));
        HIPCHK(hipEventRecord(sl.ev_done, sl.stream));
    } else if (!timing && !sl.own_stream) {
        // a stream shared between slots (probe build) cannot tell this
        // field's completion from a later one's: mark its end
        HIPCHK(hipEventRecord(sl.ev_done, sl.stream));
        sl.marked = true;
    }
    return NICE_OK;
}

int detailed_submit(nice_ctx *ctx, std::unique_lock<std::mutex> &lock, u128 s, u128 e, uint32_t base,
                    bool wait, int *ticket) {
    int t = -1;
    if (int rc = acquire_slot(ctx, lock, ctx->det, ctx->det_next, wait, "detailed", &t)) return rc;
    DetJob &job = ctx->det[t];
    const size_t nd = ctx->devs.size();
    const u128 size = e - s;
    // Shard bounds: contiguous, in device order (ascending n).
    job.bounds.assign(nd + 1, 0);
    for (size_t i = 0; i <= nd; i++) job.bounds[i] = s + size / nd * i + std::min<u128>(i, size % nd);
    for (size_t i = 0; i < nd; i++) {
        if (job.bounds[i] >= job.bounds[i + 1]) continue;
        int rc = enqueue_detailed_shard(ctx->devs[i], ctx->devs[i].slot[t], job.bounds[i], job.bounds[i + 1], base,
                                        ctx->timing);
        if (rc) return rc;
    }
    job.active = true;
    job.collected = false;
    job.owner = std::this_thread::get_id();
    job.s = s;
    job.e = e;
    job.base = base;
    ctx->det_next = (t + 1) % slots_used();
    *ticket = t;
    return NICE_OK;
}

int detailed_submit_args(nice_ctx *ctx, uint64_t start_lo, uint64_t start_hi, uint64_t end_lo, uint64_t end_hi,
                         uint32_t base, bool wait, int *ticket) {
    if (!ctx || !ticket) return fail(NICE_ERR_INVALID, "null argument");
    if (base < 2 || base > 128) return fail(NICE_ERR_INVALID, "base must be in 2..=128");
    const u128 s = mk(start_lo, start_hi), e = mk(end_lo, end_hi);
    if (s >= e)
        return fail(NICE_ERR_INVALID, "Range has invalid bounds, range_start must be < range_end");
    std::unique_lock<std::mutex> lock(ctx->mu);
    return detailed_submit(ctx, lock, s, e, base, wait, ticket);
}

// A shard's wait_field has returned: its slot's state block is zero again
// (the epilogue) and free for the next field, and the device's last-field
// record follows this run (kernel_ms read on demand, resolve_stats).  Returns
// the near-miss count the run published.
uint32_t shard_finished(Device &d, Slot &sl, int t) {
    sl.dirty = false;
    sl.inflight = false;
    d.stats_slot = t;
    d.last.launches = sl.launches;
    d.last.sib_lanes = sl.sib[0];
    d.last.sib_stride = sl.sib[1];
    d.last.sib_grid = sl.sib[2];
    return (uint32_t)sl.h_fin[nice::kFinCount];
}

// The self-check's last part: every listed number's unique count recomputed
// by the generic per-n device function (full square / cube + digit scan, a
// different code path from the FD kernel that listed it).  Each device
// recomputes its own shard's entries (job.all[off[i], off[i + 1])) on its
// auxiliary stream (so no queued field is waited for), all devices at once.
int recompute_listed(nice_ctx *ctx, const DetJob &job, const std::vector<size_t> &off) {
    const size_t nd = ctx->devs.size();
    std::vector<std::vector<uint32_t>> u(nd);
    std::vector<std::vector<uint64_t>> pairs(nd);
    // Devices whose aux stream still has copies from / into pairs and u:
    // any return drains them first (declared after the buffers, so it
    // runs before they are freed).
    struct Drain {
        nice_ctx *ctx;
        std::vector<char> q;
        ~Drain() {
            for (size_t j = 0; j < q.size(); j++)
                if (q[j]) {
                    (void)hipSetDevice(ctx->devs[j].id);
                    (void)hipStreamSynchronize(ctx->devs[j].aux);
                }
        }
    } drain{ctx, std::vector<char>(nd, 0)};
    for (size_t i = 0; i < nd; i++) {
        const size_t n = off[i + 1] - off[i];
        if (!n) continue;
        Device &d = ctx->devs[i];
        HIPCHK(hipSetDevice(d.id));
        // created on first use: an idle stream would still take one of the
        // process's few hardware queues (GPU_MAX_HW_QUEUES)
        if (!d.aux) HIPCHK(hipStreamCreateWithFlags(&d.aux, hipStreamNonBlocking));
        pairs[i].resize(2 * n);
        for (size_t q = 0; q < n; q++) {
            pairs[i][2 * q] = lo64(job.all[off[i] + q].n);
            pairs[i][2 * q + 1] = hi64(job.all[off[i] + q].n);
        }
        if (d.chk_cap < n) {
            // grown rarely (the recompute of the previous field finished
            // before its collect returned, so nothing reads the old buffers)
            const size_t c = std::max<size_t>(n, 4096);
            if (int rc = grow_device(d.chk_n, d.chk_cap, c, c * 16)) return rc;
            if (int rc = grow_device(d.chk_u, d.chk_cap, c, c * 4)) return rc;
        }
        u[i].resize(n);
        drain.q[i] = 1;
        hipError_t err = hipMemcpyAsync(d.chk_n, pairs[i].data(), n * 16, hipMemcpyHostToDevice, d.aux);
        if (err == hipSuccess) err = nice::launch_unique_counts(d.chk_n, (uint32_t)n, job.base, d.chk_u, d.aux);
        if (err == hipSuccess) err = hipMemcpyAsync(u[i].data(), d.chk_u, n * 4, hipMemcpyDeviceToHost, d.aux);
        if (err != hipSuccess) return fail(NICE_ERR_HIP, std::string("self-check: ") + hipGetErrorString(err));
    }
    for (size_t i = 0; i < nd; i++) {
        if (u[i].empty()) continue;
        Device &d = ctx->devs[i];
        HIPCHK(hipSetDevice(d.id));
        const hipError_t err = hipStreamSynchronize(d.aux);
        drain.q[i] = 0;
        if (err != hipSuccess) return fail(NICE_ERR_HIP, std::string("self-check: ") + hipGetErrorString(err));
        for (size_t q = 0; q < u[i].size(); q++)
            if (u[i][q] != job.all[off[i] + q].u)
                return fail(NICE_ERR_HIP, "self-check: unique count of a listed number does not recompute");
    }
    return NICE_OK;
}

// Wait for a submitted detailed field, merge the devices' results into the
// job and self-check them (the server's submit invariants).
int detailed_gather(nice_ctx *ctx, DetJob &job, int t) {
    const uint32_t base = job.base;
    const size_t nd = ctx->devs.size();
    job.total.assign(base + 1, 0);
    job.all.clear();
    std::vector<size_t> off(nd + 1, 0);  // device i's list entries: job.all[off[i], off[i + 1])
    for (size_t i = 0; i < nd; i++) {
        off[i] = job.all.size();
        Device &d = ctx->devs[i];
        Slot &sl = d.slot[t];
        d.last = nice_kernel_stats{};
        d.stats_slot = -1;
        if (job.bounds[i] >= job.bounds[i + 1]) continue;
        HIPCHK(hipSetDevice(d.id));
        int rc = wait_field(sl);
        if (rc) return rc;
        d.last.numbers = (uint64_t)(job.bounds[i + 1] - job.bounds[i]);
        d.last.fd_kernel = nice::fd2_supported(base) ? 1u : 0u;
        uint32_t cnt = shard_finished(d, sl, t);
        if (cnt > sl.det.cap) {
            // Near-miss list overflowed (e.g. out-of-range n, SURVEY hazard 9):
            // grow to the exact count and redo this shard (behind any field
            // queued after it; only this slot's completion is awaited).
            rc = ensure_listbuf(d, sl.det, cnt, true);
            if (!rc) rc = enqueue_detailed_shard(d, sl, job.bounds[i], job.bounds[i + 1], base, sl.timed);
            if (!rc) rc = wait_field(sl);
            if (rc) return rc;
            cnt = shard_finished(d, sl, t);
            if (cnt > sl.det.cap) return fail(NICE_ERR_HIP, "near-miss list overflow after resize");
        }
        for (uint32_t b = 0; b <= base; b++) job.total[b] += sl.tag ? (uint32_t)sl.h_fin[b] : sl.h_fin[b];
        if (cnt) {
            // the list is read after the kernel has retired (its end-of-kernel
            // cache write-back), not merely published its count
            HIPCHK(field_sync(sl));
            std::vector<uint64_t> nbuf((size_t)cnt * 2);
            std::vector<uint32_t> ubuf(cnt);
            HIPCHK(hipMemcpy(nbuf.data(), sl.det.n, (size_t)cnt * 16, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(ubuf.data(), sl.det.u, (size_t)cnt * 4, hipMemcpyDeviceToHost));
            for (uint32_t q = 0; q < cnt; q++) job.all.push_back({mk(nbuf[2 * q], nbuf[2 * q + 1]), ubuf[q]});
        }
    }
    off[nd] = job.all.size();
    // Self-check: the server's submit invariants (api/src/main.rs:309-359)
    // before anything is returned, and its last one (recompute_listed).
    int rc = validate_detailed(base, effective_cutoff(base), job.e - job.s, job.total.data(), job.all.size(),
                               [&](size_t i) { return job.all[i]; });
    if (!rc && !job.all.empty()) rc = recompute_listed(ctx, job, off);
    if (rc) return rc;
    std::sort(job.all.begin(), job.all.end(), [](const Entry &a, const Entry &b) { return a.n < b.n; });
    return NICE_OK;
}

// The field under ticket t is lost: its slot is reusable.
void detailed_drop(nice_ctx *ctx, int t) {
    ctx->det[t].active = false;
    for (auto &d : ctx->devs) d.slot[t].dirty = true, d.slot[t].inflight = false;
}

int detailed_collect(nice_ctx *ctx, int t, uint64_t *hist, nice_number *out, size_t cap, size_t *n_out) {
    if (t < 0 || t >= kSlots || !ctx->det[t].active)
        return fail(NICE_ERR_INVALID, "no detailed field in flight under this ticket");
    DetJob &job = ctx->det[t];
    if (!job.collected) {
        int rc = detailed_gather(ctx, job, t);
        if (rc) {
            detailed_drop(ctx, t);
            return rc;
        }
        job.collected = true;
    }
    std::memcpy(hist, job.total.data(), (job.base + 1) * 8);
    int rc = emit_list(job.all, out, cap, n_out);
    if (rc == NICE_ERR_CAPACITY) return rc;  // kept: the caller retries with room
    job.active = false;
    job.all = {};
    return rc;
}

int detailed_collect_locked(nice_ctx *ctx, int ticket, uint64_t *hist, nice_number *out, size_t cap,
                            size_t *n_out) {
    std::unique_lock<std::mutex> lock(ctx->mu);
    if (ticket < 0 || ticket >= kSlots || !ctx->det[ticket].active)
        return fail(NICE_ERR_INVALID, "no detailed field in flight under this ticket");
    DetJob &job = ctx->det[ticket];
    if (job.waiting) return fail(NICE_ERR_INVALID, "another thread is collecting this detailed field");
    if (!job.collected) {
        // Wait for every device's shard to publish WITHOUT the context lock,
        // so other threads can submit and collect other fields meanwhile (the
        // slot stays reserved: the job is active).  The gather below then
        // finds them finished.
        job.waiting = true;
        lock.unlock();
        int rc = NICE_OK;
        for (size_t i = 0; i < ctx->devs.size() && !rc; i++) {
            if (job.bounds[i] >= job.bounds[i + 1]) continue;
            const hipError_t err = hipSetDevice(ctx->devs[i].id);
            rc = err != hipSuccess ? fail(NICE_ERR_HIP, hipGetErrorString(err)) : wait_field(ctx->devs[i].slot[ticket]);
        }
        lock.lock();
        job.waiting = false;
        if (rc) {
            detailed_drop(ctx, ticket);
            return rc;
        }
    }
    return detailed_collect(ctx, ticket, hist, out, cap, n_out);
}

}  // namespace

extern "C" {

int nice_detailed_submit(nice_ctx *ctx, uint64_t start_lo, uint64_t start_hi, uint64_t end_lo,
                         uint64_t end_hi, uint32_t base, int *ticket) {
    return detailed_submit_args(ctx, start_lo, start_hi, end_lo, end_hi, base, false, ticket);
}

int nice_detailed_collect(nice_ctx *ctx, int ticket, uint64_t *hist, nice_number *out, size_t cap,
                          size_t *n_out) {
    if (!ctx || !hist) return fail(NICE_ERR_INVALID, "null argument");
    const int rc = detailed_collect_locked(ctx, ticket, hist, out, cap, n_out);
    ctx->freed.notify_all();  // the ticket's slot may be free now
    return rc;
}

int nice_process_range_detailed(nice_ctx *ctx, uint64_t start_lo, uint64_t start_hi,
                                uint64_t end_lo, uint64_t end_hi, uint32_t base, uint64_t *hist,
                                nice_number *out, size_t cap, size_t *n_out) {
    int t = -1;
    int rc = detailed_submit_args(ctx, start_lo, start_hi, end_lo, end_hi, base, true, &t);
    if (rc) return rc;
    rc = nice_detailed_collect(ctx, t, hist, out, cap, n_out);
    if (rc == NICE_ERR_CAPACITY) {
        // synchronous call: the caller retries the whole field with room
        {
            std::lock_guard<std::mutex> lock(ctx->mu);
            ctx->det[t].active = false;
            ctx->det[t].all = {};
        }
        ctx->freed.notify_all();
    }
    return rc;
}

}  // extern "C"
