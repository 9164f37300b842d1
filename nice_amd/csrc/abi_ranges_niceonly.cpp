// abi_ranges_niceonly.cpp -- batched niceonly ranges
// (nice_process_ranges_niceonly, nice_process_ranges_niceonly_ex): the caller's
// ranges, tested as given, in at most two launches per device -- the base's
// compile-time kernel for the ranges inside its valid range, the run-time-base
// kernel for the rest.  With the _ex call's prefix test on, a mask launch per
// device goes first (one RangeSpan per fast range of the device's share) and
// the fast group runs the kernel's prefix-testing variant.  The plan is
// niceonly_ranges_plan.hpp's, the kernels niceonly_ranges.hpp's.
#include <cstring>

#include "abi_internal.hpp"
#include "niceonly_ranges_plan.hpp"

using namespace nice::abi;
using nice::u128;

namespace {

// A device's share of a call: its leaves, the fast group's first.
struct DevShare {
    std::vector<nice::RangeLeaf> leaves;
    uint32_t n_fast = 0;
    std::vector<nice::RangeSpan> spans;  // prefix test: the fast ranges with a leaf here (RangeLeaf::mask)
};

int ranges_nice_dev_init(Device &d, RangesNiceDev &r) {
    if (r.side.stream) return NICE_OK;
    if (int rc = r.side.init(d)) return rc;
    HIPCHK(hipMalloc(&r.d_ctl, (1 + nice::kDoneWords) * 4));
    HIPCHK(hipHostMalloc(&r.h_count, 4, hipHostMallocMapped | hipHostMallocCoherent));
    *r.h_count = 0;
    HIPCHK(hipHostGetDevicePointer((void **)&r.d_count_mapped, r.h_count, 0));
    return NICE_OK;
}

}  // namespace

void nice::abi::ranges_nice_dev_free(Device &d, RangesNiceDev &r) {
    if (!r.side.stream) return;
    (void)r.side.drain(d);
    r.leaves.free();
    if (r.d_sq) (void)hipFree(r.d_sq);
    r.spans.free();
    if (r.d_masks) (void)hipFree(r.d_masks);
    if (r.d_rej) (void)hipFree(r.d_rej);
    if (r.ev_mask) (void)hipEventDestroy(r.ev_mask);
    for (auto &kv : r.lowtabs) (void)hipFree(kv.second);
    if (r.d_ctl) (void)hipFree(r.d_ctl);
    if (r.h_count) (void)hipHostFree(r.h_count);
    if (r.list.n) (void)hipFree(r.list.n);
    if (r.list.u) (void)hipFree(r.list.u);
    for (auto &kv : r.residues) (void)hipFree(kv.second);
    r.side.destroy(d);
}

namespace {

// What a call runs with, resolved once.
struct NiceRangesCall {
    uint32_t base, k, nice_min;
    size_t n_ranges;
    std::shared_ptr<nice::StrideTable> table;
    bool prefix = false;  // the prefix test is on
};

// The prefix test's buffers and tables on a device, and its share's spans
// staged (async on the call's stream).
int ranges_nice_prefix_stage(RangesNiceDev &r, const NiceRangesCall &c, const DevShare &sh, uint32_t key) {
    const size_t R = c.table->residues.size();
    if (!r.lowtabs.count(key)) {
        uint32_t *p = nullptr;
        HIPCHK(hipMalloc(&p, (R + c.table->lowmask.size()) * 4));
        r.lowtabs[key] = p;
        HIPCHK(hipMemcpy(p, c.table->residues_flagged.data(), R * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p + R, c.table->lowmask.data(), c.table->lowmask.size() * 4, hipMemcpyHostToDevice));
    }
    if (!r.ev_mask) HIPCHK(hipEventCreate(&r.ev_mask));
    const size_t ns = sh.spans.size();
    if (int rc = r.spans.ensure(ns, sizeof(nice::RangeSpan), r.side.stream)) return rc;
    if (r.masks_cap < ns) {
        const size_t cap = std::max<size_t>(ns, 4096);
        if (int rc = grow_device(r.d_masks, r.masks_cap, cap, cap * sizeof(nice::LeafMask), r.side.stream)) return rc;
    }
    if (r.rej_cap < c.n_ranges) {
        const size_t cap = std::max<size_t>(c.n_ranges, 1024);
        if (int rc = grow_device(r.d_rej, r.rej_cap, cap, cap * 8, r.side.stream)) return rc;
    }
    std::memcpy(r.spans.h, sh.spans.data(), ns * sizeof(nice::RangeSpan));
    HIPCHK(hipMemcpyAsync(r.spans.d, r.spans.h, ns * sizeof(nice::RangeSpan), hipMemcpyHostToDevice, r.side.stream));
    HIPCHK(hipMemsetAsync(r.d_rej, 0, c.n_ranges * 8, r.side.stream));
    return NICE_OK;
}

// Enqueue a device's share (async on its batch stream): the leaves, the
// counters zeroed, one launch per group present.
int ranges_nice_enqueue(Device &d, RangesNiceDev &r, const NiceRangesCall &c, const DevShare &sh,
                        uint32_t *launches) {
    HIPCHK(hipSetDevice(d.id));
    const uint32_t key = c.base * 8 + c.k;
    if (!r.residues.count(key)) {
        uint32_t *p = nullptr;
        HIPCHK(hipMalloc(&p, c.table->residues.size() * 4));
        r.residues[key] = p;
        HIPCHK(hipMemcpy(p, c.table->residues.data(), c.table->residues.size() * 4, hipMemcpyHostToDevice));
    }
    const size_t nl = sh.leaves.size();
    if (int rc = r.leaves.ensure(nl, sizeof(nice::RangeLeaf))) return rc;
    if (r.sq_cap < c.n_ranges) {
        const size_t cap = std::max<size_t>(c.n_ranges, 1024);
        if (int rc = grow_device(r.d_sq, r.sq_cap, cap, cap * 4)) return rc;
    }
    if (int rc = ensure_listbuf(d, r.list, std::max<uint32_t>(r.list.cap, 4096), true)) return rc;
    const hipStream_t stream = r.side.stream;
    const bool prefix = c.prefix && !sh.spans.empty();
    if (prefix)
        if (int rc = ranges_nice_prefix_stage(r, c, sh, key)) return rc;
    std::memcpy(r.leaves.h, sh.leaves.data(), nl * sizeof(nice::RangeLeaf));
    HIPCHK(hipMemcpyAsync(r.leaves.d, r.leaves.h, nl * sizeof(nice::RangeLeaf), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemsetAsync(r.d_sq, 0, c.n_ranges * 4, stream));
    HIPCHK(hipMemsetAsync(r.d_ctl, 0, (1 + nice::kDoneWords) * 4, stream));
    *r.h_count = 0;
    nice::NiceRangesLaunch p{};
    p.c.residues = r.residues[key];
    p.c.R = (uint32_t)c.table->residues.size();
    p.c.M = (uint32_t)c.table->modulus;
    p.c.base = c.base;
    p.c.out = nice::NumOut{r.list.n, r.list.u, r.d_ctl, r.list.cap};
    p.square_ok = r.d_sq;
    p.done = r.d_ctl + 1;
    p.count_mapped = r.d_count_mapped;
    nice::RangesPrefixLaunch pre{};
    HIPCHK(hipEventRecord(r.side.ev0, stream));
    if (prefix) {
        pre.snd.residues = r.lowtabs[key];
        pre.snd.lowmask = pre.snd.residues + p.c.R;
        pre.masks = r.d_masks;
        pre.rejected = r.d_rej;
        const hipError_t err = nice::launch_range_masks(c.base, (const nice::RangeSpan *)r.spans.d,
                                                        (uint32_t)sh.spans.size(), r.d_masks, stream);
        if (err != hipSuccess)
            return fail(NICE_ERR_HIP, std::string("niceonly range masks launch: ") + hipGetErrorString(err));
        HIPCHK(hipEventRecord(r.ev_mask, stream));
    }
    for (int fast = 1; fast >= 0; fast--) {
        p.leaves = (const nice::RangeLeaf *)r.leaves.d + (fast ? 0 : sh.n_fast);
        p.n_leaves = fast ? sh.n_fast : (uint32_t)(nl - sh.n_fast);
        if (!p.n_leaves) continue;
        p.c.in_range = (uint32_t)fast;
        p.c.nice_min = fast ? c.nice_min : c.base;
        const hipError_t err = nice::launch_niceonly_ranges(p, d.num_cus, stream, fast && prefix ? &pre : nullptr);
        if (err != hipSuccess)
            return fail(NICE_ERR_HIP, std::string("niceonly ranges launch: ") + hipGetErrorString(err));
        ++*launches;
    }
    HIPCHK(hipEventRecord(r.side.ev1, stream));
    return NICE_OK;
}

// Wait for a device's share and add its results: the per-range square
// survivors and the listed numbers with their range indices.
int ranges_nice_gather(Device &d, RangesNiceDev &r, const NiceRangesCall &c, const DevShare &sh, uint32_t *launches,
                       std::vector<uint32_t> &square_ok, std::vector<uint64_t> &prefix_rejected,
                       std::vector<Entry> &list, double *ms, double *mask_ms) {
    HIPCHK(hipSetDevice(d.id));
    const hipStream_t stream = r.side.stream;
    uint32_t cnt = 0;
    for (int attempt = 0;; attempt++) {
        HIPCHK(hipStreamSynchronize(stream));
        cnt = *r.h_count;  // published by the last launch's last workgroup
        if (cnt <= r.list.cap) break;
        // the device list overflowed: grow it and run the share again
        if (attempt) return fail(NICE_ERR_HIP, "niceonly ranges list overflow after resize");
        if (cnt > 0xfffff000u) return fail(NICE_ERR_HIP, "niceonly ranges list longer than 2^32 entries");
        int rc = ensure_listbuf(d, r.list, (cnt + 4095u) & ~4095u, true);
        *launches = 0;
        if (!rc) rc = ranges_nice_enqueue(d, r, c, sh, launches);
        if (rc) return rc;
    }
    float t = 0;
    HIPCHK(r.side.elapsed(&t));
    *ms = t;
    const bool prefix = c.prefix && !sh.spans.empty();
    std::vector<uint32_t> sq(c.n_ranges);
    HIPCHK(hipMemcpyAsync(sq.data(), r.d_sq, c.n_ranges * 4, hipMemcpyDeviceToHost, stream));
    std::vector<uint64_t> rej;
    if (prefix) {
        HIPCHK(hipEventElapsedTime(&t, r.side.ev0, r.ev_mask));
        *mask_ms = t;
        rej.resize(c.n_ranges);
        HIPCHK(hipMemcpyAsync(rej.data(), r.d_rej, c.n_ranges * 8, hipMemcpyDeviceToHost, stream));
    }
    std::vector<uint64_t> nbuf;
    std::vector<uint32_t> ubuf;
    if (int rc = read_list(r.list, cnt, nbuf, ubuf, stream)) return rc;
    HIPCHK(hipStreamSynchronize(stream));
    for (size_t i = 0; i < c.n_ranges; i++) square_ok[i] += sq[i];
    for (size_t i = 0; i < rej.size(); i++) prefix_rejected[i] += rej[i];
    for (uint32_t q = 0; q < cnt; q++) {
        if (ubuf[q] >= c.n_ranges) return fail(NICE_ERR_HIP, "self-check: a listed number's range index is out of bounds");
        list.push_back({mk(nbuf[2 * q], nbuf[2 * q + 1]), ubuf[q]});
    }
    return NICE_OK;
}

int ranges_nice_emit(RangesNiceState &st, uint64_t *candidates, uint32_t *square_ok, uint64_t *prefix_rejected,
                     nice_number *out, uint32_t *out_range, size_t cap, size_t *n_out) {
    if (candidates) std::memcpy(candidates, st.candidates.data(), st.candidates.size() * 8);
    if (square_ok) std::memcpy(square_ok, st.square_ok.data(), st.square_ok.size() * 4);
    if (prefix_rejected) std::memcpy(prefix_rejected, st.prefix_rejected.data(), st.prefix_rejected.size() * 8);
    if (int rc = st.fits(cap, n_out)) return rc;
    for (size_t i = 0; i < st.list.size(); i++) {
        put_entry(out[i], Entry{st.list[i].n, st.base});  // num_uniques = base, like every niceonly entry
        if (out_range) out_range[i] = st.list[i].u;
    }
    st.drop();
    st.candidates = {};
    st.square_ok = {};
    st.prefix_rejected = {};
    return NICE_OK;
}

// Run every device's share: all enqueued, then all gathered.
int ranges_nice_run(nice_ctx *ctx, RangesNiceState &st, const NiceRangesCall &c, const std::vector<DevShare> &shares) {
    const size_t nd = ctx->devs.size();
    std::vector<uint32_t> launches(nd, 0);
    for (size_t dv = 0; dv < nd; dv++) {
        if (shares[dv].leaves.empty()) continue;
        int rc = ranges_nice_dev_init(ctx->devs[dv], st.dev[dv]);
        if (!rc) rc = ranges_nice_enqueue(ctx->devs[dv], st.dev[dv], c, shares[dv], &launches[dv]);
        if (rc) return drain_all(ctx, st.dev), rc;
    }
    for (size_t dv = 0; dv < nd; dv++) {
        if (shares[dv].leaves.empty()) continue;
        double ms = 0, mask_ms = 0;
        const int rc = ranges_nice_gather(ctx->devs[dv], st.dev[dv], c, shares[dv], &launches[dv], st.square_ok,
                                          st.prefix_rejected, st.list, &ms, &mask_ms);
        if (rc) return drain_all(ctx, st.dev), rc;
        st.stats.launches += launches[dv];
        st.stats.kernel_ms = std::max(st.stats.kernel_ms, ms);
        if (c.prefix && !shares[dv].spans.empty()) {
            st.prefix.launches++;
            st.prefix.mask_ms = std::max(st.prefix.mask_ms, mask_ms);
        }
    }
    return NICE_OK;
}

}  // namespace

extern "C" {

int nice_debug_ranges_niceonly_plan(uint32_t base, uint32_t stride_k, const uint64_t *bounds, size_t n_ranges,
                                    uint32_t n_devices, uint64_t *leaves, size_t cap, size_t *n_out) {
    if (!bounds || !n_out || (cap && !leaves)) return fail(NICE_ERR_INVALID, "null argument");
    const uint32_t k = stride_k ? stride_k : 2;
    if (const char *why = nice::nice_ranges_check(base, n_ranges, k)) return fail(NICE_ERR_INVALID, why);
    if (n_devices < 1 || n_devices > 64) return fail(NICE_ERR_INVALID, "n_devices must be in 1..64");
    *n_out = 0;
    if (nice::residue_filter(base).empty()) return NICE_OK;
    const std::shared_ptr<nice::StrideTable> table = g_stride.get(base, k);
    if (table->residues.empty()) return NICE_OK;
    const nice::NiceRangesPlan pl = nice::plan_nice_ranges(base, k, *table, bounds, n_ranges, n_devices);
    if (!pl.error.empty()) return fail(NICE_ERR_INVALID, pl.error);
    *n_out = pl.leaves.size();
    for (size_t i = 0; i < pl.leaves.size() && i < cap; i++) {
        const nice::PlanLeaf &l = pl.leaves[i];
        uint64_t *o = leaves + 7 * i;
        o[0] = l.b0_lo, o[1] = l.b0_hi, o[2] = l.g0, o[3] = l.count, o[4] = l.range, o[5] = l.group, o[6] = l.device;
    }
    return NICE_OK;
}

int nice_last_ranges_niceonly_stats(nice_ctx *ctx, nice_ranges_niceonly_stats *out) {
    if (!ctx || !out) return fail(NICE_ERR_INVALID, "bad args");
    std::lock_guard<std::mutex> lock(ctx->ranges_nice_mu);
    *out = ctx->ranges_nice.stats;
    return NICE_OK;
}

int nice_last_ranges_niceonly_prefix(nice_ctx *ctx, nice_ranges_niceonly_prefix_stats *out) {
    if (!ctx || !out) return fail(NICE_ERR_INVALID, "bad args");
    std::lock_guard<std::mutex> lock(ctx->ranges_nice_mu);
    *out = ctx->ranges_nice.prefix;
    return NICE_OK;
}

int nice_process_ranges_niceonly_ex(nice_ctx *ctx, uint32_t base, const uint64_t *bounds, size_t n_ranges,
                                    const nice_ranges_niceonly_opts *opts, uint64_t *candidates, uint32_t *square_ok,
                                    uint64_t *prefix_rejected, nice_number *out, uint32_t *out_range, size_t cap,
                                    size_t *n_out) {
    if (!ctx || !bounds || (cap && !out)) return fail(NICE_ERR_INVALID, "null argument");
    const nice_ranges_niceonly_opts o = opts ? *opts : nice_ranges_niceonly_opts{};
    if (o.prefix_test > NICE_RANGES_PREFIX_ON)
        return fail(NICE_ERR_INVALID, "prefix_test must be NICE_RANGES_PREFIX_OFF or NICE_RANGES_PREFIX_ON");
    if (o.reserved[0] || o.reserved[1]) return fail(NICE_ERR_INVALID, "reserved option words must be zero");
    const bool prefix = o.prefix_test == NICE_RANGES_PREFIX_ON;
    const uint32_t k = o.stride_k ? o.stride_k : 2;
    if (const char *why = nice::nice_ranges_check(base, n_ranges, k)) return fail(NICE_ERR_INVALID, why);
    if (int rc = check_ranges(bounds, n_ranges)) return rc;
    std::lock_guard<std::mutex> lock(ctx->ranges_nice_mu);
    RangesNiceState &st = ctx->ranges_nice;
    const uint32_t key = k | (prefix ? kRangesPrefixKey : 0u);  // (k <= 32: the modulus fits a u32)
    if (st.holds(base, key, bounds, n_ranges))
        return ranges_nice_emit(st, candidates, square_ok, prefix_rejected, out, out_range, cap, n_out);
    st.begin(base, key, bounds, n_ranges);
    const size_t nd = ctx->devs.size();
    st.dev.resize(nd);
    st.stats = nice_ranges_niceonly_stats{};
    st.prefix = nice_ranges_niceonly_prefix_stats{};
    // as a field submitted now would take it: in range, the compile-time kernels
    const uint32_t hook = g_nice_min_override[base].load(std::memory_order_relaxed);
    st.nice_min = hook ? hook : base;
    st.candidates.assign(n_ranges, 0);
    st.square_ok.assign(n_ranges, 0);
    st.prefix_rejected.assign(n_ranges, 0);
    st.list.clear();
    NiceRangesCall c{base, k, st.nice_min, n_ranges, nullptr, false};
    // a residue-empty base (client_process_gpu.rs:525-531), or a table without
    // a residue: all-zero counts, an empty list, no launch
    if (!nice::residue_filter(base).empty()) c.table = g_stride.get(base, k);
    if (c.table && !c.table->residues.empty()) {
        const nice::NiceRangesPlan pl = nice::plan_nice_ranges(base, k, *c.table, bounds, n_ranges, nd);
        if (!pl.error.empty()) return fail(NICE_ERR_INVALID, pl.error);
        st.candidates = pl.candidates;
        st.stats.fast_ranges = pl.fast_ranges;
        st.stats.generic_ranges = pl.generic_ranges;
        st.stats.candidates = pl.total;
        // the test runs on the fast group (k = 2, so the table has its low masks)
        c.prefix = prefix && pl.fast_ranges && !c.table->lowmask.empty();
        if (c.prefix) st.prefix.prefix_ranges = pl.fast_ranges;
        std::vector<DevShare> shares(nd);
        for (size_t q = 0; q < pl.leaves.size(); q++) {
            const nice::PlanLeaf &l = pl.leaves[q];
            DevShare &sh = shares[l.device];
            uint32_t mask = 0;
            if (c.prefix && q < pl.n_fast_leaves) {
                // a range's pieces are consecutive leaves: one span per range and device
                if (sh.leaves.empty() || sh.leaves.back().range != l.range) {
                    const u128 first = nice::range_at(bounds, l.range, 0), last = nice::range_at(bounds, l.range, 1) - 1;
                    sh.spans.push_back(nice::RangeSpan{lo64(first), hi64(first), lo64(last), hi64(last)});
                }
                mask = (uint32_t)(sh.spans.size() - 1);
            }
            sh.leaves.push_back(nice::RangeLeaf{l.b0_lo, l.b0_hi, l.g0, l.count, l.range, mask});
            if (q < pl.n_fast_leaves) sh.n_fast++;
        }
        if (int rc = ranges_nice_run(ctx, st, c, shares)) return rc;
        // each range's numbers ascending, in range order (a range's pieces may
        // have run on several devices)
        std::sort(st.list.begin(), st.list.end(),
                  [](const Entry &a, const Entry &b) { return a.u != b.u ? a.u < b.u : a.n < b.n; });
        for (uint32_t v : st.square_ok) st.stats.square_ok += v;
        for (uint64_t v : st.prefix_rejected) st.prefix.rejected += v;
    }
    return ranges_nice_emit(st, candidates, square_ok, prefix_rejected, out, out_range, cap, n_out);
}

int nice_process_ranges_niceonly(nice_ctx *ctx, uint32_t base, const uint64_t *bounds, size_t n_ranges,
                                 uint32_t stride_k, uint64_t *candidates, uint32_t *square_ok, nice_number *out,
                                 uint32_t *out_range, size_t cap, size_t *n_out) {
    const nice_ranges_niceonly_opts o{stride_k, NICE_RANGES_PREFIX_OFF, {0, 0}};
    return nice_process_ranges_niceonly_ex(ctx, base, bounds, n_ranges, &o, candidates, square_ok, nullptr, out,
                                           out_range, cap, n_out);
}

}  // extern "C"
