// abi_ranges.cpp -- batched detailed ranges (nice_process_ranges_detailed):
// many small ranges in one launch per limb layout and device.
#include <cstring>

#include "abi_internal.hpp"

using namespace nice::abi;
using nice::kHistBins;
using nice::kHistCopies;
using nice::u128;

namespace {

constexpr size_t kRangesMax = (size_t)1 << 20;
// One pass = one batch (a launch per limb layout present) on one device: at
// most kPassUnits workgroups (20 MB of descriptors) for kPassRanges ranges
// (17 MB of rows).  A range's workgroups may continue in the next pass.
constexpr size_t kPassUnits = (size_t)1 << 18, kPassRanges = (size_t)1 << 14;
// A longer range fills the chip on its own: it runs as a field (and its plan
// would not be worth holding: one 32-byte unit per ~4e4 numbers).
constexpr u128 kBatchRangeMax = (u128)1 << 28;

struct PassRange {
    size_t ri;    // range index of the call
    u128 ps, pe;  // the part of the range this pass's workgroups cover
};
struct Pass {
    std::vector<nice::BatchUnit> units;
    std::vector<PassRange> pr;  // row k of the pass
};

// A call's ranges and where its results gather.
struct RangesCall {
    uint32_t base;
    const uint64_t *bounds;
    size_t n_ranges;
    bool sum;
    std::vector<std::vector<Entry>> per;  // the listed numbers of each range
};

}  // namespace

void nice::abi::ranges_dev_free(Device &d, RangesDev &r) {
    if (!r.side.stream) return;
    (void)r.side.drain(d);
    r.desc.free();
    if (r.d_rows) (void)hipFree(r.d_rows);
    if (r.list.n) (void)hipFree(r.list.n);
    if (r.list.u) (void)hipFree(r.list.u);
    if (r.chk_u) (void)hipFree(r.chk_u);
    r.side.destroy(d);
}

namespace {

// Enqueue one pass (async on the device's batch stream).
int ranges_enqueue(Device &d, RangesDev &r, const Pass &p, uint32_t base, bool sum, uint32_t *launches) {
    HIPCHK(hipSetDevice(d.id));
    const size_t nu = p.units.size();
    const size_t nrows = sum ? kHistCopies : p.pr.size();
    if (int rc = r.desc.ensure(nu, nice::kBatchDescBytes)) return rc;
    if (r.rows_cap < nrows) {
        const size_t c = std::max<size_t>(nrows, 1024);
        if (int rc = grow_device(r.d_rows, r.rows_cap, c, c * kHistBins * 8 + 16)) return rc;
        r.d_count = (uint32_t *)(r.d_rows + c * kHistBins);
    }
    int rc = ensure_listbuf(d, r.list, std::max<uint32_t>(r.list.cap, 4096), true);
    if (rc) return rc;
    const hipStream_t stream = r.side.stream;
    HIPCHK(hipMemsetAsync(r.d_rows, 0, nrows * kHistBins * 8, stream));
    HIPCHK(hipMemsetAsync(r.d_count, 0, 4, stream));
    nice::BatchLaunch b{};
    b.base = base;
    b.cutoff = effective_cutoff(base);
    b.units = p.units.data();
    b.n_units = nu;
    b.h_desc = r.desc.h;
    b.d_desc = r.desc.d;
    b.hist = r.d_rows;
    b.ncopies = sum ? (uint32_t)kHistCopies : 0u;
    b.out = nice::NumOut{r.list.n, r.list.u, r.d_count, r.list.cap};
    b.launches = launches;
    HIPCHK(hipEventRecord(r.side.ev0, stream));
    const hipError_t err = nice::launch_detailed_fd2_batch(b, stream);
    if (err != hipSuccess) return fail(NICE_ERR_HIP, std::string("batch launch: ") + hipGetErrorString(err));
    HIPCHK(hipEventRecord(r.side.ev1, stream));
    return NICE_OK;
}

// Wait for a pass and read its results: rows (nrows x kHistBins) and the
// list, sorted by n with repeats (overlapping ranges) removed.
int ranges_gather(Device &d, RangesDev &r, const Pass &p, uint32_t base, bool sum, uint32_t *launches,
                  std::vector<uint64_t> &rows, std::vector<Entry> &list, double *ms) {
    HIPCHK(hipSetDevice(d.id));
    const size_t nrows = sum ? kHistCopies : p.pr.size();
    const hipStream_t stream = r.side.stream;
    uint32_t cnt = 0;
    for (int attempt = 0;; attempt++) {
        HIPCHK(hipMemcpyAsync(&cnt, r.d_count, 4, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (cnt <= r.list.cap) break;
        // the device list overflowed: grow it and run the pass again
        if (attempt) return fail(NICE_ERR_HIP, "near-miss list overflow after resize");
        int rc = ensure_listbuf(d, r.list, (cnt + 4095u) & ~4095u, true);
        *launches = 0;
        if (!rc) rc = ranges_enqueue(d, r, p, base, sum, launches);
        if (rc) return rc;
    }
    float t = 0;
    HIPCHK(r.side.elapsed(&t));
    *ms += t;
    rows.resize(nrows * kHistBins);
    HIPCHK(hipMemcpyAsync(rows.data(), r.d_rows, nrows * kHistBins * 8, hipMemcpyDeviceToHost, stream));
    list.clear();
    if (cnt) {
        if (r.chk_cap < cnt)
            if (int rc = grow_device(r.chk_u, r.chk_cap, r.list.cap, (size_t)r.list.cap * 4)) return rc;
        // self-check: every listed number's unique count recomputed by the
        // generic per-n device function
        std::vector<uint64_t> nbuf;
        std::vector<uint32_t> ubuf, chk(cnt);
        const hipError_t err = nice::launch_unique_counts(r.list.n, cnt, base, r.chk_u, stream);
        if (err != hipSuccess) return fail(NICE_ERR_HIP, std::string("self-check: ") + hipGetErrorString(err));
        if (int rc = read_list(r.list, cnt, nbuf, ubuf, stream)) return rc;
        HIPCHK(hipMemcpyAsync(chk.data(), r.chk_u, (size_t)cnt * 4, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        list.reserve(cnt);
        for (uint32_t q = 0; q < cnt; q++) {
            if (chk[q] != ubuf[q])
                return fail(NICE_ERR_HIP, "self-check: unique count of a listed number does not recompute");
            list.push_back({mk(nbuf[2 * q], nbuf[2 * q + 1]), ubuf[q]});
        }
        std::sort(list.begin(), list.end(), [](const Entry &a, const Entry &b) { return a.n < b.n; });
        list.erase(std::unique(list.begin(), list.end(), [](const Entry &a, const Entry &b) { return a.n == b.n; }),
                   list.end());
    } else {
        HIPCHK(hipStreamSynchronize(stream));
    }
    return NICE_OK;
}

int ranges_emit(RangesState &st, uint64_t *hist, nice_number *out, uint32_t *out_range, size_t cap,
                size_t *n_out) {
    std::memcpy(hist, st.hist.data(), st.hist.size() * 8);
    if (int rc = st.fits(cap, n_out)) return rc;
    for (size_t i = 0; i < st.list.size(); i++) {
        put_entry(out[i], st.list[i]);
        if (out_range) out_range[i] = st.list_range[i];
    }
    st.drop();
    st.hist = {};
    st.list_range = {};
    return NICE_OK;
}

int ranges_check_args(uint32_t base, const uint64_t *bounds, size_t n_ranges) {
    if (base < 2 || base > 128) return fail(NICE_ERR_INVALID, "base must be in 2..=128");
    if (n_ranges == 0 || n_ranges > kRangesMax) return fail(NICE_ERR_INVALID, "n_ranges must be in 1..2^20");
    return check_ranges(bounds, n_ranges);
}

// Whether [s, e) runs in the batch: inside the valid range of an FD base.
bool ranges_batchable(uint32_t base, u128 s, u128 e) {
    u128 rs = 0, re = 0;
    return nice::fd2_supported(base) && nice::base_range_cached(base, rs, re) == 1 && s >= rs && e <= re &&
           e - s <= kBatchRangeMax;
}

// The batch: ranges dealt to the nd devices in contiguous groups balanced by
// numbers (batch_total in all), each device's group cut into passes.
std::vector<std::vector<Pass>> ranges_plan_passes(const RangesCall &c, const std::vector<size_t> &batch,
                                                  u128 batch_total, size_t nd) {
    std::vector<std::vector<Pass>> passes(nd);
    std::vector<nice::BatchUnit> tmp;
    u128 before = 0;
    std::vector<Pass> cur(nd);
    for (size_t i : batch) {
        const u128 s = nice::range_at(c.bounds, i, 0), e = nice::range_at(c.bounds, i, 1);
        size_t dv = batch_total ? (size_t)(before * nd / batch_total) : 0;
        if (dv >= nd) dv = nd - 1;
        before += e - s;
        tmp.clear();
        nice::fd2_batch_plan(c.base, s, e, 0, tmp);
        size_t k = 0;
        while (k < tmp.size()) {
            Pass &p = cur[dv];
            if (p.units.size() >= kPassUnits || p.pr.size() >= kPassRanges) {
                passes[dv].push_back(std::move(p));
                p = Pass{};
            }
            const size_t take = std::min(tmp.size() - k, kPassUnits - p.units.size());
            const uint32_t row = (uint32_t)p.pr.size();
            const nice::BatchUnit &f = tmp[k], &l = tmp[k + take - 1];
            p.pr.push_back({i, mk(f.lo, f.hi), mk(l.lo, l.hi) + (u128)l.lanes * l.chunk});
            for (size_t j = 0; j < take; j++) {
                p.units.push_back(tmp[k + j]);
                p.units.back().row = row;
            }
            k += take;
        }
    }
    for (size_t dv = 0; dv < nd; dv++)
        if (!cur[dv].units.empty()) passes[dv].push_back(std::move(cur[dv]));
    return passes;
}

// Run the passes, one per device at a time, and add their rows and lists to
// st.hist and c.per.
int ranges_run_rounds(nice_ctx *ctx, RangesState &st, RangesCall &c, const std::vector<std::vector<Pass>> &passes) {
    const size_t nb = c.base + 1, nd = ctx->devs.size();
    size_t rounds = 0;
    for (auto &p : passes) rounds = std::max(rounds, p.size());
    std::vector<double> ms(nd, 0.0);
    std::vector<uint64_t> rows;
    std::vector<Entry> list;
    for (size_t r = 0; r < rounds; r++) {
        std::vector<uint32_t> launches(nd, 0);
        for (size_t dv = 0; dv < nd; dv++) {
            if (r >= passes[dv].size()) continue;
            int rc = st.dev[dv].side.init(ctx->devs[dv]);
            if (!rc) rc = ranges_enqueue(ctx->devs[dv], st.dev[dv], passes[dv][r], c.base, c.sum, &launches[dv]);
            if (rc) return drain_all(ctx, st.dev), rc;
        }
        for (size_t dv = 0; dv < nd; dv++) {
            if (r >= passes[dv].size()) continue;
            const Pass &p = passes[dv][r];
            int rc = ranges_gather(ctx->devs[dv], st.dev[dv], p, c.base, c.sum, &launches[dv], rows, list, &ms[dv]);
            if (rc) return drain_all(ctx, st.dev), rc;  // the other devices' passes
            st.stats.launches += launches[dv];
            if (c.sum) {
                for (size_t cp = 0; cp < kHistCopies; cp++)
                    for (size_t b = 0; b < nb; b++) st.hist[b] += rows[cp * kHistBins + b];
            }
            for (size_t k = 0; k < p.pr.size(); k++) {
                const PassRange &q = p.pr[k];
                if (!c.sum)
                    for (size_t b = 0; b < nb; b++) st.hist[q.ri * nb + b] += rows[k * kHistBins + b];
                auto lo = std::lower_bound(list.begin(), list.end(), q.ps,
                                           [](const Entry &a, u128 v) { return a.n < v; });
                auto hi = std::lower_bound(lo, list.end(), q.pe, [](const Entry &a, u128 v) { return a.n < v; });
                c.per[q.ri].insert(c.per[q.ri].end(), lo, hi);
            }
        }
    }
    for (double m : ms) st.stats.kernel_ms = std::max(st.stats.kernel_ms, m);
    return NICE_OK;
}

// Everything else: range by range as fields.
int ranges_fallback(nice_ctx *ctx, RangesState &st, RangesCall &c, const std::vector<size_t> &fallback) {
    const size_t nb = c.base + 1;
    std::vector<uint64_t> row(kHistBins);
    std::vector<nice_number> one(64);
    for (size_t i : fallback) {
        size_t n = 0;
        const uint64_t *b = c.bounds + 4 * i;
        int rc = nice_process_range_detailed(ctx, b[0], b[1], b[2], b[3], c.base, row.data(), one.data(), one.size(),
                                             &n);
        if (rc == NICE_ERR_CAPACITY) {
            one.resize(n);
            rc = nice_process_range_detailed(ctx, b[0], b[1], b[2], b[3], c.base, row.data(), one.data(),
                                             one.size(), &n);
        }
        if (rc) return rc;
        for (size_t u = 0; u < nb; u++) st.hist[(c.sum ? 0 : i * nb) + u] += row[u];
        for (size_t j = 0; j < n; j++)
            c.per[i].push_back({mk(one[j].number_lo, one[j].number_hi), one[j].num_uniques});
    }
    return NICE_OK;
}

// The list in range order, and the self-check of every row (`total`: the
// numbers of all ranges).
int ranges_assemble(RangesState &st, const RangesCall &c, u128 total) {
    const size_t nb = c.base + 1;
    st.list.clear();
    st.list_range.clear();
    for (size_t i = 0; i < c.n_ranges; i++) {
        if (!c.sum) {
            const u128 size = nice::range_at(c.bounds, i, 1) - nice::range_at(c.bounds, i, 0);
            int rc = validate_detailed(c.base, effective_cutoff(c.base), size, &st.hist[i * nb], c.per[i].size(),
                                       [&](size_t j) { return c.per[i][j]; });
            if (rc) return fail(rc, "range " + std::to_string(i) + ": " + nice_last_error());
        }
        st.list.insert(st.list.end(), c.per[i].begin(), c.per[i].end());
        st.list_range.insert(st.list_range.end(), c.per[i].size(), (uint32_t)i);
    }
    if (c.sum)
        return validate_detailed(c.base, effective_cutoff(c.base), total, st.hist.data(), st.list.size(),
                                 [&](size_t j) { return st.list[j]; });
    return NICE_OK;
}

}  // namespace

extern "C" {

int nice_debug_ranges_plan(uint32_t base, const uint64_t *bounds, size_t n_ranges, uint64_t *units, size_t cap,
                           size_t *n_out) {
    if (!bounds || !n_out || (cap && !units)) return fail(NICE_ERR_INVALID, "null argument");
    if (int rc = ranges_check_args(base, bounds, n_ranges)) return rc;
    if (!nice::fd2_supported(base)) return fail(NICE_ERR_INVALID, "base has no FD kernel");
    u128 rs = 0, re = 0;
    nice::base_range_cached(base, rs, re);
    std::vector<nice::BatchUnit> v;
    size_t n = 0;
    for (size_t i = 0; i < n_ranges; i++) {
        const u128 s = nice::range_at(bounds, i, 0), e = nice::range_at(bounds, i, 1);
        if (s < rs || e > re)
            return fail(NICE_ERR_INVALID, "range " + std::to_string(i) + " is not inside the base's valid range");
        v.clear();
        nice::fd2_batch_plan(base, s, e, (uint32_t)i, v);
        for (const nice::BatchUnit &u : v) {
            if (n < cap) {
                uint64_t *o = units + 6 * n;
                o[0] = u.lo, o[1] = u.hi, o[2] = u.lanes, o[3] = u.chunk, o[4] = u.row, o[5] = u.combo;
            }
            n++;
        }
    }
    *n_out = n;
    return NICE_OK;
}

int nice_last_ranges_stats(nice_ctx *ctx, nice_ranges_stats *out) {
    if (!ctx || !out) return fail(NICE_ERR_INVALID, "bad args");
    std::lock_guard<std::mutex> lock(ctx->ranges_mu);
    *out = ctx->ranges.stats;
    return NICE_OK;
}

int nice_process_ranges_detailed(nice_ctx *ctx, uint32_t base, const uint64_t *bounds, size_t n_ranges,
                                 uint32_t flags, uint64_t *hist, nice_number *out, uint32_t *out_range, size_t cap,
                                 size_t *n_out) {
    if (!ctx || !bounds || !hist || (cap && !out)) return fail(NICE_ERR_INVALID, "null argument");
    if (flags > NICE_RANGES_SUM) return fail(NICE_ERR_INVALID, "bad flags");
    if (int rc = ranges_check_args(base, bounds, n_ranges)) return rc;
    std::lock_guard<std::mutex> lock(ctx->ranges_mu);
    RangesState &st = ctx->ranges;
    if (st.holds(base, flags, bounds, n_ranges)) return ranges_emit(st, hist, out, out_range, cap, n_out);
    st.begin(base, flags, bounds, n_ranges);
    RangesCall c{base, bounds, n_ranges, flags == NICE_RANGES_SUM, std::vector<std::vector<Entry>>(n_ranges)};
    const size_t nb = base + 1, nd = ctx->devs.size();
    st.dev.resize(nd);
    st.stats = nice_ranges_stats{};
    st.hist.assign(c.sum ? nb : n_ranges * nb, 0);
    std::vector<size_t> batch, fallback;
    u128 total = 0, batch_total = 0;
    for (size_t i = 0; i < n_ranges; i++) {
        const u128 s = nice::range_at(c.bounds, i, 0), e = nice::range_at(c.bounds, i, 1);
        total += e - s;
        if (ranges_batchable(base, s, e)) batch.push_back(i), batch_total += e - s;
        else fallback.push_back(i);
    }
    st.stats.numbers = total > (u128)UINT64_MAX ? UINT64_MAX : (uint64_t)total;
    st.stats.fallback_ranges = (uint32_t)fallback.size();
    int rc = ranges_run_rounds(ctx, st, c, ranges_plan_passes(c, batch, batch_total, nd));
    if (!rc) rc = ranges_fallback(ctx, st, c, fallback);
    if (!rc) rc = ranges_assemble(st, c, total);
    if (rc) return rc;
    return ranges_emit(st, hist, out, out_range, cap, n_out);
}

}  // extern "C"
