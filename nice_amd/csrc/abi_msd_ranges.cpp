// abi_msd_ranges.cpp -- the device MSD recursion's range list
// (nice_msd_ranges): many roots per call, each root's surviving ranges out, in
// the layout nice_msd_valid_ranges writes.  The plan (devices, batches, kernel
// form per root) is msd_ranges_plan.hpp's, the kernels msd_ranges.hpp's.  A
// batch runs its groups -- one or many workgroup-per-root launches, the level
// BFS -- into one record list, orders the records by (root, offset) with the
// device sort and copies back only the records written; the host expands
// them to quadruples.
#include <cstring>

#include "abi_internal.hpp"
#include "msd_ranges_plan.hpp"
#include "niceonly_bases.h"

using namespace nice::abi;
using nice::u128;

namespace {

constexpr uint32_t kCtlWords = nice::kMsdOverflow + 1;  // level sizes, record count, overflow flag

int msd_ranges_dev_init(Device &d, MsdRangesDev &r) {
    if (r.side.stream) return NICE_OK;
    if (int rc = r.side.init(d)) return rc;
    HIPCHK(hipEventCreate(&r.so0));
    HIPCHK(hipEventCreate(&r.so1));
    HIPCHK(hipMalloc(&r.d_ctl, kCtlWords * 4));
    HIPCHK(hipHostMalloc(&r.h_ctl, 2 * 4, hipHostMallocDefault));
    return NICE_OK;
}

}  // namespace

void nice::abi::msd_ranges_dev_free(Device &d, MsdRangesDev &r) {
    if (!r.side.stream) return;
    (void)r.side.drain(d);
    r.roots.free();
    r.lists.free();
    for (auto &q : r.q)
        if (q) (void)hipFree(q);
    if (r.rec) (void)hipFree(r.rec);
    if (r.scratch) (void)hipFree(r.scratch);
    if (r.sort_tmp) (void)hipFree(r.sort_tmp);
    if (r.d_ctl) (void)hipFree(r.d_ctl);
    if (r.h_ctl) (void)hipHostFree(r.h_ctl);
    if (r.h_rec) (void)hipHostFree(r.h_rec);
    if (r.so0) (void)hipEventDestroy(r.so0);
    if (r.so1) (void)hipEventDestroy(r.so1);
    r.side.destroy(d);
}

namespace {

// What a call runs with, resolved once.
struct MsdRangesCall {
    uint32_t base;
    bool sound, fast_base;
    uint64_t floor_size;
    const uint64_t *roots;
    u128 rs, re;  // the base's valid range (re == 0: none)
};

// A batch of a device: roots [first, last) of the call.
struct Batch {
    uint32_t first = 0, last = 0;
    uint32_t count = 0;  // records written
};

bool root_in_range(const MsdRangesCall &c, size_t i) {
    return c.re != 0 && c.rs <= nice::range_at(c.roots, i, 0) && nice::range_at(c.roots, i, 1) <= c.re;
}

// Enqueue a batch's recursion (async on the device's stream): the roots and
// the group lists staged, the counters zeroed, each group present launched,
// the record count copied to pinned memory.
int msd_ranges_enqueue(Device &d, MsdRangesDev &r, const MsdRangesCall &c, const nice::MsdRangesPlan &pl,
                       const Batch &b, nice_msd_ranges_stats &st) {
    HIPCHK(hipSetDevice(d.id));
    const hipStream_t stream = r.side.stream;
    const uint32_t n = b.last - b.first;
    // groups: form (1: a workgroup per root) x placement (1: the base's compile-time kernels)
    std::vector<uint32_t> list[2][2];
    uint64_t max_size[2][2] = {{0, 0}, {0, 0}};
    uint64_t rec_need = 0, q_need = 0;
    if (int rc = r.roots.ensure(n, sizeof(nice::MsdRangeRoot), stream)) return rc;
    if (int rc = r.lists.ensure(n, 4, stream)) return rc;
    nice::MsdRangeRoot *hr = (nice::MsdRangeRoot *)r.roots.h;
    for (uint32_t i = 0; i < n; i++) {
        const size_t gi = b.first + i;
        const u128 s = nice::range_at(c.roots, gi, 0);
        const bool in = root_in_range(c, gi);
        const uint64_t size = pl.roots[gi].size;
        hr[i] = nice::MsdRangeRoot{lo64(s), hi64(s), size, in ? 1u : 0u, 0};
        // the field kernels' placement: the reference filter's compile-time
        // kernels take every field of a fast base, the sound ones in-range fields
        const bool fast = c.fast_base && (!c.sound || in);
        const uint32_t form = pl.roots[gi].group;
        list[form][fast].push_back(i);
        max_size[form][fast] = std::max(max_size[form][fast], size);
        const uint64_t bound = nice::msd_ranges_bound(size, c.floor_size);
        rec_need += bound;
        if (!form) q_need += bound;
        (form ? st.fused_roots : st.level_roots)++;
    }
    if (r.rec_cap < rec_need) {
        const size_t cap = std::max<size_t>(rec_need, 1 << 16);
        if (int rc = grow_device(r.rec, r.rec_cap, cap, cap * 32, stream)) return rc;
    }
    if (q_need && r.q_cap < q_need + 64) {
        const size_t cap = std::max<size_t>(q_need + 64, 1 << 16);
        size_t c0 = 0;
        if (int rc = grow_device(r.q[0], c0, cap, cap * sizeof(nice::MsdNode), stream)) return rc;
        r.q_cap = 0;
        if (int rc = grow_device(r.q[1], r.q_cap, cap, cap * sizeof(nice::MsdNode))) return rc;
    }
    uint32_t fcap[2] = {0, 0}, fgrid[2] = {0, 0};
    size_t scratch_need = 0;
    for (int fast = 0; fast < 2; fast++) {
        if (list[1][fast].empty()) continue;
        fcap[fast] = nice::msd_fused_cap(max_size[1][fast], c.floor_size);
        fgrid[fast] = (uint32_t)nice::msd_fused_grid(list[1][fast].size(), d.num_cus);
        scratch_need = std::max(scratch_need, (size_t)fgrid[fast] * 2 * fcap[fast]);
    }
    if (r.scratch_nodes < scratch_need)
        if (int rc = grow_device(r.scratch, r.scratch_nodes, scratch_need, scratch_need * sizeof(nice::ChunkNode), stream))
            return rc;
    uint32_t *hl = (uint32_t *)r.lists.h;
    size_t at = 0, off[2][2];
    for (int form = 0; form < 2; form++)
        for (int fast = 0; fast < 2; fast++) {
            off[form][fast] = at;
            std::copy(list[form][fast].begin(), list[form][fast].end(), hl + at);
            at += list[form][fast].size();
        }
    HIPCHK(hipMemcpyAsync(r.roots.d, r.roots.h, (size_t)n * sizeof(nice::MsdRangeRoot), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(r.lists.d, r.lists.h, (size_t)n * 4, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemsetAsync(r.d_ctl, 0, kCtlWords * 4, stream));
    nice::MsdRangesLaunch p{};
    p.roots = (const nice::MsdRangeRoot *)r.roots.d;
    p.floor_size = c.floor_size;
    p.q[0] = r.q[0];
    p.q[1] = r.q[1];
    p.q_cap = (uint32_t)std::min<size_t>(r.q_cap, 0xffffffffu);
    p.ctl = r.d_ctl;
    p.keys = r.rec;
    p.sizes = r.rec + r.rec_cap;
    p.leaf_cap = (uint32_t)std::min<size_t>(r.rec_cap, 0xffffffffu);
    HIPCHK(hipEventRecord(r.side.ev0, stream));
    for (int form = 1; form >= 0; form--)
        for (int fast = 1; fast >= 0; fast--) {
            if (list[form][fast].empty()) continue;
            p.list = (const uint32_t *)r.lists.d + off[form][fast];
            p.n = (uint32_t)list[form][fast].size();
            const hipError_t err =
                nice::launch_msd_ranges(p, c.base, fast != 0, c.sound, max_size[form][fast], d.num_cus, stream,
                                        form ? r.scratch : nullptr, fcap[fast], fgrid[fast], &st.launches);
            if (err != hipSuccess) return fail(NICE_ERR_HIP, std::string("msd ranges launch: ") + hipGetErrorString(err));
        }
    HIPCHK(hipEventRecord(r.side.ev1, stream));
    HIPCHK(hipMemcpyAsync(r.h_ctl, r.d_ctl + nice::kMsdLeafCount, 2 * 4, hipMemcpyDeviceToHost, stream));
    return NICE_OK;
}

// Wait for a batch's recursion, order its records on the device and copy the
// ones written back to the pinned staging (async: read after the next drain).
int msd_ranges_order(Device &d, MsdRangesDev &r, Batch &b, double *kernel_ms) {
    HIPCHK(hipSetDevice(d.id));
    const hipStream_t stream = r.side.stream;
    HIPCHK(hipStreamSynchronize(stream));
    if (r.h_ctl[1] || r.h_ctl[0] > r.rec_cap)
        return fail(NICE_ERR_MSD_OVERFLOW, "msd ranges: a queue sized from the leaf bound overflowed");
    float t = 0;
    HIPCHK(r.side.elapsed(&t));
    *kernel_ms += t;
    b.count = r.h_ctl[0];
    if (r.h_rec_cap < b.count) {
        const size_t cap = std::max<size_t>(b.count, 1 << 16);
        if (int rc = grow_pinned(r.h_rec, r.h_rec_cap, cap, cap * 16)) return rc;
    }
    HIPCHK(hipEventRecord(r.so0, stream));
    if (b.count) {
        size_t bytes = 0;
        hipError_t err = nice::msd_ranges_sort_bytes(b.count, &bytes);
        if (err == hipSuccess && r.sort_bytes < bytes) {
            if (int rc = grow_device(r.sort_tmp, r.sort_bytes, bytes, bytes)) return rc;
        }
        uint64_t *k = r.rec, *s = r.rec + r.rec_cap, *ko = r.rec + 2 * r.rec_cap, *so = r.rec + 3 * r.rec_cap;
        if (err == hipSuccess) err = nice::msd_ranges_sort(r.sort_tmp, r.sort_bytes, k, ko, s, so, b.count, stream);
        if (err != hipSuccess) return fail(NICE_ERR_HIP, std::string("msd ranges sort: ") + hipGetErrorString(err));
        HIPCHK(hipEventRecord(r.so1, stream));
        HIPCHK(hipMemcpyAsync(r.h_rec, ko, (size_t)b.count * 8, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(r.h_rec + r.h_rec_cap, so, (size_t)b.count * 8, hipMemcpyDeviceToHost, stream));
    } else {
        HIPCHK(hipEventRecord(r.so1, stream));
    }
    return NICE_OK;
}

// A batch's ordered records as list entries (the start and the root) and
// sizes; counted per root and summed on the way.
int msd_ranges_expand(const MsdRangesCall &c, const Batch &b, const uint64_t *keys, const uint64_t *sizes,
                      std::vector<Entry> &list, std::vector<uint64_t> &out_sizes, std::vector<uint64_t> &counts,
                      uint64_t *numbers) {
    const uint64_t mask = (1ull << nice::kMsdRangesOffBits) - 1;
    const size_t need = list.size() + b.count;
    if (list.capacity() < need) list.reserve(std::max(need, 2 * list.capacity()));
    out_sizes.insert(out_sizes.end(), sizes, sizes + b.count);
    for (uint32_t q = 0; q < b.count; q++) {
        const uint64_t root = b.first + (keys[q] >> nice::kMsdRangesOffBits);
        if (root >= b.last) return fail(NICE_ERR_HIP, "self-check: a record's root index is out of bounds");
        list.push_back(Entry{nice::range_at(c.roots, root, 0) + (keys[q] & mask), (uint32_t)root});
        counts[root]++;
        *numbers += sizes[q];
    }
    return NICE_OK;
}

int msd_ranges_emit(MsdRangesState &st, uint64_t *out, uint32_t *out_root, uint64_t *counts, size_t cap,
                    size_t *n_out) {
    if (counts) std::memcpy(counts, st.counts.data(), st.counts.size() * 8);
    if (int rc = st.fits(cap, n_out)) return rc;
    for (size_t i = 0; i < st.list.size(); i++) {
        const u128 a = st.list[i].n, e = a + st.sizes[i];
        out[4 * i] = lo64(a), out[4 * i + 1] = hi64(a), out[4 * i + 2] = lo64(e), out[4 * i + 3] = hi64(e);
        if (out_root) out_root[i] = st.list[i].u;
    }
    st.drop();
    st.sizes = {};
    st.counts = {};
    return NICE_OK;
}

// Every device's batches: batch k of all devices enqueued, then ordered, then
// expanded, so the devices run side by side.
int msd_ranges_run(nice_ctx *ctx, MsdRangesState &st, const MsdRangesCall &c, const nice::MsdRangesPlan &pl) {
    const size_t nd = ctx->devs.size();
    std::vector<std::vector<Batch>> batches(nd);
    size_t most = 0;
    for (size_t dv = 0; dv < nd; dv++) {
        batches[dv].resize(pl.nbatches[dv]);
        for (uint32_t i = pl.first[dv]; i < pl.first[dv + 1]; i++) {
            Batch &b = batches[dv][pl.roots[i].batch];
            if (b.last == 0) b.first = i;
            b.last = i + 1;
        }
        most = std::max(most, batches[dv].size());
    }
    std::vector<std::vector<Entry>> lists(nd);
    std::vector<std::vector<uint64_t>> szs(nd);
    std::vector<double> kernel_ms(nd, 0), order_ms(nd, 0);
    for (size_t k = 0; k < most; k++) {
        for (size_t dv = 0; dv < nd; dv++) {
            if (k >= batches[dv].size()) continue;
            int rc = msd_ranges_dev_init(ctx->devs[dv], st.dev[dv]);
            if (!rc) rc = msd_ranges_enqueue(ctx->devs[dv], st.dev[dv], c, pl, batches[dv][k], st.stats);
            if (rc) return drain_all(ctx, st.dev), rc;
        }
        for (size_t dv = 0; dv < nd; dv++) {
            if (k >= batches[dv].size()) continue;
            const int rc = msd_ranges_order(ctx->devs[dv], st.dev[dv], batches[dv][k], &kernel_ms[dv]);
            if (rc) return drain_all(ctx, st.dev), rc;
        }
        for (size_t dv = 0; dv < nd; dv++) {
            if (k >= batches[dv].size()) continue;
            const hipError_t err = st.dev[dv].side.drain(ctx->devs[dv]);
            float t = 0;
            if (err != hipSuccess || hipEventElapsedTime(&t, st.dev[dv].so0, st.dev[dv].so1) != hipSuccess)
                return drain_all(ctx, st.dev), fail(NICE_ERR_HIP, "msd ranges: the copy back failed");
            order_ms[dv] += t;
            const MsdRangesDev &r = st.dev[dv];
            if (int rc = msd_ranges_expand(c, batches[dv][k], r.h_rec, r.h_rec + r.h_rec_cap, lists[dv], szs[dv],
                                           st.counts, &st.stats.numbers))
                return rc;
        }
    }
    for (size_t dv = 0; dv < nd; dv++) {
        if (st.list.empty()) {  // (one device: no copy)
            st.list.swap(lists[dv]);
            st.sizes.swap(szs[dv]);
        } else {
            st.list.insert(st.list.end(), lists[dv].begin(), lists[dv].end());
            st.sizes.insert(st.sizes.end(), szs[dv].begin(), szs[dv].end());
        }
        lists[dv] = {};
        szs[dv] = {};
        st.stats.kernel_ms = std::max(st.stats.kernel_ms, kernel_ms[dv]);
        st.stats.order_ms = std::max(st.stats.order_ms, order_ms[dv]);
    }
    return NICE_OK;
}

}  // namespace

extern "C" {

int nice_debug_msd_ranges_plan(uint32_t base, const uint64_t *roots, size_t n_roots, uint64_t floor_size,
                               uint32_t n_devices, uint64_t *records, size_t cap, size_t *n_out) {
    if (!roots || !n_out || (cap && !records)) return fail(NICE_ERR_INVALID, "null argument");
    const nice::MsdRangesPlan pl = nice::plan_msd_ranges(base, roots, n_roots, floor_size, n_devices);
    if (!pl.error.empty()) return fail(NICE_ERR_INVALID, pl.error);
    *n_out = pl.roots.size();
    for (size_t i = 0; i < pl.roots.size() && i < cap; i++) {
        uint64_t *o = records + 4 * i;
        o[0] = i, o[1] = pl.roots[i].group, o[2] = pl.roots[i].device, o[3] = pl.roots[i].batch;
    }
    return NICE_OK;
}

int nice_last_msd_ranges_stats(nice_ctx *ctx, nice_msd_ranges_stats *out) {
    if (!ctx || !out) return fail(NICE_ERR_INVALID, "bad args");
    std::lock_guard<std::mutex> lock(ctx->msd_ranges_mu);
    *out = ctx->msd_ranges.stats;
    return NICE_OK;
}

int nice_msd_ranges(nice_ctx *ctx, uint32_t base, const uint64_t *roots, size_t n_roots, uint64_t floor_size,
                    uint32_t filter, uint64_t *out, uint32_t *out_root, uint64_t *counts, size_t cap,
                    size_t *n_out) {
    if (!ctx || !roots || !n_out || (cap && !out)) return fail(NICE_ERR_INVALID, "null argument");
    if (filter > NICE_FILTER_SOUND)
        return fail(NICE_ERR_INVALID, "filter must be NICE_FILTER_REFERENCE or NICE_FILTER_SOUND");
    {
        const std::string why = nice::msd_ranges_check(base, roots, n_roots, floor_size);
        if (!why.empty()) return fail(NICE_ERR_INVALID, why);
    }
    std::lock_guard<std::mutex> lock(ctx->msd_ranges_mu);
    MsdRangesState &st = ctx->msd_ranges;
    if (st.holds(base, filter, roots, n_roots) && st.floor_size == floor_size)
        return msd_ranges_emit(st, out, out_root, counts, cap, n_out);
    st.begin(base, filter, roots, n_roots);
    st.floor_size = floor_size;
    const size_t nd = ctx->devs.size();
    st.dev.resize(nd);
    st.stats = nice_msd_ranges_stats{};
    st.list.clear();
    st.sizes.clear();
    const nice::MsdRangesPlan pl = nice::plan_msd_ranges(base, roots, n_roots, floor_size, nd);
    if (!pl.error.empty()) return fail(NICE_ERR_INVALID, pl.error);
    MsdRangesCall c{base, filter == NICE_FILTER_SOUND, nice::niceonly_fast_base(base), floor_size, roots, 0, 0};
    if (nice::base_range_cached(base, c.rs, c.re) != 1) c.rs = c.re = 0;
    st.counts.assign(n_roots, 0);
    if (int rc = msd_ranges_run(ctx, st, c, pl)) return rc;
    st.stats.ranges = st.list.size();
    return msd_ranges_emit(st, out, out_root, counts, cap, n_out);
}

}  // extern "C"
