// abi_hooks.cpp -- the C ABI's debug and check hooks: per-n device
// diagnostics, host restatements of the fast-base device functions, the MSD
// filter and stride tables, and the test knobs of the detailed paths.
#include "abi_internal.hpp"
#include "niceonly_bases.h"
#include "radix_fast.hpp"

using namespace nice::abi;
using nice::u128;

namespace {

// The bases with niceonly fast paths (niceonly_bases.h, the one list).
#define NICE_FAST_BASES(X) NICE_NICEONLY_BASES(X)

// The valid range of a niceonly fast base (false: not one).
bool fast_base_range(uint32_t base, u128 &rs, u128 &re) {
    return nice::niceonly_fast_base(base) && nice::base_range_cached(base, rs, re) == 1;
}

template <int B>
int prefix_reject_host(u128 s, u128 l, u128 n) {
    constexpr int MW = nice::Radix<B>::MW;
    uint32_t pm[MW] = {}, low[MW];
    const uint32_t multi = l > s ? 1u : 0u;
    if (multi && nice::msd_prefix_masks<B>(lo64(s), hi64(s), lo64(l), hi64(l), pm))
        for (int w = 0; w < MW; w++) pm[w] = ~0u;  // the prefix repeats: every candidate goes
    const uint32_t dup = nice::low_digit_mask(B, (uint32_t)(n % ((uint32_t)B * B)), low, MW);
    return nice::prefix_rejects<MW>(pm, multi, low, dup) ? 1 : 0;
}

// One u32 per n from a diagnostic kernel, on device 0.
template <class Launch>
int debug_per_n(nice_ctx *ctx, const uint64_t *n_pairs, uint32_t count, uint32_t *out, Launch launch) {
    if (count == 0) return NICE_OK;
    Device &d = ctx->devs[0];
    HIPCHK(hipSetDevice(d.id));
    uint64_t *dn;
    uint32_t *du;
    HIPCHK(hipMalloc(&dn, (size_t)count * 16));
    HIPCHK(hipMalloc(&du, (size_t)count * 4));
    HIPCHK(hipMemcpy(dn, n_pairs, (size_t)count * 16, hipMemcpyHostToDevice));
    HIPCHK(launch(dn, du, d.slot[0].stream));
    HIPCHK(hipStreamSynchronize(d.slot[0].stream));
    HIPCHK(hipMemcpy(out, du, (size_t)count * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipFree(dn));
    HIPCHK(hipFree(du));
    return NICE_OK;
}

}  // namespace

extern "C" {

int nice_validate_detailed(uint32_t base, uint64_t size_lo, uint64_t size_hi, const uint64_t *hist,
                           const nice_number *list, size_t n) {
    if (base < 2 || base > 128 || !hist || (n && !list)) return fail(NICE_ERR_INVALID, "bad args");
    // the server's cutoff, whatever nice_debug_set_near_miss_cutoff has set
    const int rc = validate_detailed(base, nice::near_miss_cutoff(base), mk(size_lo, size_hi), hist, n, [&](size_t i) {
        return Entry{mk(list[i].number_lo, list[i].number_hi), list[i].num_uniques};
    });
    return rc ? NICE_ERR_INVALID : NICE_OK;
}

int nice_debug_unique_counts(nice_ctx *ctx, const uint64_t *n_pairs, uint32_t count,
                             uint32_t base, uint32_t *out) {
    if (!ctx || base < 2 || base > 128) return fail(NICE_ERR_INVALID, "bad args");
    return debug_per_n(ctx, n_pairs, count, out, [&](const uint64_t *dn, uint32_t *du, hipStream_t s) {
        return nice::launch_unique_counts(dn, count, base, du, s);
    });
}

int nice_debug_is_nice(nice_ctx *ctx, const uint64_t *n_pairs, uint32_t count, uint32_t base,
                       uint32_t *out) {
    if (!ctx || base < 2 || base > 128) return fail(NICE_ERR_INVALID, "bad args");
    return debug_per_n(ctx, n_pairs, count, out, [&](const uint64_t *dn, uint32_t *du, hipStream_t s) {
        return nice::launch_is_nice(dn, count, base, du, s);
    });
}

int nice_debug_unique_fast(nice_ctx *ctx, const uint64_t *n_pairs, uint32_t count, uint32_t base,
                           uint32_t *out) {
    u128 rs, re;
    if (!ctx || !fast_base_range(base, rs, re))
        return fail(NICE_ERR_INVALID, "base without a niceonly fast path");
    for (uint32_t i = 0; i < count; i++) {
        const u128 n = mk(n_pairs[2 * i], n_pairs[2 * i + 1]);
        if (n < rs || n >= re) return fail(NICE_ERR_INVALID, "n outside the base's valid range");
    }
    return debug_per_n(ctx, n_pairs, count, out, [&](const uint64_t *dn, uint32_t *du, hipStream_t s) {
        return nice::launch_unique_fast(dn, count, base, du, s);
    });
}

int nice_debug_cube_count(nice_ctx *ctx, const uint64_t *n_pairs, uint32_t count, uint32_t base,
                          uint32_t *out) {
    u128 rs, re;
    if (!ctx || !fast_base_range(base, rs, re))
        return fail(NICE_ERR_INVALID, "base without a niceonly fast path");
    for (uint32_t i = 0; i < count; i++) {
        const u128 n = mk(n_pairs[2 * i], n_pairs[2 * i + 1]);
        if (n < rs || n >= re) return fail(NICE_ERR_INVALID, "n outside the base's valid range");
    }
    return debug_per_n(ctx, n_pairs, count, out, [&](const uint64_t *dn, uint32_t *du, hipStream_t s) {
        return nice::launch_cube_count(dn, count, base, du, s);
    });
}

int nice_check_is_nice_inrange(uint32_t base, uint64_t lo, uint64_t hi) {
    u128 rs, re;
    const u128 n = mk(lo, hi);
    if (!fast_base_range(base, rs, re) || n < rs || n >= re)
        return fail(NICE_ERR_INVALID, "n outside the base's valid range (or base without a niceonly fast path)");
    switch (base) {
#define X(b) case b: return nice::is_nice_fast<b>(lo, hi) ? 1 : 0;
        NICE_FAST_BASES(X)
#undef X
    default: return NICE_ERR_INVALID;
    }
}

int nice_check_unique_inrange(uint32_t base, uint64_t lo, uint64_t hi) {
    u128 rs, re;
    const u128 n = mk(lo, hi);
    if (!fast_base_range(base, rs, re) || n < rs || n >= re)
        return fail(NICE_ERR_INVALID, "n outside the base's valid range (or base without a niceonly fast path)");
    switch (base) {
#define X(b) case b: return (int)nice::unique_fast<b>(lo, hi);
        NICE_FAST_BASES(X)
#undef X
    default: return NICE_ERR_INVALID;
    }
}

int nice_check_msd_skippable_inrange(uint32_t base, uint64_t slo, uint64_t shi, uint64_t elo,
                                     uint64_t ehi) {
    u128 rs, re;
    const u128 s = mk(slo, shi), e = mk(elo, ehi);
    if (!fast_base_range(base, rs, re) || s < rs || e > re || s >= e)
        return fail(NICE_ERR_INVALID, "range outside the base's valid range (or base without a niceonly fast path)");
    if (e - s == 1) return 0;  // a single number is never skipped (msd_prefix_filter.rs:395)
    const u128 l = e - 1;
    const uint64_t llo = lo64(l), lhi = hi64(l);
    switch (base) {
#define X(b) case b: return nice::msd_skippable_fast<b>(slo, shi, llo, lhi) ? 1 : 0;
        NICE_FAST_BASES(X)
#undef X
    default: return NICE_ERR_INVALID;
    }
}

int nice_check_prefix_reject_inrange(uint32_t base, uint64_t slo, uint64_t shi, uint64_t elo, uint64_t ehi,
                                     uint64_t nlo, uint64_t nhi) {
    u128 rs, re;
    const u128 s = mk(slo, shi), e = mk(elo, ehi), n = mk(nlo, nhi);
    if (!fast_base_range(base, rs, re) || s < rs || e > re || n < s || n >= e)
        return fail(NICE_ERR_INVALID, "leaf or n outside the base's valid range (or base without a niceonly fast path)");
    switch (base) {
#define X(b) case b: return prefix_reject_host<b>(s, e - 1, n);
        NICE_FAST_BASES(X)
#undef X
    default: return NICE_ERR_INVALID;
    }
}

int nice_fd_segment_cuts(uint32_t base, uint64_t *out, size_t cap, size_t *n_out) {
    std::vector<u128> c(8);
    const size_t n = nice::fd2_cuts(base, c.data(), c.size());
    for (size_t i = 0; i < n && i < cap; i++) {
        out[2 * i] = lo64(c[i]);
        out[2 * i + 1] = hi64(c[i]);
    }
    if (n_out) *n_out = n;
    return NICE_OK;
}

int nice_msd_skippable(uint64_t slo, uint64_t shi, uint64_t elo, uint64_t ehi, uint32_t base) {
    if (base < 2 || base > 128 || mk(slo, shi) >= mk(elo, ehi)) return fail(NICE_ERR_INVALID, "bad args");
    return nice::make_msd(base)->skippable(mk(slo, shi), mk(elo, ehi)) ? 1 : 0;
}

int nice_msd_valid_ranges(uint64_t slo, uint64_t shi, uint64_t elo, uint64_t ehi, uint32_t base,
                          uint64_t floor_size, uint64_t *out, size_t cap, size_t *n_out) {
    return nice_msd_valid_ranges_ex(slo, shi, elo, ehi, base, floor_size, NICE_FILTER_REFERENCE, out, cap, n_out);
}

int nice_msd_valid_ranges_ex(uint64_t slo, uint64_t shi, uint64_t elo, uint64_t ehi, uint32_t base,
                             uint64_t floor_size, uint32_t filter, uint64_t *out, size_t cap, size_t *n_out) {
    if (base < 2 || base > 128 || mk(slo, shi) >= mk(elo, ehi) || filter > NICE_FILTER_SOUND)
        return fail(NICE_ERR_INVALID, "bad args");
    std::vector<std::pair<u128, u128>> rs;
    nice::make_msd(base)->ranges(mk(slo, shi), mk(elo, ehi), floor_size, rs, filter == NICE_FILTER_SOUND);
    size_t n = rs.size();
    for (size_t i = 0; i < n && i < cap; i++) {
        out[4 * i] = lo64(rs[i].first);
        out[4 * i + 1] = hi64(rs[i].first);
        out[4 * i + 2] = lo64(rs[i].second);
        out[4 * i + 3] = hi64(rs[i].second);
    }
    *n_out = n;
    return n > cap ? fail(NICE_ERR_CAPACITY, "range list exceeds capacity") : NICE_OK;
}

int nice_stride_table(uint32_t base, uint32_t k, uint64_t *modulus, uint32_t *residues,
                      size_t cap, size_t *n_out) {
    if (base < 3 || base > 128 || k > 3) return fail(NICE_ERR_INVALID, "bad args");
    auto t = g_stride.get(base, k);
    *modulus = t->modulus;
    *n_out = t->residues.size();
    for (size_t i = 0; i < std::min(cap, t->residues.size()); i++) residues[i] = t->residues[i];
    return t->residues.size() > cap && residues ? fail(NICE_ERR_CAPACITY, "capacity") : NICE_OK;
}

int nice_debug_force_sib_stride(uint32_t L) {
    if (L && (L % 2 == 0 || L > 255))
        return fail(NICE_ERR_INVALID, "sibling lane stride must be odd and <= 255 (0: the production pick)");
    nice::fd2_force_sib_stride(L);
    return NICE_OK;
}

int nice_debug_force_sib_persistent(uint32_t mode, uint32_t max_workgroups) {
    if (mode > 2) return fail(NICE_ERR_INVALID, "mode must be 0 (production), 1 (persistent) or 2 (rounds)");
    nice::fd2_force_sib_persistent(mode, max_workgroups);
    return NICE_OK;
}

int nice_debug_fd_window(uint32_t base, uint32_t *w0, uint32_t *w) {
    if (!w0 || !w) return fail(NICE_ERR_INVALID, "null argument");
    if (!nice::fd2_window(base, w0, w)) return fail(NICE_ERR_INVALID, "base has no FD kernel");
    return NICE_OK;
}

int nice_debug_set_near_miss_cutoff(uint32_t base, uint32_t cutoff) {
    uint32_t w0 = 0, w = 0;
    if (!nice::fd2_window(base, &w0, &w)) return fail(NICE_ERR_INVALID, "base has no FD kernel");
    // the FD launchers take any cutoff at or above the top of the histogram
    // window; at cutoff >= base nothing would be listed
    if (cutoff && (cutoff + 1 < w0 + w || cutoff >= base))
        return fail(NICE_ERR_INVALID, "cutoff must be 0 (production) or in [" + std::to_string(w0 + w - 1) + ", " +
                                          std::to_string(base - 1) + "]");
    g_cutoff_override[base].store(cutoff, std::memory_order_relaxed);
    return NICE_OK;
}

int nice_debug_set_nice_min(uint32_t base, uint32_t nice_min) {
    if (!nice::niceonly_fast_base(base)) return fail(NICE_ERR_INVALID, "base without a niceonly fast path");
    if (nice_min > base)
        return fail(NICE_ERR_INVALID, "nice_min must be 0 (production) or in [1, " + std::to_string(base) + "]");
    g_nice_min_override[base].store(nice_min, std::memory_order_relaxed);
    return NICE_OK;
}

}  // extern "C"
