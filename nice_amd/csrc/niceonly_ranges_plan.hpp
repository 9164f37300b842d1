// niceonly_ranges_plan.hpp -- how nice_process_ranges_niceonly turns a call's
// ranges into leaf records, which kernel each range runs and which device
// each leaf goes to: pure arithmetic (no HIP), checked on its own by
// tests/test_ranges_niceonly.py through nice_debug_ranges_niceonly_plan.
//
// A range becomes one leaf record per kLeafPiece candidates, as flush_ranges
// (abi_niceonly.cpp) makes them for the host MSD producer, plus its range
// index: the cycle base start - start mod M, g0 = lower_bound(residues, start
// mod M) and the count.  Ranges fall into two groups: a niceonly fast base's
// ranges wholly inside its valid range on the k = 2 table run the base's
// compile-time kernel (in_range = 1, square_ok counted), the rest the
// run-time-base kernel (in_range = 0).  Each group's leaves are dealt to the
// devices in contiguous runs balanced by candidate count: at most two launches
// per device.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "host_math.hpp"
#include "layout.h"

namespace nice {

constexpr size_t kNiceRangesMax = (size_t)1 << 20;       // ranges per call
constexpr u128 kNiceRangeCandMax = (u128)1 << 40;        // candidates per range
constexpr size_t kNiceRangesLeafMax = (size_t)1 << 24;   // leaf records per call
// The compile-time kernel's survivor ring carries a leaf's range index above
// its n's high word: in range n_hi < 2^kRangeIdShift (b80, the largest fast
// base, ends at 80^16 < 2^102).
constexpr uint32_t kRangeIdShift = 40;
static_assert(kNiceRangesMax <= ((size_t)1 << (64 - kRangeIdShift)), "a range index fits above the high word");

struct PlanLeaf {
    uint64_t b0_lo, b0_hi;
    uint32_t g0, count;
    uint32_t range;   // range index of the call
    uint32_t group;   // 1: compile-time kernel (fast, in range), 0: run-time base
    uint32_t device;  // index among the context's devices
};

struct NiceRangesPlan {
    std::vector<PlanLeaf> leaves;       // the fast group's, then the generic group's; range order in each
    size_t n_fast_leaves = 0;           // leaves[0, n_fast_leaves) are the fast group
    std::vector<uint64_t> candidates;   // per range
    std::vector<uint8_t> fast;          // per range: its group
    uint32_t fast_ranges = 0, generic_ranges = 0;
    uint64_t total = 0;                 // candidates of the call
    std::string error;                  // non-empty: the call is invalid
};

// The stride modulus (b - 1) * b^k (k > 0), or 0 when it does not fit a u32.
inline uint64_t nice_ranges_modulus(uint32_t base, uint32_t k) {
    uint64_t m = base - 1;
    for (uint32_t i = 0; i < k; i++) {
        m *= base;
        if (m > 0xffffffffull) return 0;
    }
    return m;
}

// What both the GPU call and its CPU twin refuse before looking at a range;
// null when the arguments pass.
inline const char *nice_ranges_check(uint32_t base, size_t n_ranges, uint32_t k) {
    if (base < 2 || base > 128) return "base must be in 2..=128";
    if (n_ranges == 0 || n_ranges > kNiceRangesMax) return "n_ranges must be in 1..2^20";
    if (k == 0 || nice_ranges_modulus(base, k) == 0) return "stride modulus exceeds u32";
    return nullptr;
}

// Whether [s, e) runs the compile-time kernel of `base` on the k table.
inline bool nice_range_fast(uint32_t base, uint32_t k, u128 s, u128 e) {
    if (k != 2 || !niceonly_fast_base(base)) return false;
    u128 rs = 0, re = 0;
    return base_range_cached(base, rs, re) == 1 && rs <= s && e <= re && !(e >> (64 + kRangeIdShift));
}

// The leaves of one group (`want_fast`) appended in range order, then dealt:
// the leaf whose first candidate is number `before` of the group's `total`
// goes to device before * nd / total.
inline void plan_group(const StrideTable &t, const uint64_t *bounds, size_t n_ranges, bool want_fast, size_t nd,
                       NiceRangesPlan &pl) {
    const size_t R = t.residues.size();
    const size_t first = pl.leaves.size();
    u128 total = 0;
    for (size_t i = 0; i < n_ranges; i++) {
        if ((pl.fast[i] != 0) != want_fast) continue;
        const u128 start = range_at(bounds, i, 0);
        const u128 i0 = t.index_of(start), i1 = t.index_of(range_at(bounds, i, 1));
        for (u128 g = i0; g < i1; g += kLeafPiece) {
            // candidate g of the global residue sequence: (g / R) * M + res[g % R].
            // The first piece keeps the range's own cycle, start - start mod M,
            // so its g0 is R when start mod M lies above the last residue.
            const u128 cyc = g == i0 ? start / t.modulus : g / R;
            const u128 bs = cyc * t.modulus;
            const uint32_t cnt = (uint32_t)std::min<u128>(kLeafPiece, i1 - g);
            pl.leaves.push_back(PlanLeaf{(uint64_t)bs, (uint64_t)(bs >> 64), (uint32_t)(g - cyc * R), cnt,
                                         (uint32_t)i, want_fast ? 1u : 0u, 0u});
            total += cnt;
        }
    }
    u128 before = 0;
    for (size_t q = first; q < pl.leaves.size(); q++) {
        size_t dv = total ? (size_t)(before * nd / total) : 0;
        if (dv >= nd) dv = nd - 1;
        pl.leaves[q].device = (uint32_t)dv;
        before += pl.leaves[q].count;
    }
}

// The plan of a call (bounds already checked non-null; t: the base's table
// for k, with at least one residue).  pl.error names what makes it invalid.
inline NiceRangesPlan plan_nice_ranges(uint32_t base, uint32_t k, const StrideTable &t, const uint64_t *bounds,
                                       size_t n_ranges, size_t n_devices) {
    NiceRangesPlan pl;
    if (n_devices < 1) n_devices = 1;
    pl.candidates.assign(n_ranges, 0);
    pl.fast.assign(n_ranges, 0);
    size_t n_leaves = 0;
    for (size_t i = 0; i < n_ranges; i++) {
        const u128 s = range_at(bounds, i, 0), e = range_at(bounds, i, 1);
        if (!range_proper(bounds, i)) {
            pl.error = range_refusal(i);
            return pl;
        }
        const u128 c = t.index_of(e) - t.index_of(s);
        if (c > kNiceRangeCandMax) {
            pl.error = "range " + std::to_string(i) + " holds more than 2^40 candidates: use a field";
            return pl;
        }
        pl.candidates[i] = (uint64_t)c;
        pl.total += (uint64_t)c;
        n_leaves += (size_t)((c + kLeafPiece - 1) / kLeafPiece);
        if (n_leaves > kNiceRangesLeafMax) {
            pl.error = "the call needs more than 2^24 leaf records: use fields";
            return pl;
        }
        pl.fast[i] = nice_range_fast(base, k, s, e) ? 1 : 0;
        if (pl.fast[i]) pl.fast_ranges++;
        else pl.generic_ranges++;
    }
    pl.leaves.reserve(n_leaves);
    plan_group(t, bounds, n_ranges, true, n_devices, pl);
    pl.n_fast_leaves = pl.leaves.size();
    plan_group(t, bounds, n_ranges, false, n_devices, pl);
    return pl;
}

}  // namespace nice
