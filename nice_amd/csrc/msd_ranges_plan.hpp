// msd_ranges_plan.hpp -- how nice_msd_ranges cuts a call's roots into devices,
// batches and kernel forms, and how large a batch's buffers are: pure
// arithmetic (no HIP), beside msd_plan.hpp, checked on its own by
// tests/test_msd_ranges.py and tests/msd_ranges_san.cpp.
//
// A root is one recursion root (depth 0, depth cap 22, factor 2).  A node
// splits only if it holds >= 2 floor numbers and a level-22 node is a leaf, so
// a root of s numbers has at most min(s / floor + 1, 2^22) leaves and as many
// nodes per level: msd_ranges_bound.  Every buffer of a batch is sized from the
// sum of its roots' bounds, so no valid call overflows one.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "host_math.hpp"
#include "msd_plan.hpp"

namespace nice {

constexpr size_t kMsdRangesMaxRoots = (size_t)1 << 20;   // the key's 20 root bits
constexpr uint64_t kMsdRangesMaxNumbers = 1ull << 40;    // ... and its 40 offset bits
constexpr uint32_t kMsdRangesOffBits = 40;
// Nodes (and leaf records) of one batch: 16 bytes each in two level queues,
// the record list and the sort's second buffer -- 8 GB at most, allocated as
// a call needs them.  A root's bound is <= 2^22, so a batch holds >= 32 roots.
// The bound is loose where the filter prunes well (the massive b50 field's 1e8
// chunks at floor 250: 400 001 against ~1 600 ranges), and a batch's level
// launches are then short and bound by launch latency, so batches are large:
// 2^25 nodes took 15.0 ms of recursion on a 1e12 slice of that field
// (profiles/msd_ranges/ranges_batch25.jsonl).
constexpr uint64_t kMsdRangesBatchNodes = 1ull << 27;

inline uint64_t msd_ranges_bound(uint64_t size, uint64_t floor_size) {
    return std::min<uint64_t>(size / floor_size + 1, 1ull << 22);
}

// Form 1 (one workgroup per root, msd_ranges_fused_kernel) for roots whose
// levels fit kFusedMaxCap nodes, form 0 (the level BFS) for the rest.
inline uint32_t msd_ranges_group(uint64_t size, uint64_t floor_size) { return msd_fused_cap(size, floor_size) ? 1u : 0u; }

struct MsdRangesRoot {
    uint32_t group, device, batch;  // batch: counted per device
    uint64_t size;
};
struct MsdRangesPlan {
    std::vector<MsdRangesRoot> roots;   // one per root of the call, in its order
    std::vector<uint32_t> first;        // per device: its first root (n_devices + 1 entries)
    std::vector<uint32_t> nbatches;     // per device
    std::string error;                  // empty, or why the call is refused
};

// What nice_msd_ranges, its CPU twin and the plan hook refuse alike.
inline std::string msd_ranges_check(uint32_t base, const uint64_t *roots, size_t n_roots, uint64_t floor_size) {
    if (base < 2 || base > 128) return "base must be in 2..128";
    if (n_roots == 0 || n_roots > kMsdRangesMaxRoots) return "n_roots must be in 1..2^20";
    if (floor_size == 0) return "floor_size must be at least 1";
    for (size_t i = 0; i < n_roots; i++) {
        if (!range_proper(roots, i)) return "root " + std::to_string(i) + " is empty or inverted";
        if (range_at(roots, i, 1) - range_at(roots, i, 0) > kMsdRangesMaxNumbers)
            return "root " + std::to_string(i) + " holds more than 2^40 numbers";
    }
    return "";
}

// Devices take contiguous runs of roots balanced by numbers (root i goes where
// the numbers before it fall in the call's total); within a device batches are
// contiguous runs whose bounds sum to <= kMsdRangesBatchNodes.
inline MsdRangesPlan plan_msd_ranges(uint32_t base, const uint64_t *roots, size_t n_roots, uint64_t floor_size,
                                     size_t n_devices) {
    MsdRangesPlan pl;
    pl.error = msd_ranges_check(base, roots, n_roots, floor_size);
    if (pl.error.empty() && (n_devices < 1 || n_devices > 64)) pl.error = "n_devices must be in 1..64";
    if (!pl.error.empty()) return pl;
    pl.roots.resize(n_roots);
    u128 total = 0;
    for (size_t i = 0; i < n_roots; i++) {
        pl.roots[i].size = (uint64_t)(range_at(roots, i, 1) - range_at(roots, i, 0));
        total += pl.roots[i].size;
    }
    pl.first.assign(n_devices + 1, (uint32_t)n_roots);
    pl.nbatches.assign(n_devices, 0);
    u128 before = 0;
    uint64_t in_batch = 0;
    uint32_t dev = 0, batch = 0;
    pl.first[0] = 0;
    for (size_t i = 0; i < n_roots; i++) {
        MsdRangesRoot &r = pl.roots[i];
        const uint32_t d = (uint32_t)(before * n_devices / total);  // before < total: d < n_devices
        if (d != dev) {
            for (uint32_t q = dev + 1; q <= d; q++) pl.first[q] = (uint32_t)i;
            dev = d, batch = 0, in_batch = 0;
        }
        const uint64_t b = msd_ranges_bound(r.size, floor_size);
        if (in_batch && in_batch + b > kMsdRangesBatchNodes) batch++, in_batch = 0;
        in_batch += b;
        r.group = msd_ranges_group(r.size, floor_size);
        r.device = dev;
        r.batch = batch;
        pl.nbatches[dev] = batch + 1;
        before += r.size;
    }
    return pl;
}

}  // namespace nice
