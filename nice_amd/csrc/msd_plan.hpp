// msd_plan.hpp -- how a niceonly field's device MSD is cut into batches, how
// large its buffers are and how many workgroups each of its launches gets:
// pure arithmetic (no HIP), checked on its own by tests/test_msd_plan.py.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "layout.h"

namespace nice {

// Nodes per level of a fused chunk recursion (msd_fused_kernel; a power of
// two), or 0 when the chunk needs the level-launch BFS (chunk / floor too
// large, or chunk >= 2^32).
inline uint32_t msd_fused_cap(uint64_t chunk, uint64_t floor_size) {
    if (chunk > 0xffffffffull || floor_size == 0) return 0;
    const uint64_t need = chunk / floor_size + 2;
    if (need > kFusedMaxCap) return 0;
    uint32_t cap = 64;
    while (cap < need) cap <<= 1;
    return cap;
}
// ... and its workgroups: one per chunk of the batch (grid-strided past 4 per CU).
inline uint64_t msd_fused_grid(uint64_t chunks, int num_cus) { return std::min<uint64_t>(chunks, (uint64_t)num_cus * 4); }

// msd_wave_kernel: waves per workgroup, and the work stacks of `grid` workgroups.
inline uint32_t msd_wave_waves_per_group() { return kWaveWG / 64; }
inline size_t msd_wave_scratch_bytes(uint32_t grid) {
    return (size_t)grid * msd_wave_waves_per_group() * kStackCap * kStackNodeBytes;
}

// The last level of the level BFS that can hold a node that splits.  A node
// of level d has at most ceil(chunk / 2^d) numbers and splits only if it
// holds >= 2 * floor, so levels past the first d with ceil(chunk / 2^d) <
// 2 * floor are empty (b40 1e9 field, chunk 1e6, floor 250: levels 0..11
// instead of 0..22).
inline uint32_t msd_last_level(uint64_t chunk, uint64_t floor_size) {
    uint32_t last = 0;
    while (last < 22 && ((chunk + (1ull << last) - 1) >> last) >= 2 * floor_size) last++;
    return last;
}

// Workgroups (256 lanes, one per node) of msd_level_kernel at `level`: the
// level holds <= nchunks * 2^level nodes (the first levels are a few thousand
// lanes), capped at 2 per CU -- also when that product overflows.
inline uint32_t msd_level_grid(uint64_t nchunks, uint32_t level, int num_cus) {
    const uint64_t nodes = level < 40 ? nchunks << level : ~0ull;
    uint64_t grid = (nodes + 255) / 256;
    const uint64_t cap = (uint64_t)num_cus * 2;
    if (grid > cap || nodes >> level != nchunks) grid = cap;
    return (uint32_t)grid;
}

// Workgroups (4 waves) of niceonly_kernel: a wave per 8 leaves, or 32 waves
// per CU when the leaf count is on the device; at most `cap` (8 per CU; the
// probe build's NICE_NICE_GRID), at least 1.
inline uint32_t nice_grid(bool count_on_device, uint32_t n_leaves, int num_cus, uint64_t cap) {
    const uint64_t waves = count_on_device ? (uint64_t)num_cus * 32 : ((uint64_t)n_leaves + 7) / 8;
    uint64_t grid = (waves + 3) / 4;
    if (grid > cap) grid = cap;
    if (grid < 1) grid = 1;
    return (uint32_t)grid;
}

namespace abi __attribute__((visibility("hidden"))) {

struct MsdPlan {
    uint64_t cpb;        // chunks per batch
    uint64_t per;        // nodes per level queue
    uint64_t leaf_cap;   // leaf records per batch (level-BFS and fused paths)
    uint32_t fcap;       // nodes per level of a fused chunk recursion (0: not fused)
    bool wave;           // the level BFS down to wlevel, then msd_wave_kernel
    uint32_t wlevel;     // ... its root level
    uint32_t wgrid;      // ... its workgroups
    uint64_t wleaf_cap;  // ... leaf records of its BFS levels
    uint64_t nbatches;
    const char *error;   // null, or why the field cannot run on the device
};

// The probe build's overrides (NICE_MSD_CPB, NICE_MSD_NOWAVE, NICE_MSD_ROOTS;
// NICE_MSD_FCAP goes in as fused_cap); the product passes none.
struct MsdPlanKnobs {
    uint64_t cpb = 0;       // chunks per batch of the level-BFS and fused paths (0: the rule below)
    bool nowave = false;    // A/B: the level-BFS + leaf-list path for large chunks
    uint64_t roots = 2048;  // roots per wave
};

constexpr const char *kMsdChunkTooLarge = "device MSD: chunk_size too large";
constexpr const char *kMsdChunkTooLargeForFloor = "device MSD: chunk_size too large for the floor";

inline uint64_t nbatches_of(uint64_t chunks, uint64_t per_batch) { return (chunks + per_batch - 1) / per_batch; }

// chunk, floor_size: the field's MSD chunk size and recursion floor; mine: the
// caller's chunks (> 0); max_cus: the largest device; fused_cap:
// msd_fused_cap(chunk, floor_size), or the probe build's override;
// waves_per_group: msd_wave_waves_per_group().
inline MsdPlan plan_device_msd(unsigned __int128 chunk, uint64_t floor_size, uint64_t mine, size_t n_devices,
                               int max_cus, uint32_t fused_cap, uint32_t waves_per_group,
                               const MsdPlanKnobs &knobs = MsdPlanKnobs{}) {
    MsdPlan pl{};
    if (chunk > ((unsigned __int128)1 << 40)) {
        pl.error = kMsdChunkTooLarge;
        return pl;
    }
    const uint64_t cnk = (uint64_t)chunk;
    // Nodes per level and leaves per batch are <= batch / floor + chunks
    // (every split child holds >= floor numbers); size batches for 2^27
    // (16-byte nodes: 2 x 2 GB of level queues and 3 GB of leaf records at
    // most, allocated as a field needs them).  Batches are the unit of the
    // level launches, so larger ones amortise their fixed cost: the massive
    // field (chunk 1e8) took 0.365 s at 41 chunks per batch (2^24), 0.20 s
    // at 164, 0.17 s at 328 (profiles/r02/massive_batch_sweep.log).
    const uint64_t fl = std::min<uint64_t>(floor_size, 1ull << 30);
    uint64_t cpb = std::max<uint64_t>(1, (fl << 27) / cnk);
    if (knobs.cpb) cpb = knobs.cpb;
    cpb = std::min(cpb, mine);
    const uint64_t batch_n = cpb * cnk;
    uint64_t per = std::min<uint64_t>(batch_n / fl + cpb, cpb << 22) + 64;
    per = std::min<uint64_t>(per, 1ull << 28);  // (the bound above stays below this)
    // leaf records: one per range plus one per kLeafPiece candidates
    pl.leaf_cap = std::min<uint64_t>(per + (batch_n / kLeafPiece) + 64, 0xffffffffull);
    // Chunks whose recursion fits a workgroup run fused: one launch per
    // batch, one workgroup per chunk (grid-strided), no level queues.
    pl.fcap = fused_cap;
    // Chunks too large for the fused kernel: the level BFS only down to a
    // root level `wlevel` (nodes <= 2^26 numbers, ~2048 roots per wave of
    // the fused MSD + candidate kernel), then msd_wave_kernel.  Nothing of
    // a batch grows with its survivors any more (leaves are tested inside
    // the wave that finds them), so a batch is bounded only by the level
    // queues: 2^24 nodes at the root level.  The massive field is ONE
    // batch.
    pl.wave = !fused_cap && !knobs.nowave;
    if (pl.wave) {
        const int cus = std::max(256, max_cus);
        pl.wgrid = (uint32_t)cus * 16 / waves_per_group;  // 4 waves per SIMD
        // roots per wave: 2048 (the whole massive field 0.097 s at 32, 0.080 s
        // at 2048; a 1/8 dealt share 0.0135 / 0.0101 s, scripts/roots_sweep.py)
        const uint64_t waves = (uint64_t)pl.wgrid * waves_per_group;
        const uint64_t target = waves * knobs.roots;
        const uint32_t last = msd_last_level(cnk, fl);
        uint32_t wlevel = 0;
        while (wlevel < last && ((cnk + (1ull << wlevel) - 1) >> wlevel) > (1ull << 26)) wlevel++;
        for (;;) {
            // (a multi-device context gets at least one batch per device)
            const uint64_t per_dev = (mine + n_devices - 1) / n_devices;
            cpb = std::min<uint64_t>(per_dev, std::max<uint64_t>(1, (1ull << 24) >> wlevel));
            if ((cpb << wlevel) >= target || wlevel >= last) break;
            wlevel++;
        }
        if (((cnk + (1ull << wlevel) - 1) >> wlevel) > (1ull << 26)) {
            pl.error = kMsdChunkTooLargeForFloor;
            return pl;
        }
        pl.wlevel = wlevel;
        per = (cpb << wlevel) + 64;
        // leaves of the BFS levels (clipped / depth-limited nodes), in pieces
        pl.wleaf_cap = per * (1 + (fl >> 28)) + 64;
    }
    pl.cpb = cpb;
    pl.per = per;
    pl.nbatches = nbatches_of(mine, cpb);
    return pl;
}

}  // namespace abi
}  // namespace nice
