// msd_plan.hpp -- how a niceonly field's device MSD is cut into batches and
// how large its buffers are: pure arithmetic (no HIP), so it can be checked
// on its own.
#pragma once

#include <stdint.h>

#include <algorithm>

#include "layout.h"

namespace nice {
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
// msd_fused_cap(chunk, floor_size); waves_per_group: msd_wave_waves_per_group().
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
        uint32_t last = 0;  // first level without splits
        while (last < 22 && ((cnk + (1ull << last) - 1) >> last) >= 2 * fl) last++;
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
