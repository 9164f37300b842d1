// fd2_map_plan.hpp -- how nice_unique_map (abi_map.cpp) turns [start, end)
// into launches: pure arithmetic (no HIP), checked on its own by
// tests/test_map.py through nice_debug_map_plan and by tests/map_san.cpp.
//
// The range is cut at the ends of the base's valid range and, inside it, at
// the FD kernel's limb-layout cuts (fd2_cuts, what nice_fd_segment_cuts
// reports).  A piece inside the valid range of a base with an FD kernel
// becomes workgroup descriptors of fd2_map_kernel (fd2_map_kernel.hpp), tiled
// as the batch plan tiles a range (fd2_plan.hpp batch_tile): main workgroups
// of up to `wg` lanes walking `chunk` <= tchunk <= B numbers each, then at
// most one tail workgroup with the < chunk numbers left over, one per lane.
// Everything else -- a base without an FD kernel, the parts of the range
// outside the valid range -- becomes one generic segment per piece
// (generic_map_kernel, detailed.hip).  Every record carries the output offset
// of its first number, n - start (+ off0, the range's own offset in a larger
// map: a device's shard).  The records come out in ascending n and cover
// [start, end) exactly once.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "fd2_plan.hpp"
#include "layout.h"

namespace nice {

constexpr u128 kMapMaxNumbers = (u128)1 << 32;  // numbers per nice_unique_map call

enum : uint32_t { kMapFd = 0, kMapGeneric = 1 };

struct MapRec {
    uint64_t lo, hi;   // first n
    uint64_t off;      // output offset of the first n
    uint32_t lanes;    // FD: active lanes (<= wg); generic: 0
    uint32_t chunk;    // FD: numbers per lane (<= B; 1 for a tail workgroup); generic: 0
    uint32_t combo;    // FD: index of the cut interval (the limb layout); generic: 0
    uint32_t kind;     // kMapFd, kMapGeneric
    uint64_t count;    // numbers the record covers (FD: lanes * chunk)
};

// What the plan needs to know about a base.
struct MapBase {
    bool fd = false;            // the base has an FD kernel and a valid range
    u128 rs = 0, re = 0;        // the valid range (fd only)
    std::vector<u128> cuts;     // limb-layout cuts, ascending (fd only)
    uint64_t wg = 512;          // workgroup size of the base's map kernel
    uint64_t tchunk = 81;       // target chunk, odd, <= B
};

struct MapPlan {
    std::vector<MapRec> recs;
    uint32_t fd_segments = 0, generic_segments = 0;
    uint64_t fd_numbers = 0, generic_numbers = 0;
};

inline void map_plan_generic(u128 s, u128 e, u128 start, uint64_t off0, MapPlan &pl) {
    if (s >= e) return;
    pl.recs.push_back(MapRec{(uint64_t)s, (uint64_t)(s >> 64), off0 + (uint64_t)(s - start), 0u, 0u, 0u,
                             kMapGeneric, (uint64_t)(e - s)});
    pl.generic_segments++;
    pl.generic_numbers += (uint64_t)(e - s);
}

// The plan of [start, end) (start < end, at most kMapMaxNumbers numbers),
// appended to pl.
inline void map_plan(const MapBase &b, u128 start, u128 end, uint64_t off0, MapPlan &pl) {
    if (!b.fd || end <= b.rs || start >= b.re) {
        map_plan_generic(start, end, start, off0, pl);
        return;
    }
    const u128 fs = start > b.rs ? start : b.rs, fe = end < b.re ? end : b.re;
    map_plan_generic(start, fs, start, off0, pl);
    u128 a = fs;
    for (size_t i = 0; i <= b.cuts.size() && a < fe; i++) {
        const u128 stop = i < b.cuts.size() && b.cuts[i] < fe ? b.cuts[i] : fe;
        if (stop <= a) continue;
        const fd2::BatchTile tile = fd2::batch_tile(stop - a, b.wg, b.tchunk);
        u128 units = tile.units, n = a;
        while (units) {
            const uint64_t lanes = units < b.wg ? (uint64_t)units : b.wg;
            pl.recs.push_back(MapRec{(uint64_t)n, (uint64_t)(n >> 64), off0 + (uint64_t)(n - start), (uint32_t)lanes,
                                     (uint32_t)tile.chunk, (uint32_t)i, kMapFd, lanes * tile.chunk});
            n += (u128)lanes * tile.chunk;
            units -= lanes;
        }
        if (tile.tail)
            pl.recs.push_back(MapRec{(uint64_t)n, (uint64_t)(n >> 64), off0 + (uint64_t)(n - start),
                                     (uint32_t)tile.tail, 1u, (uint32_t)i, kMapFd, tile.tail});
        pl.fd_segments++;
        pl.fd_numbers += (uint64_t)(stop - a);
        a = stop;
    }
    map_plan_generic(fe, end, start, off0, pl);
}

}  // namespace nice
