// unique_map.h -- host-side launch entry points of the per-number unique-count
// map (fd2_map_kernel, fd2_map_kernel.hpp; generic_map_kernel, detailed.hip),
// implemented in fd2_detailed.hip / fd2_map_part.hip / detailed.hip and used
// by abi_map.cpp.  The plan they take is fd2_map_plan.hpp's.
#pragma once

#include <hip/hip_runtime.h>

#include "fd2_map_plan.hpp"

namespace nice {

constexpr size_t kMapDescBytes = 80;  // device descriptor per FD record (Fd2MapUnit)

// What map_plan needs to know about `base` (the valid range, the FD kernel's
// cuts, the map kernel's workgroup size and target chunk).
MapBase map_base(uint32_t base);

struct MapLaunch {
    uint32_t base;
    const MapRec *recs;      // host; ascending n
    size_t n_recs;
    void *h_desc, *d_desc;   // pinned staging / device array, kMapDescBytes per FD record
    uint8_t *out;            // device memory; a record writes out[rec.off ...)
    uint32_t *launches;      // if set, incremented per kernel launch enqueued
};
// Copies the FD records' descriptors (async, on s) and enqueues one launch per
// run of FD records of one limb layout and one per generic record.
hipError_t launch_unique_map(const MapLaunch &p, hipStream_t s);
// out[i] = the unique-digit count of start + i, i < count <= 2^32: any base
// 2..128, any n < 2^128 (one thread per n, the generic device function).
hipError_t launch_generic_map(uint64_t start_lo, uint64_t start_hi, uint64_t count, uint32_t base, uint8_t *out,
                              hipStream_t s);

}  // namespace nice
