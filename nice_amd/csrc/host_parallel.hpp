// host_parallel.hpp -- what the niceonly pipeline takes from
// host_parallel.cpp (plain host code, no HIP).
#pragma once

#include <stdint.h>

#include "../../include/nice_hip.h"

namespace nice {
namespace abi __attribute__((visibility("hidden"))) {

// Rust's std::thread::available_parallelism: the affinity mask capped by the
// cgroup v2 CPU quota.
unsigned available_parallelism();

// The floor a niceonly field's MSD recursion uses (resolved once per field:
// a re-run of the field keeps it).
uint64_t resolve_floor(const nice_niceonly_opts *opts);

// A host-MSD field on the adaptive floor has been collected: move the floor
// (update_msd_floor, client_process_gpu.rs:551, 563-568, 130-157).
void adapt_floor(double msd_seconds, double total_seconds);

}  // namespace abi
}  // namespace nice
