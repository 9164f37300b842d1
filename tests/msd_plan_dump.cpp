// msd_plan_dump.cpp -- prints the niceonly device MSD's batch plans and launch
// grids (nice_amd/csrc/msd_plan.hpp) for tests/test_msd_plan.py, which asserts
// on them.  Host-only: built with a plain C++17 compiler from msd_plan.hpp and
// layout.h, which is itself the check that they need no GPU toolchain.
//
// stdin: lines "<chunk> <floor> <mine> <devices> <cus> <nofuse>" (decimal;
// nofuse 1: the plan gets a fused cap of 0, as the probe build can force).
// stdout, one record per line, fields separated by spaces; a case is its K
// record and the records that follow it:
//   K chunk floor mine devices cus nofuse
//   F cap                        msd_fused_cap(chunk, floor)
//   P err cpb per leaf_cap fcap wave wlevel wgrid wleaf_cap nbatches
//                                the plan (err 0: none, 1: chunk too large,
//                                2: chunk too large for the floor; then zeros)
//   L planner launcher           msd_last_level at the planner's clamped floor
//                                and at the launcher's
//   U chunks grid                msd_fused_grid
//   G nchunks level grid         msd_level_grid, levels 0..launcher's last, for
//                                a full batch and for the field's last batch
//   N on_device n_leaves cap grid    nice_grid
//   W waves_per_group scratch_bytes  of the plan's wave grid
#include <stdio.h>

#include "msd_plan.hpp"

using namespace nice;
using namespace nice::abi;

typedef unsigned long long ull;

static void grids(uint64_t nchunks, uint32_t last, int cus) {
    for (uint32_t level = 0; level <= last; level++)
        printf("G %llu %u %u\n", (ull)nchunks, level, msd_level_grid(nchunks, level, cus));
}

int main() {
    char cbuf[64];
    ull floor_size, mine, nd;
    int cus, nofuse;
    while (scanf("%63s %llu %llu %llu %d %d", cbuf, &floor_size, &mine, &nd, &cus, &nofuse) == 6) {
        u128 chunk = 0;
        for (const char *s = cbuf; *s >= '0' && *s <= '9'; s++) chunk = chunk * 10 + (u128)(*s - '0');
        const uint64_t cnk = (uint64_t)chunk;  // (every case's chunk fits 64 bits)
        printf("K %s %llu %llu %llu %d %d\n", cbuf, floor_size, mine, nd, cus, nofuse);
        const uint32_t cap = msd_fused_cap(cnk, floor_size);
        printf("F %u\n", cap);
        const MsdPlan pl = plan_device_msd(chunk, floor_size, mine, (size_t)nd, cus, nofuse ? 0u : cap,
                                           msd_wave_waves_per_group());
        const int err = !pl.error ? 0 : pl.error == kMsdChunkTooLarge ? 1 : pl.error == kMsdChunkTooLargeForFloor ? 2 : 3;
        if (err) {
            printf("P %d 0 0 0 0 0 0 0 0 0\n", err);
            continue;
        }
        printf("P 0 %llu %llu %llu %u %d %u %u %llu %llu\n", (ull)pl.cpb, (ull)pl.per, (ull)pl.leaf_cap, pl.fcap,
               pl.wave ? 1 : 0, pl.wlevel, pl.wgrid, (ull)pl.wleaf_cap, (ull)pl.nbatches);
        const uint32_t last = msd_last_level(cnk, floor_size);
        printf("L %u %u\n", msd_last_level(cnk, floor_size < (1ull << 30) ? floor_size : 1ull << 30), last);
        const uint64_t tail = mine - (pl.nbatches - 1) * pl.cpb;
        printf("U %llu %llu\n", (ull)pl.cpb, (ull)msd_fused_grid(pl.cpb, cus));
        printf("U %llu %llu\n", (ull)tail, (ull)msd_fused_grid(tail, cus));
        grids(pl.cpb, last, cus);
        if (tail != pl.cpb) grids(tail, last, cus);
        const uint32_t leaves[] = {0u, 1u, 33u, 35000u, 0xffffffffu};
        const uint64_t caps[] = {(uint64_t)cus * 8, 128};
        for (uint64_t c : caps) {
            printf("N 1 0 %llu %u\n", (ull)c, nice_grid(true, 0, cus, c));
            for (uint32_t n : leaves) printf("N 0 %u %llu %u\n", n, (ull)c, nice_grid(false, n, cus, c));
        }
        printf("W %u %llu\n", msd_wave_waves_per_group(), (ull)msd_wave_scratch_bytes(pl.wgrid));
    }
    return 0;
}
