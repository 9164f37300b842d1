// fd2_sib_pers_plan_dump.cpp -- the persistent sibling grid's launch plans
// (nice_amd/csrc/fd2_plan.hpp plan_sib_pers / plan_sib_launch) for
// tests/test_fd2_sib_pers_plan.py.  Host-only.  For every launch the program
// also walks the grid the way the device does (fd2_kernel.hpp: workgroup g
// takes the batches g + G k, lane l of batch b the unit sib_unit_at gives, all
// in 32-bit words) and counts how often each sibling and edge unit is taken.
//
//   fd2_sib_pers_plan_dump [L_STEP]     odd lane strides 105, 105 + L_STEP, ... (default 2)
//
// stdout, one record per line:
//   K cus per_cu count L mode max_wg overlapped   a case; its records follow
//   N | X                                   no sibling walk / invalid
//   S pers pers_grid wave_cap upb has_edge r
//   T off Q cnt R sib_units edge_units sib_blocks edge_blocks main_blocks grid batches wave_cap
//     chunk nunits tail walked missed twice max_per_wg
//                                           a launch; walked 1: the grid was walked, missed / twice:
//                                           units taken never / more than once, max_per_wg: the most
//                                           batches one workgroup owns
//   O R chunk nunits tail main_blocks       the rounds plan's remainder parts of the same segment
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "fd2_cfg.hpp"
#include "fd2_plan.hpp"

using namespace nice;
using namespace nice::fd2;

typedef unsigned long long ull;
using P = BigCfg<40, 4, 8, 5>;  // production: the pipelined b40 sibling kernel
static_assert(P::HAS_SIBPERS && P::SibPers::SIBPERS && !P::SibPers::PERS && P::SibPers::WG == P::WG &&
                  P::SibPers::LDS_BYTES == P::LDS_BYTES,
              "the persistent twin shares the rounds kernel's layout");

// The device's walk of one launch's sibling part.
static void walk(const SibLaunchPlan &pl, ull &missed, ull &twice, ull &max_per_wg) {
    const u32 sib_units = (u32)pl.sib_units, edge_units = (u32)pl.edge_units, G = (u32)pl.sib_blocks;
    std::vector<unsigned char> s(sib_units, 0), e(edge_units, 0);
    const u32 nsb = (sib_units + 63) / 64, nb = nsb + (edge_units + 63) / 64;
    max_per_wg = 0;
    for (u32 g = 0; g < G; g++) {
        const u32 nk = nb > g ? (nb - g + G - 1) / G : 0;
        if (nk > max_per_wg) max_per_wg = nk;
        for (u32 k = 0; k < nk; k++) {
            const u32 b = g + G * k;
            const bool edge = b >= nsb;
            for (u32 lane = 0; lane < 64; lane++) {
                const u32 unit = 64 * (edge ? b - nsb : b) + lane;
                if (unit >= (edge ? edge_units : sib_units)) continue;
                unsigned char &c = edge ? e[unit] : s[unit];
                if (c < 2) c++;
            }
        }
    }
    missed = twice = 0;
    for (unsigned char c : s) missed += c == 0, twice += c > 1;
    for (unsigned char c : e) missed += c == 0, twice += c > 1;
}

static void run_case(u128 start, u64 count, int cus, int per_cu, u64 L, u32 mode, u32 max_wg, bool overlapped,
                     bool walk_it) {
    constexpr u64 SB = (u64)P::SIB * P::B * P::B;
    printf("K %d %d %llu %llu %u %u %d\n", cus, per_cu, (ull)count, (ull)L, mode, max_wg, (int)overlapped);
    PlanKnobs<P> k;
    k.sib_pers_mode = mode;
    k.sib_pers_max_wg = max_wg;
    SibShape sh = plan_sib<P>(start, count, cus, per_cu, overlapped, L, k);
    if (sh.kind != SibShape::kSib) {
        puts(sh.kind == SibShape::kNoSib ? "N" : "X");
        return;
    }
    const SibShape rounds = sh;
    plan_sib_pers<P>(sh, count, cus, per_cu, overlapped, k);
    printf("S %d %llu %u %llu %d %llu\n", (int)sh.pers, (ull)sh.pers_grid, sh.wave_cap, (ull)sh.upb, (int)sh.has_edge,
           (ull)sh.r);
    u64 left = count, off = 0;
    while (left) {
        const SibLaunchPlan pl = plan_sib_launch<P>(left, sh, cus, per_cu, k);
        ull missed = 0, twice = 0, max_per_wg = 0;
        const bool w = sh.pers && walk_it && pl.sib_units <= 0xffffffffull;
        if (w) walk(pl, missed, twice, max_per_wg);
        printf("T %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %u %llu %llu %llu %d %llu %llu %llu\n", (ull)off,
               (ull)pl.Q, (ull)pl.cnt, (ull)pl.R, (ull)pl.sib_units, (ull)pl.edge_units, (ull)pl.sib_blocks,
               (ull)pl.edge_blocks, (ull)pl.main_blocks, (ull)pl.grid, (ull)pl.batches, pl.wave_cap, (ull)pl.chunk,
               (ull)pl.nunits, (ull)pl.tail, (int)w, missed, twice, max_per_wg);
        if (!pl.cnt) break;  // (a plan that takes nothing: the test fails on the counts)
        off += pl.cnt;
        left -= pl.cnt;
    }
    // the rounds plan's remainder: the last launch of the same segment
    left = count;
    for (;;) {
        const SibLaunchPlan pl = plan_sib_launch<P>(left, rounds, cus, per_cu, k);
        if (pl.cnt == left || !pl.cnt) {
            printf("O %llu %llu %llu %llu %llu\n", (ull)pl.R, (ull)pl.chunk, (ull)pl.nunits, (ull)pl.tail,
                   (ull)pl.main_blocks);
            break;
        }
        left -= pl.cnt;
    }
    (void)SB;
}

int main(int argc, char **argv) {
    const u64 step = argc > 1 ? strtoull(argv[1], nullptr, 10) & ~1ull : 2;
    constexpr u64 SB = (u64)P::SIB * P::B * P::B;
    const u128 start = 1916284264916ull;  // b40's range start
    const u64 counts[] = {4 * SB, 4 * SB + 1234567, 8 * SB + 54321, 100000000, 250000000, 1000000000, 32000000000ull};
    std::vector<u64> strides = {45, 61, 125, 143, 159, 255};
    for (u64 L = 105; L <= 211; L += step ? step : 2) strides.push_back(L | 1);
    for (int cus : {8, 64, 256, 304})
        for (int per_cu : {1, 2})
            for (u64 count : counts)
                for (u64 L : strides) {
                    // the device's walk of the big fields at three strides only
                    // (and the 3.2e10 field on the MI355X's shape at one)
                    const bool pinned = L == 125 || L == 143 || L == 159;
                    const bool walk_it = count <= 250000000 || (pinned && count <= 1000000000) ||
                                         (L == 143 && cus == 256 && per_cu == 2);
                    run_case(start, count, cus, per_cu, L, 0, 0, true, walk_it);
                    run_case(start, count, cus, per_cu, L, 0, 0, false, false);
                    run_case(start, count, cus, per_cu, L, 2, 0, true, false);
                    for (u32 max_wg : {0u, 1u, 3u, 64u})
                        run_case(start, count, cus, per_cu, L, 1, max_wg, false, walk_it);
                }
    return 0;
}
