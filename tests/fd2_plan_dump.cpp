// fd2_plan_dump.cpp -- prints the FD detailed kernel's launch plans
// (nice_amd/csrc/fd2_plan.hpp) for tests/test_fd2_plan.py, which asserts on
// them.  Host-only: built with a plain C++17 compiler from the two headers
// below, which is itself the check that they need no GPU toolchain.
//
// stdin: lines "<base> <start>" (decimal; start inside the base's range).
// stdout, one record per line, fields separated by spaces:
//   C name WG B LDE SIB LSD PERS HQ TCHUNK     a configuration
//   K name cus per_cu start count overlapped forced    a case; its records follow
//   R WG B LSD HQ PERS off cnt chunk nunits tail grid main_blocks wave_cap
//                                              a regular launch at start + off
//   E                                          no regular launch holds the numbers
//   N                                          sibling config: run the NoSib kernel (its R records follow)
//   X                                          sibling config: invalid
//   S L U upb r has_edge qmax                  sibling shape
//   T off Q cnt R chunk nunits tail sib_blocks edge_blocks main_blocks grid
//                                              a sibling launch at start + off
//   P name lane small                          the pinned picks of the bench field
#include <stdio.h>
#include <string.h>

#include "fd2_cfg.hpp"
#include "fd2_plan.hpp"

using namespace nice;
using namespace nice::fd2;

typedef unsigned long long ull;

static u128 parse_u128(const char *s) {
    u128 v = 0;
    for (; *s >= '0' && *s <= '9'; s++) v = v * 10 + (u128)(*s - '0');
    return v;
}

static const char *str_u128(u128 v, char (&buf)[48]) {
    char *p = buf + sizeof(buf) - 1;
    *p = 0;
    do {
        *--p = (char)('0' + (int)(v % 10));
        v /= 10;
    } while (v);
    return p;
}

// launch_cfg's dispatch: the persistent grid where it suits, else the same
// kernel in rounds; then one plan per launch until the numbers are done.
template <class P>
static void regular(u64 count, int cus, int per_cu) {
    if constexpr (P::PERS) {
        if (!pers_suits<P>(count, cus, per_cu)) return regular<typename P::NoPers>(count, cus, per_cu);
    }
    u64 left = count, off = 0;
    while (left) {
        const RegularPlan pl = plan_regular<P>(left, cus, per_cu);
        if (!pl.ok) {
            puts("E");
            return;
        }
        printf("R %d %u %d %d %d %llu %llu %llu %llu %llu %llu %llu %u\n", P::WG, P::B, (int)P::LSD, P::HQ, (int)P::PERS,
               (ull)off, (ull)pl.cnt, (ull)pl.chunk, (ull)pl.nunits, (ull)pl.tail, (ull)pl.grid, (ull)pl.main_blocks,
               pl.wave_cap);
        off += pl.cnt;
        left -= pl.cnt;
    }
}

template <class P>
static void run_case(const char *name, u128 start, u64 count, int cus, int per_cu, bool overlapped, u64 forced) {
    char buf[48];
    printf("K %s %d %d %s %llu %d %llu\n", name, cus, per_cu, str_u128(start, buf), (ull)count, (int)overlapped,
           (ull)forced);
    if constexpr (P::SIB > 1) {
        const SibShape sh = plan_sib<P>(start, count, cus, per_cu, overlapped, forced);
        if (sh.kind == SibShape::kNoSib) {
            puts("N");
            return regular<typename P::NoSib>(count, cus, per_cu);
        }
        if (sh.kind == SibShape::kError) {
            puts("X");
            return;
        }
        printf("S %llu %llu %llu %llu %d %llu\n", (ull)sh.L, (ull)sh.U, (ull)sh.upb, (ull)sh.r, (int)sh.has_edge,
               (ull)sh.qmax);
        u64 left = count, off = 0;
        while (left) {
            const SibLaunchPlan pl = plan_sib_launch<P>(left, sh, cus, per_cu);
            printf("T %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", (ull)off, (ull)pl.Q, (ull)pl.cnt,
                   (ull)pl.R, (ull)pl.chunk, (ull)pl.nunits, (ull)pl.tail, (ull)pl.sib_blocks, (ull)pl.edge_blocks,
                   (ull)pl.main_blocks, (ull)pl.grid);
            off += pl.cnt;
            left -= pl.cnt;
        }
    } else {
        regular<P>(count, cus, per_cu);
    }
}

template <class P>
static void run_cfg(const char *name, u128 start) {
    static bool described = false;
    if (!described) {
        printf("C %s %d %u %d %d %d %d %d %d\n", name, P::WG, P::B, P::LDE, P::SIB, (int)P::LSD, (int)P::PERS, P::HQ,
               P::TCHUNK);
        described = true;
    }
    const u64 WG = P::WG, SB = (u64)P::SIB * P::B * P::B;
    const u64 counts[] = {1, 3, 4, 63, 64, 65, WG, WG + 1, 1000000, 10000000, 4 * SB - 1, 4 * SB,
                          4 * SB + 1234567, 1000000000, 32000000000ull};
    for (int cus : {256, 8})
        for (int per_cu : {1, 2, 3})
            for (u64 count : counts) {
                run_case<P>(name, start, count, cus, per_cu, false, 0);
                if constexpr (P::SIB > 1) {
                    run_case<P>(name, start, count, cus, per_cu, true, 0);
                    for (u64 L = 45; L <= 255; L += 2)
                        for (int ov = 0; ov < 2; ov++) run_case<P>(name, start, count, cus, per_cu, ov != 0, L);
                }
            }
}

int main() {
    // the bench field: pick_lane_stride over [105, 210] at target 140, and the
    // lone-field pick over the same range on 262 144 lanes
    {
        using P = BigCfg<40, 4, 8, 5>;
        const u128 start = 1916284264916ull;
        const u64 count = 1000000000, D = (u64)P::B * P::B, SB = P::SIB * D;
        double rounds = 0;
        printf("P b40_sib3_pipe %llu %llu\n", (ull)pick_lane_stride<P>(start, count, 105, 210, 140, P::LO + 1),
               (ull)pick_small_stride<P>(start, count, 105, 210, P::LO + 1, count / SB, 256 * 1024, D, rounds));
    }
    char line[128];
    while (fgets(line, sizeof line, stdin)) {
        int base = 0;
        char num[64];
        if (sscanf(line, "%d %63s", &base, num) != 2) continue;
        const u128 start = parse_u128(num);
        // configurations fd2_part.hip dispatches to (fd2_cfg.hpp: BigCfg for
        // fields >= 1e7, its NoSib fallback, SmallCfg below)
        if (base == 40) {
            run_cfg<BigCfg<40, 4, 8, 5>>("b40_sib3_pipe", start);
            run_cfg<BigCfg<40, 5, 8, 5>>("b40_sib3", start);
            run_cfg<SmallCfg<40, 4, 8, 5>>("b40_512", start);
        } else if (base == 44) {
            run_cfg<BigCfg<44, 5, 9, 5>>("b44_sib3", start);
        } else if (base == 52) {
            run_cfg<BigCfg<52, 6, 11, 6>>("b52_sib2", start);
        } else if (base == 50) {
            run_cfg<BigCfg<50, 5, 10, 6>::NoSib>("b50_big", start);
        } else if (base == 80) {
            run_cfg<BigCfg<80, 8, 16, 9>>("b80_big", start);
            run_cfg<SmallCfg<80, 8, 16, 9>>("b80_512", start);
        }
    }
    return 0;
}
