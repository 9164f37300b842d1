// Host code of the per-number map with a main of its own, for the sanitizers:
// the launch plan (fd2_map_plan.hpp) and the CPU twin (cpu_path.cpp, compiled
// beside this file).  Built by tests/test_map.py and scripts/sanitize.sh with
// ASan + UBSan; no Python, no GPU, no preloaded runtime.  Exits non-zero on a
// wrong answer.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../include/nice_hip.h"
#include "fd2_map_plan.hpp"
#include "host_math.hpp"

namespace nice {
static std::string g_msg;
void set_last_error(const char *msg) { g_msg = msg; }  // abi_context.cpp's, for cpu_path.cpp
}  // namespace nice

using nice::u128;

#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                    \
        }                                                                \
    } while (0)

// The plan of [s, e): the records tile it exactly once, in order, no FD record
// crosses a cut or an end of the valid range, lanes <= wg, chunk <= tchunk.
static int check_plan(const nice::MapBase &b, u128 s, u128 e, uint64_t off0) {
    nice::MapPlan pl;
    nice::map_plan(b, s, e, off0, pl);
    u128 at = s;
    uint64_t fd = 0, gen = 0;
    for (const nice::MapRec &r : pl.recs) {
        const u128 lo = ((u128)r.hi << 64) | r.lo;
        CHECK(lo == at && r.off == off0 + (uint64_t)(lo - s) && r.count >= 1);
        if (r.kind == nice::kMapFd) {
            CHECK(b.fd && r.lanes >= 1 && r.lanes <= b.wg && r.chunk >= 1 && r.chunk <= b.tchunk);
            CHECK(r.count == (uint64_t)r.lanes * r.chunk && lo >= b.rs && lo + r.count <= b.re);
            size_t below = 0;
            for (u128 c : b.cuts) {
                CHECK(!(lo < c && c < lo + r.count));
                below += c < lo + r.count;
            }
            CHECK(r.combo == below);
            fd += r.count;
        } else {
            CHECK(r.kind == nice::kMapGeneric && r.lanes == 0 && r.chunk == 0);
            CHECK(!b.fd || lo + r.count <= b.rs || lo >= b.re);
            gen += r.count;
        }
        at = lo + r.count;
    }
    CHECK(at == e && fd == pl.fd_numbers && gen == pl.generic_numbers);
    return 0;
}

static int run_plans(uint32_t base, uint64_t wg, uint64_t tchunk) {
    nice::MapBase b;
    CHECK(nice::base_range_cached(base, b.rs, b.re) == 1);
    b.fd = true;
    b.wg = wg;
    b.tchunk = tchunk;
    // two cuts of this program's own: the plan only needs them ascending and inside the range
    b.cuts = {b.rs + 1000, b.rs + (b.re - b.rs) / 2};
    for (uint64_t size : {(uint64_t)1, (uint64_t)63, (uint64_t)(64 * 80 + 1), (uint64_t)100003}) {
        if (check_plan(b, b.rs, b.rs + size, 0)) return 1;
        if (check_plan(b, b.re - size, b.re, 7)) return 1;
    }
    for (u128 c : b.cuts)
        if (check_plan(b, c - 300, c + 300, 0)) return 1;
    if (check_plan(b, b.re - 150, b.re + 150, 0) || check_plan(b, b.rs - 150, b.rs + 150, 0)) return 1;
    if (check_plan(b, b.rs, b.rs + ((u128)1 << 32), 0)) return 1;
    nice::MapBase none;  // a base without an FD kernel: one generic record
    nice::MapPlan pl;
    nice::map_plan(none, 47, 100, 0, pl);
    CHECK(pl.recs.size() == 1 && pl.recs[0].kind == nice::kMapGeneric && pl.recs[0].count == 53);
    return 0;
}

// The CPU twin on [s, e): every count in 1..base, the same with one and with
// three threads, and not a byte outside the map.
static int run_twin(uint32_t base, u128 s, u128 e) {
    const size_t n = (size_t)(e - s);
    std::vector<uint8_t> a(n + 32, 0xEE), b(n + 32, 0xEE);
    CHECK(nice_cpu_unique_map((uint64_t)s, (uint64_t)(s >> 64), (uint64_t)e, (uint64_t)(e >> 64), base, 1,
                              a.data() + 16, n) == NICE_OK);
    CHECK(nice_cpu_unique_map((uint64_t)s, (uint64_t)(s >> 64), (uint64_t)e, (uint64_t)(e >> 64), base, 3,
                              b.data() + 16, n) == NICE_OK);
    CHECK(a == b);
    for (size_t i = 0; i < n + 32; i++) {
        if (i < 16 || i >= n + 16) CHECK(a[i] == 0xEE);
        else CHECK(a[i] >= 1 && a[i] <= base);
    }
    return 0;
}

int main() {
    if (run_plans(40, 512, 81) || run_plans(50, 512, 161) || run_plans(64, 1024, 241) || run_plans(80, 512, 241))
        return 1;
    u128 rs = 0, re = 0;
    if (run_twin(10, 47, 100)) return 1;
    for (uint32_t base : {40u, 80u}) {
        CHECK(nice::base_range_cached(base, rs, re) == 1);
        if (run_twin(base, rs, rs + 2000)) return 1;
    }
    CHECK(nice::base_range_cached(70, rs, re) == 1);
    if (run_twin(70, rs + 12345, rs + 12345 + 2000)) return 1;
    CHECK(nice::base_range_cached(40, rs, re) == 1);
    if (run_twin(40, re - 150, re + 150)) return 1;
    // 69 is the one nice number of base 10
    uint8_t m[64];
    CHECK(nice_cpu_unique_map(47, 0, 100, 0, 10, 2, m, 64) == NICE_OK && m[69 - 47] == 10);
    // the errors
    std::vector<uint8_t> canary(64, 0xEE);
    CHECK(nice_cpu_unique_map(47, 0, 100, 0, 10, 1, canary.data(), 52) == NICE_ERR_CAPACITY);
    for (uint8_t v : canary) CHECK(v == 0xEE);
    CHECK(nice_cpu_unique_map(47, 0, 47, 0, 10, 1, m, 64) == NICE_ERR_INVALID);
    CHECK(nice_cpu_unique_map(100, 0, 47, 0, 10, 1, m, 64) == NICE_ERR_INVALID);
    CHECK(nice_cpu_unique_map(47, 0, 100, 0, 1, 1, m, 64) == NICE_ERR_INVALID);
    CHECK(nice_cpu_unique_map(47, 0, 100, 0, 129, 1, m, 64) == NICE_ERR_INVALID);
    CHECK(nice_cpu_unique_map(47, 0, 100, 0, 10, 1, nullptr, 64) == NICE_ERR_INVALID);
    CHECK(nice_cpu_unique_map(47, 0, 48 + (1ull << 32), 0, 10, 1, m, 64) == NICE_ERR_INVALID);
    std::puts("map_san ok");
    return 0;
}
