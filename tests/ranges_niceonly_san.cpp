// Host code of the batched niceonly ranges with a main of its own, for the
// sanitizers: the leaf plan (niceonly_ranges_plan.hpp) and the CPU twin
// (cpu_path.cpp, compiled beside this file).  Built by
// tests/test_ranges_niceonly.py and scripts/sanitize.sh with ASan + UBSan; no
// Python, no GPU, no preloaded runtime.  Exits non-zero on a wrong answer.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../include/nice_hip.h"
#include "niceonly_ranges_plan.hpp"

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

static void push(std::vector<uint64_t> &b, u128 s, u128 e) {
    b.push_back((uint64_t)s), b.push_back((uint64_t)(s >> 64)), b.push_back((uint64_t)e), b.push_back((uint64_t)(e >> 64));
}

// Ranges of every shape the plan tells apart, around the start of the base's
// valid range (or from 1 for a base whose range is tiny).
static std::vector<uint64_t> ranges_of(uint32_t base, const nice::StrideTable &t, u128 long_len) {
    u128 rs = 0, re = 0;
    nice::base_range_cached(base, rs, re);
    const u128 M = t.modulus, c = (rs / M + 2) * M;
    std::vector<uint64_t> b;
    push(b, c + 1, c + 2);
    push(b, c + t.residues[0], c + t.residues[0] + 1);
    push(b, c + t.residues.back() + 1, c + M + t.residues[0] + 1);
    push(b, c + M - 3, c + 3 * M + 7);
    push(b, rs > 500 ? rs - 500 : 1, rs + 500);
    push(b, re - 100, re + 900);
    push(b, re + 1, re + 4000);
    push(b, c + 5, c + 5 + long_len);
    push(b, c + M - 3, c + 3 * M + 7);  // repeated
    return b;
}

static int run_base(uint32_t base, u128 long_len, bool twin) {
    const nice::StrideTable t(base, 2);
    CHECK(!t.residues.empty());
    const std::vector<uint64_t> b = ranges_of(base, t, long_len);
    const size_t n = b.size() / 4;
    for (size_t nd : {(size_t)1, (size_t)2, (size_t)8}) {
        const nice::NiceRangesPlan pl = nice::plan_nice_ranges(base, 2, t, b.data(), n, nd);
        CHECK(pl.error.empty());
        std::vector<uint64_t> per(n, 0);
        uint32_t last_dev[2] = {0, 0};
        for (size_t q = 0; q < pl.leaves.size(); q++) {
            const nice::PlanLeaf &l = pl.leaves[q];
            CHECK(l.range < n && l.count > 0 && l.count <= nice::kLeafPiece && l.g0 <= t.residues.size());
            CHECK(l.device < nd && l.device >= last_dev[l.group] && (q < pl.n_fast_leaves) == (l.group == 1));
            last_dev[l.group] = l.device;
            per[l.range] += l.count;
        }
        uint64_t total = 0;
        for (size_t i = 0; i < n; i++) {
            CHECK(per[i] == pl.candidates[i]);
            total += per[i];
        }
        CHECK(total == pl.total && pl.fast_ranges + pl.generic_ranges == n);
    }
    if (!twin) return 0;
    std::vector<uint64_t> cand(n), cand1(n);
    std::vector<uint32_t> sq(n), sq1(n), idx(4096), idx1(4096);
    std::vector<nice_number> out(4096), out1(4096);
    size_t got = 0, got1 = 0;
    CHECK(nice_cpu_process_ranges_niceonly(base, b.data(), n, 0, 4, cand.data(), sq.data(), out.data(), idx.data(),
                                           out.size(), &got) == NICE_OK);
    CHECK(nice_cpu_process_ranges_niceonly(base, b.data(), n, 0, 1, cand1.data(), sq1.data(), out1.data(),
                                           idx1.data(), out1.size(), &got1) == NICE_OK);
    CHECK(got == got1 && cand == cand1 && sq == sq1);
    const nice::NiceRangesPlan pl = nice::plan_nice_ranges(base, 2, t, b.data(), n, 1);
    CHECK(cand == pl.candidates);
    for (size_t j = 0; j < got; j++)
        CHECK(idx[j] == idx1[j] && out[j].number_lo == out1[j].number_lo && out[j].num_uniques == base &&
              (j == 0 || idx[j - 1] <= idx[j]));
    // null count arrays, a list too short, then the error paths
    size_t need = 0;
    const int rc = nice_cpu_process_ranges_niceonly(base, b.data(), n, 0, 2, nullptr, nullptr, out.data(), nullptr, 0, &need);
    CHECK(need == got && rc == (got ? NICE_ERR_CAPACITY : NICE_OK));
    return 0;
}

int main() {
    // b40: a range of 4e9 numbers splits into pieces (plan only: the twin would walk 3e8 candidates)
    if (run_base(40, (u128)4000000000ull, false)) return 1;
    if (run_base(40, 150000, true)) return 1;
    if (run_base(10, 100000, true)) return 1;
    if (run_base(62, 60000, true)) return 1;  // n past 64 bits
    if (run_base(97, 50000, true)) return 1;
    std::vector<uint64_t> b;
    push(b, 47, 100);
    push(b, 9, 9);
    size_t n_out = 0;
    nice_number one[4];
    uint32_t idx[4];
    uint64_t cand[2];
    uint32_t sq[2];
    CHECK(nice_cpu_process_ranges_niceonly(10, b.data(), 2, 0, 1, cand, sq, one, idx, 4, &n_out) == NICE_ERR_INVALID);
    CHECK(nice::g_msg.find("range 1") != std::string::npos);
    CHECK(nice_cpu_process_ranges_niceonly(10, b.data(), 1, 0, 1, cand, sq, one, idx, 4, &n_out) == NICE_OK);
    CHECK(n_out == 1 && one[0].number_lo == 69 && idx[0] == 0);
    CHECK(nice_cpu_process_ranges_niceonly(43, b.data(), 1, 0, 1, cand, sq, one, idx, 4, &n_out) == NICE_OK);
    CHECK(n_out == 0 && cand[0] == 0 && sq[0] == 0);
    CHECK(nice_cpu_process_ranges_niceonly(97, b.data(), 1, 4, 1, cand, sq, one, idx, 4, &n_out) == NICE_ERR_INVALID);
    CHECK(nice_cpu_process_ranges_niceonly(10, b.data(), 0, 0, 1, cand, sq, one, idx, 4, &n_out) == NICE_ERR_INVALID);
    b.clear();
    push(b, 1, (u128)1 << 60);
    CHECK(nice_cpu_process_ranges_niceonly(10, b.data(), 1, 0, 1, cand, sq, one, idx, 4, &n_out) == NICE_ERR_INVALID);
    const nice::StrideTable t10(10, 2);
    CHECK(!nice::plan_nice_ranges(10, 2, t10, b.data(), 1, 1).error.empty());
    std::puts("ranges_niceonly_san ok");
    return 0;
}
