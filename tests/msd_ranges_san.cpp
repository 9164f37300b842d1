// Host code of the recursion's range list with a main of its own, for the
// sanitizers: the plan (msd_ranges_plan.hpp) and the CPU twin
// (nice_cpu_msd_ranges in cpu_path.cpp, compiled beside this file).  Built by
// tests/test_msd_ranges.py with ASan + UBSan; no Python, no GPU, no preloaded
// runtime.  Exits non-zero on a wrong answer.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../include/nice_hip.h"
#include "host_math.hpp"
#include "msd_ranges_plan.hpp"

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

static void push(std::vector<uint64_t> &r, u128 s, u128 e) {
    r.push_back((uint64_t)s), r.push_back((uint64_t)(s >> 64)), r.push_back((uint64_t)e),
        r.push_back((uint64_t)(e >> 64));
}

// The plan of `roots`: every root once, devices in contiguous ascending runs,
// batches ascending from 0 per device with bounds inside the budget, the group
// by the root's size.
static int check_plan(uint32_t base, const std::vector<uint64_t> &roots, uint64_t floor_size, size_t nd) {
    const size_t n = roots.size() / 4;
    const nice::MsdRangesPlan pl = nice::plan_msd_ranges(base, roots.data(), n, floor_size, nd);
    CHECK(pl.error.empty() && pl.roots.size() == n && pl.first.size() == nd + 1 && pl.nbatches.size() == nd);
    CHECK(pl.first[0] == 0 && pl.first[nd] == n);
    uint32_t dev = 0, batch = 0;
    uint64_t in_batch = 0;
    for (size_t i = 0; i < n; i++) {
        const nice::MsdRangesRoot &r = pl.roots[i];
        CHECK(r.size == (uint64_t)(nice::range_at(roots.data(), i, 1) - nice::range_at(roots.data(), i, 0)));
        CHECK(r.device >= dev && r.device < nd);
        if (r.device != dev) dev = r.device, batch = 0, in_batch = 0;
        CHECK(pl.first[dev] <= i && i < pl.first[dev + 1]);
        CHECK(r.batch == batch || r.batch == batch + 1);
        if (r.batch != batch) batch = r.batch, in_batch = 0;
        in_batch += nice::msd_ranges_bound(r.size, floor_size);
        CHECK(in_batch <= nice::kMsdRangesBatchNodes && r.batch < pl.nbatches[dev]);
        CHECK(r.group == (r.size / floor_size + 2 <= nice::kFusedMaxCap && r.size <= 0xffffffffull ? 1u : 0u));
    }
    return 0;
}

// The CPU twin against nice::MsdFilterT's recursion root by root, with one and
// three threads, a short capacity, and not a word outside the outputs.
static int run_twin(uint32_t base, const std::vector<uint64_t> &roots, uint64_t floor_size, uint32_t filter) {
    const size_t n = roots.size() / 4;
    std::vector<uint64_t> want;
    std::vector<uint32_t> want_root;
    std::vector<uint64_t> want_counts(n, 0);
    const auto msd = nice::make_msd(base);
    for (size_t i = 0; i < n; i++) {
        std::vector<std::pair<u128, u128>> rs;
        msd->ranges(nice::range_at(roots.data(), i, 0), nice::range_at(roots.data(), i, 1), floor_size, rs, filter != 0);
        for (auto &r : rs) push(want, r.first, r.second), want_root.push_back((uint32_t)i);
        want_counts[i] = rs.size();
    }
    const size_t m = want_root.size();
    for (int threads : {1, 3}) {
        std::vector<uint64_t> out(4 * m + 8, 0xEEEEEEEEEEEEEEEEull), counts(n + 2, 0xEEEEEEEEEEEEEEEEull);
        std::vector<uint32_t> idx(m + 2, 0xEEEEEEEEu);
        size_t got = 0;
        if (m > 0) {
            CHECK(nice_cpu_msd_ranges(base, roots.data(), n, floor_size, filter, threads, out.data() + 4, idx.data() + 1,
                                      counts.data() + 1, m - 1, &got) == NICE_ERR_CAPACITY);
            CHECK(got == m && out[4] == 0xEEEEEEEEEEEEEEEEull);
        }
        CHECK(nice_cpu_msd_ranges(base, roots.data(), n, floor_size, filter, threads, out.data() + 4, idx.data() + 1,
                                  counts.data() + 1, m, &got) == NICE_OK);
        CHECK(got == m);
        for (size_t q = 0; q < 4 * m; q++) CHECK(out[4 + q] == want[q]);
        for (size_t q = 0; q < m; q++) CHECK(idx[1 + q] == want_root[q]);
        for (size_t i = 0; i < n; i++) CHECK(counts[1 + i] == want_counts[i]);
        for (size_t q = 0; q < 4; q++) CHECK(out[q] == 0xEEEEEEEEEEEEEEEEull && out[4 + 4 * m + q] == 0xEEEEEEEEEEEEEEEEull);
        CHECK(idx[0] == 0xEEEEEEEEu && idx[m + 1] == 0xEEEEEEEEu);
        CHECK(counts[0] == 0xEEEEEEEEEEEEEEEEull && counts[n + 1] == 0xEEEEEEEEEEEEEEEEull);
        // null out_root and counts
        CHECK(nice_cpu_msd_ranges(base, roots.data(), n, floor_size, filter, threads, out.data() + 4, nullptr, nullptr,
                                  m, &got) == NICE_OK);
    }
    return 0;
}

int main() {
    u128 rs = 0, re = 0;
    CHECK(nice::base_range_cached(40, rs, re) == 1);
    const u128 a40 = 4234942132458ull;
    std::vector<uint64_t> roots;
    // sizes on both sides of the form boundary at floor 250, a root across the range's end, a repeat
    for (uint64_t size : {(uint64_t)1, (uint64_t)249, (uint64_t)250, (uint64_t)501, (uint64_t)1003, (uint64_t)100000,
                          (uint64_t)250 * 16382, (uint64_t)250 * 16382 + 250, (uint64_t)1 << 23})
        push(roots, a40, a40 + size);
    push(roots, re - 700, re + 700);
    push(roots, a40, a40 + 100000);
    for (size_t nd : {(size_t)1, (size_t)2, (size_t)3, (size_t)64})
        if (check_plan(40, roots, 250, nd) || check_plan(40, roots, 1, nd)) return 1;
    // more than one batch: 40 roots at the depth cap's bound of 2^22 each
    std::vector<uint64_t> big;
    for (int i = 0; i < 40; i++) push(big, a40 + i, a40 + i + ((u128)1 << 23));
    if (check_plan(40, big, 1, 1) || check_plan(40, big, 1, 2)) return 1;
    {
        const nice::MsdRangesPlan pl = nice::plan_msd_ranges(40, big.data(), 40, 1, 1);
        CHECK(pl.nbatches[0] == 2 && pl.roots[31].batch == 0 && pl.roots[32].batch == 1);
    }
    // the twin: small roots only (the recursion under the sanitizers is slow)
    std::vector<uint64_t> small;
    for (uint64_t size : {(uint64_t)1, (uint64_t)6, (uint64_t)7, (uint64_t)8, (uint64_t)13, (uint64_t)14, (uint64_t)15,
                          (uint64_t)31, (uint64_t)20000})
        push(small, a40, a40 + size);
    push(small, re - 300, re + 300);
    push(small, a40, a40 + 15);
    for (uint32_t filter : {0u, 1u})
        if (run_twin(40, small, 7, filter) || run_twin(40, small, 250, filter)) return 1;
    std::vector<uint64_t> ten;
    push(ten, 47, 100);
    if (run_twin(10, ten, 4, 0) || run_twin(10, ten, 4, 1)) return 1;
    // the errors
    uint64_t out[64];
    size_t got = 0;
    uint64_t bad[8] = {47, 0, 100, 0, 100, 0, 100, 0};
    CHECK(nice_cpu_msd_ranges(10, bad, 2, 4, 0, 1, out, nullptr, nullptr, 16, &got) == NICE_ERR_INVALID);
    CHECK(nice::g_msg.find("root 1") != std::string::npos);
    CHECK(nice_cpu_msd_ranges(10, bad, 0, 4, 0, 1, out, nullptr, nullptr, 16, &got) == NICE_ERR_INVALID);
    CHECK(nice_cpu_msd_ranges(10, bad, 1, 0, 0, 1, out, nullptr, nullptr, 16, &got) == NICE_ERR_INVALID);
    CHECK(nice_cpu_msd_ranges(10, bad, 1, 4, 2, 1, out, nullptr, nullptr, 16, &got) == NICE_ERR_INVALID);
    CHECK(nice_cpu_msd_ranges(1, bad, 1, 4, 0, 1, out, nullptr, nullptr, 16, &got) == NICE_ERR_INVALID);
    CHECK(nice_cpu_msd_ranges(129, bad, 1, 4, 0, 1, out, nullptr, nullptr, 16, &got) == NICE_ERR_INVALID);
    uint64_t huge[4] = {47, 0, 48 + (1ull << 40), 0};
    CHECK(nice_cpu_msd_ranges(10, huge, 1, 4, 0, 1, out, nullptr, nullptr, 16, &got) == NICE_ERR_INVALID);
    CHECK(nice_cpu_msd_ranges(10, nullptr, 1, 4, 0, 1, out, nullptr, nullptr, 16, &got) == NICE_ERR_INVALID);
    std::puts("msd_ranges_san ok");
    return 0;
}
