// Host code of the sound prefix test per caller range with a main of its own,
// for the sanitizers: the CPU twin nice_cpu_process_ranges_niceonly_ex
// (cpu_path.cpp, compiled beside this file) with the test on and off, on ranges
// inside, across and outside a base's valid range.  Built by
// tests/test_ranges_prefix.py with ASan + UBSan; no Python, no GPU, no
// preloaded runtime.  The answers themselves are checked in Python against the
// restatement; here only what must hold between the calls.  Exits non-zero when
// it does not.
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

struct Answer {
    std::vector<uint64_t> cand, rej;
    std::vector<uint32_t> sq;
    size_t listed = 0;
};

static int call(uint32_t base, const std::vector<uint64_t> &b, uint32_t prefix, int threads, Answer &a) {
    const size_t n = b.size() / 4;
    a.cand.assign(n, 7), a.rej.assign(n, 7), a.sq.assign(n, 7);
    std::vector<nice_number> out(256);
    std::vector<uint32_t> idx(256);
    const nice_ranges_niceonly_opts o{0, prefix, {0, 0}};
    return nice_cpu_process_ranges_niceonly_ex(base, b.data(), n, &o, threads, a.cand.data(), a.sq.data(), a.rej.data(),
                                               out.data(), idx.data(), out.size(), &a.listed);
}

// `inside`: how many leading ranges lie wholly inside the valid range.
static int run_base(uint32_t base, bool fast) {
    u128 rs = 0, re = 0;
    CHECK(nice::base_range_cached(base, rs, re) == 1);
    const nice::StrideTable t(base, 2);
    const u128 M = t.modulus, c = ((rs + (re - rs) / 3) / M + 1) * M;
    std::vector<uint64_t> b;
    for (int i = 0; i < 24; i++) push(b, c + 1000 * i, c + 1000 * i + 700 + 13 * i);  // leaf-sized
    push(b, c + t.residues[1], c + t.residues[1] + 1);                                // one number, a candidate
    push(b, c + t.residues[2], c + t.residues[2] + 2);                                // two numbers
    push(b, c, c + M + 5);                                                            // a whole cycle
    const size_t inside = b.size() / 4;
    push(b, re - 2000, re + 2000);  // across the end
    push(b, re + 10, re + 3000);    // outside
    const size_t n = b.size() / 4;
    Answer off, on, on1;
    CHECK(call(base, b, NICE_RANGES_PREFIX_OFF, 4, off) == NICE_OK);
    CHECK(call(base, b, NICE_RANGES_PREFIX_ON, 4, on) == NICE_OK);
    CHECK(call(base, b, NICE_RANGES_PREFIX_ON, 1, on1) == NICE_OK);
    CHECK(on.cand == on1.cand && on.rej == on1.rej && on.sq == on1.sq && on.listed == on1.listed);
    CHECK(on.cand == off.cand && on.listed <= off.listed);
    uint64_t rejected = 0;
    for (size_t i = 0; i < n; i++) {
        CHECK(off.rej[i] == 0 && on.rej[i] <= on.cand[i] && on.sq[i] <= off.sq[i]);
        CHECK(on.rej[i] + on.sq[i] <= on.cand[i]);
        const bool runs = fast && i < inside;
        CHECK(runs == nice::nice_range_fast(base, 2, nice::range_at(b.data(), i, 0), nice::range_at(b.data(), i, 1)));
        if (!runs) CHECK(on.rej[i] == 0 && on.sq[i] == off.sq[i]);
        rejected += on.rej[i];
    }
    CHECK(on.cand[24] == 1 && on.rej[24] == 0);  // a range of one number rejects nothing
    CHECK(fast ? rejected > 0 : rejected == 0);
    return 0;
}

int main() {
    if (run_base(40, true)) return 1;
    if (run_base(57, true)) return 1;  // n past 64 bits
    if (run_base(65, true)) return 1;  // three mask words
    if (run_base(70, false)) return 1;
    std::vector<uint64_t> b;
    push(b, 47, 100);
    Answer a;
    CHECK(call(10, b, NICE_RANGES_PREFIX_ON, 2, a) == NICE_OK && a.listed == 1 && a.rej[0] == 0);
    CHECK(call(10, b, 2, 1, a) == NICE_ERR_INVALID && nice::g_msg.find("prefix_test") != std::string::npos);
    nice_ranges_niceonly_opts o{0, NICE_RANGES_PREFIX_ON, {0, 9}};
    size_t n_out = 0;
    CHECK(nice_cpu_process_ranges_niceonly_ex(10, b.data(), 1, &o, 1, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                              &n_out) == NICE_ERR_INVALID);
    CHECK(nice_cpu_process_ranges_niceonly_ex(10, b.data(), 1, nullptr, 1, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                              &n_out) == NICE_ERR_CAPACITY && n_out == 1);
    CHECK(call(43, b, NICE_RANGES_PREFIX_ON, 1, a) == NICE_OK && a.cand[0] == 0 && a.rej[0] == 0 && a.listed == 0);
    std::puts("ranges_prefix_san ok");
    return 0;
}
