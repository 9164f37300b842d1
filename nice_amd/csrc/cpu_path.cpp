// cpu_path.cpp -- the reference's CPU API for the field-processing path
// (common/src/client_process.rs:150 process_range_detailed, :439
// process_range_niceonly) on the host cores: for callers of that API that
// have no GPU, and for the reference client's CPU mode.  Product code
// (independent of oracle/, which stays test-only); the GPU entry points
// never call it -- there is no silent fallback from the device.
//
// Detailed: every n's square and cube as u32 words (host_math.hpp powers),
// their base-b digits by chunked division (compile-time divisors for the
// benchmark and live bases), a digit-set popcount.  Niceonly: the MSD filter
// over the whole range (msd_prefix_filter.rs:665-674, floor 250), then the
// stride candidates of every surviving range (stride_filter.rs:139-155) with
// the early-exit niceness test (client_process.rs:222-253: the square's digits
// first, then the cube's).  `threads` splits the work into contiguous pieces
// whose results are concatenated in order, so lists stay ascending.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "../../include/nice_hip.h"
#include "host_math.hpp"
#include "niceonly_bases.h"
#include "msd_ranges_plan.hpp"
#include "niceonly_ranges_plan.hpp"

namespace {

using nice::u128;

int cpu_fail(int code, const char *msg);

inline u128 mk(uint64_t lo, uint64_t hi) { return ((u128)hi << 64) | lo; }

struct Bits {
    uint64_t w[2] = {0, 0};
    // false if the digit was already present
    bool add(uint8_t d) {
        const uint64_t b = 1ull << (d & 63);
        uint64_t &x = w[d >> 6];
        const bool fresh = (x & b) == 0;
        x |= b;
        return fresh;
    }
    uint32_t count() const { return (uint32_t)(__builtin_popcountll(w[0]) + __builtin_popcountll(w[1])); }
};

template <class BP>
uint32_t unique_digits(u128 n, const BP &bp) {
    uint32_t sq[8], cu[12];
    nice::MsdFilterT<BP>::powers(n, sq, cu);
    nice::DigitBuf d;
    Bits s;
    nice::digits_of(sq, 8, bp, d);
    for (int i = 0; i < d.n; i++) s.add(d.d[i]);
    nice::digits_of(cu, 12, bp, d);
    for (int i = 0; i < d.n; i++) s.add(d.d[i]);
    return s.count();
}

template <class BP>
bool is_nice(u128 n, const BP &bp) {
    uint32_t sq[8], cu[12];
    nice::MsdFilterT<BP>::powers(n, sq, cu);
    nice::DigitBuf d;
    Bits s;
    nice::digits_of(sq, 8, bp, d);
    for (int i = 0; i < d.n; i++)
        if (!s.add(d.d[i])) return false;
    nice::digits_of(cu, 12, bp, d);
    for (int i = 0; i < d.n; i++)
        if (!s.add(d.d[i])) return false;
    // No digit-count test: the reference's get_is_nice returns true once both
    // scans finish without a repeat (client_process.rs:258-290), so below a
    // base's valid range an n whose digits are merely distinct is listed.
    return true;
}

struct Piece {
    std::vector<uint64_t> hist;
    std::vector<std::pair<u128, uint32_t>> list;
};

template <class BP>
void detailed_piece(u128 s, u128 e, const BP &bp, uint32_t cutoff, Piece &out) {
    out.hist.assign(bp.b + 1, 0);
    for (u128 n = s; n < e; n++) {
        const uint32_t u = unique_digits(n, bp);
        out.hist[u]++;
        if (u > cutoff) out.list.emplace_back(n, u);
    }
}

// Candidates of [s, e) in the stride table's residue sequence, nice ones appended.
template <class BP>
void niceonly_range(u128 s, u128 e, const BP &bp, const nice::StrideTable &t,
                    std::vector<u128> &out) {
    const size_t R = t.residues.size();
    if (!R) return;
    const u128 M = t.modulus;
    const u128 i0 = t.index_of(s), i1 = t.index_of(e);
    u128 cyc = i0 / R;
    size_t r = (size_t)(i0 - cyc * R);
    for (u128 g = i0; g < i1; g++) {
        const u128 n = cyc * M + t.residues[r];
        if (is_nice(n, bp)) out.push_back(n);
        if (++r == R) {
            r = 0;
            cyc++;
        }
    }
}

// The square's half of is_nice: n^2 has no repeated digit (get_is_nice
// reaches the cube scan, client_process.rs:222-253).
template <class BP>
bool square_free(u128 n, const BP &bp) {
    uint32_t sq[8], cu[12];
    nice::MsdFilterT<BP>::powers(n, sq, cu);
    nice::DigitBuf d;
    Bits s;
    nice::digits_of(sq, 8, bp, d);
    for (int i = 0; i < d.n; i++)
        if (!s.add(d.d[i])) return false;
    return true;
}

// One range of nice_cpu_process_ranges_niceonly: the stride walk of
// niceonly_range, which also counts the candidates and the repeat-free squares.
struct RangeAnswer {
    uint64_t candidates = 0;
    uint32_t square_ok = 0;
    uint64_t prefix_rejected = 0;
    std::vector<u128> nice;
};

// The sound filter's prefix mask of the range [s, e) of >= 2 numbers, by the
// digits themselves (no limb path: the device's msd_prefix_masks is checked
// against this): the digit mask of P2 + P3, the common leading digits of
// s^2, (e - 1)^2 and of the two cubes (none where the digit counts differ);
// all ones when P2 + P3 itself holds a repeat.
template <class BP>
void range_prefix_mask(u128 s, u128 e, const BP &bp, uint32_t pm[4]) {
    typedef nice::MsdFilterT<BP> F;
    uint32_t fsq[8], fcu[12], lsq[8], lcu[12];
    F::powers(s, fsq, fcu);
    F::powers(e - 1, lsq, lcu);
    nice::DigitBuf a, b;
    Bits seen;
    bool dup = false;
    auto common = [&] {
        if (a.n != b.n) return;
        const int c = F::common_msd(a, b);
        for (int i = 0; i < c; i++) dup |= !seen.add(a.d[a.n - 1 - i]);
    };
    nice::digits_of(fsq, 8, bp, a);
    nice::digits_of(lsq, 8, bp, b);
    common();
    nice::digits_of(fcu, 12, bp, a);
    nice::digits_of(lcu, 12, bp, b);
    common();
    for (int w = 0; w < 4; w++) pm[w] = dup ? ~0u : (uint32_t)(seen.w[w / 2] >> (32 * (w % 2)));
}

// Candidates [g0, g1) of the residue sequence, all inside the range [s, e).
// prefix: the range is one the prefix test runs on (nice_range_fast, the test
// asked for): a rejected candidate is counted and goes no further.
template <class BP>
void niceonly_range_counted(u128 s, u128 e, u128 g0, u128 g1, const BP &bp, const nice::StrideTable &t, bool prefix,
                            RangeAnswer &out) {
    const size_t R = t.residues.size();
    const u128 M = t.modulus;
    u128 cyc = g0 / R;
    size_t r = (size_t)(g0 - cyc * R);
    const int mw = (int)(bp.b + 31) / 32;
    const uint32_t multi = e - s > 1 ? 1u : 0u;
    uint32_t pm[4] = {0, 0, 0, 0};
    if (prefix && multi && g1 > g0) range_prefix_mask(s, e, bp, pm);
    for (u128 g = g0; g < g1; g++) {
        const u128 n = cyc * M + t.residues[r];
        bool gone = false;
        if (prefix) {  // radix_fast.hpp prefix_rejects
            for (int w = 0; w < mw; w++) gone |= (pm[w] & t.lowmask[r * mw + w]) != 0;
            gone |= multi && (t.residues_flagged[r] & nice::StrideTable::kLowDup);
        }
        if (gone) {
            out.prefix_rejected++;
        } else if (square_free(n, bp)) {
            out.square_ok++;
            if (is_nice(n, bp)) out.nice.push_back(n);
        }
        if (++r == R) {
            r = 0;
            cyc++;
        }
    }
}

int nthreads(int threads, u128 work);

// The ranges spread over the threads in pieces of at most kCpuPiece candidates
// (a range of 2^28 candidates would otherwise keep one thread busy alone); a
// range's pieces are added up in ascending order.
constexpr uint64_t kCpuPiece = 1u << 20;

template <class BP>
void ranges_niceonly_cpu(const BP &bp, const nice::StrideTable &t, const uint64_t *bounds, size_t n_ranges,
                         uint32_t k, bool prefix, int threads, std::vector<RangeAnswer> &ans) {
    struct Work {
        size_t range;
        u128 g0, g1;
        RangeAnswer part;
    };
    std::vector<Work> work;
    for (size_t i = 0; i < n_ranges; i++) {
        const u128 i0 = t.index_of(nice::range_at(bounds, i, 0)), i1 = t.index_of(nice::range_at(bounds, i, 1));
        ans[i].candidates = (uint64_t)(i1 - i0);
        for (u128 g = i0; g < i1; g += kCpuPiece) work.push_back(Work{i, g, std::min<u128>(g + kCpuPiece, i1), {}});
    }
    std::atomic<size_t> next{0};
    auto run = [&] {
        for (size_t q; (q = next.fetch_add(1)) < work.size();) {
            Work &w = work[q];
            const u128 s = nice::range_at(bounds, w.range, 0), e = nice::range_at(bounds, w.range, 1);
            // the test's domain is the GPU call's: the ranges its plan calls fast
            const bool pre = prefix && !t.lowmask.empty() && nice::nice_range_fast(bp.b, k, s, e);
            niceonly_range_counted(s, e, w.g0, w.g1, bp, t, pre, w.part);
        }
    };
    const int nt = nthreads(threads, work.size());
    std::vector<std::thread> ws;
    for (int i = 0; i + 1 < nt; i++) ws.emplace_back(run);
    run();  // the caller's thread
    for (auto &w : ws) w.join();
    for (const Work &w : work) {
        RangeAnswer &a = ans[w.range];
        a.square_ok += w.part.square_ok;
        a.prefix_rejected += w.part.prefix_rejected;
        a.nice.insert(a.nice.end(), w.part.nice.begin(), w.part.nice.end());
    }
}

int nthreads(int threads, u128 work) {
    int t = threads < 1 ? 1 : threads;
    if ((u128)t > work) t = work ? (int)work : 1;
    return t;
}

template <class BP>
int detailed_cpu(u128 s, u128 e, const BP &bp, int threads, uint64_t *hist, nice_number *out,
                 size_t cap, size_t *n_out) {
    const uint32_t cutoff = nice::near_miss_cutoff(bp.b);
    const u128 size = e - s;
    const int nt = nthreads(threads, size);
    std::vector<Piece> pieces(nt);
    std::vector<std::thread> ws;
    for (int i = 0; i < nt; i++) {
        const u128 a = s + size / nt * i + std::min<u128>(i, size % nt);
        const u128 b = s + size / nt * (i + 1) + std::min<u128>(i + 1, size % nt);
        if (i + 1 == nt) detailed_piece(a, b, bp, cutoff, pieces[i]);  // the caller's thread
        else ws.emplace_back([&, a, b, i] { detailed_piece(a, b, bp, cutoff, pieces[i]); });
    }
    for (auto &w : ws) w.join();
    size_t total = 0;
    for (uint32_t u = 0; u <= bp.b; u++) hist[u] = 0;
    for (auto &p : pieces) {
        for (uint32_t u = 0; u <= bp.b; u++) hist[u] += p.hist[u];
        total += p.list.size();
    }
    *n_out = total;
    if (total > cap) return cpu_fail(NICE_ERR_CAPACITY, "output capacity too small (n_out = required)");
    size_t k = 0;
    for (auto &p : pieces)
        for (auto &x : p.list)
            out[k++] = nice_number{(uint64_t)x.first, (uint64_t)(x.first >> 64), x.second, 0};
    return NICE_OK;
}

template <class BP>
int niceonly_cpu(u128 s, u128 e, const BP &bp, uint32_t k, int threads, bool sound, nice_number *out,
                 size_t cap, size_t *n_out) {
    // get_valid_ranges over the whole range (msd_prefix_filter.rs:665-674)
    std::vector<std::pair<u128, u128>> ranges;
    nice::MsdFilterT<BP> f(bp);
    f.valid_ranges(s, e, 0, 250, [&](u128 a, u128 b) { ranges.emplace_back(a, b); }, sound);
    const nice::StrideTable table(bp.b, k);
    const int nt = nthreads(threads, ranges.size());
    std::vector<std::vector<u128>> found(nt);
    std::vector<std::thread> ws;
    const size_t nr = ranges.size();
    for (int i = 0; i < nt; i++) {
        const size_t a = nr / nt * i + std::min<size_t>(i, nr % nt);
        const size_t b = nr / nt * (i + 1) + std::min<size_t>(i + 1, nr % nt);
        auto run = [&, a, b, i] {
            for (size_t q = a; q < b; q++) niceonly_range(ranges[q].first, ranges[q].second, bp, table, found[i]);
        };
        if (i + 1 == nt) run();
        else ws.emplace_back(run);
    }
    for (auto &w : ws) w.join();
    size_t total = 0;
    for (auto &v : found) total += v.size();
    *n_out = total;
    if (total > cap) return cpu_fail(NICE_ERR_CAPACITY, "output capacity too small (n_out = required)");
    size_t q = 0;
    for (auto &v : found)
        for (u128 n : v) out[q++] = nice_number{(uint64_t)n, (uint64_t)(n >> 64), bp.b, 0};
    return NICE_OK;
}

// Compile-time divisors for b10 and the niceonly fast bases
// (niceonly_bases.h), run-time otherwise.
template <class F>
int with_base(uint32_t base, F &&f) {
    switch (base) {
    case 10: return f(nice::CtBase<10>{});
#define X(b) case b: return f(nice::CtBase<b>{});
        NICE_NICEONLY_BASES(X)
#undef X
    default: return f(nice::RtBase(base));
    }
}

}  // namespace

namespace nice {
void set_last_error(const char *msg);  // abi_context.cpp: nice_last_error()'s thread-local message
}

namespace {
int cpu_fail(int code, const char *msg) {
    nice::set_last_error(msg);
    return code;
}
}  // namespace

extern "C" int nice_cpu_process_range_detailed(uint64_t start_lo, uint64_t start_hi, uint64_t end_lo,
                                               uint64_t end_hi, uint32_t base, int32_t threads,
                                               uint64_t *hist, nice_number *out, size_t cap,
                                               size_t *n_out) {
    if (!hist || !n_out || (cap && !out)) return cpu_fail(NICE_ERR_INVALID, "null output pointer");
    if (base < 2 || base > 128) return cpu_fail(NICE_ERR_INVALID, "base must be in 2..128");
    const u128 s = mk(start_lo, start_hi), e = mk(end_lo, end_hi);
    if (e < s) return cpu_fail(NICE_ERR_INVALID, "range end before start");
    return with_base(base, [&](const auto &bp) { return detailed_cpu(s, e, bp, threads, hist, out, cap, n_out); });
}

// nice_unique_map on the host cores: get_num_unique_digits per n
// (client_process.rs:47-143), the range split contiguously over the threads.
extern "C" int nice_cpu_unique_map(uint64_t start_lo, uint64_t start_hi, uint64_t end_lo, uint64_t end_hi,
                                   uint32_t base, int32_t threads, uint8_t *out, size_t cap) {
    if (!out) return cpu_fail(NICE_ERR_INVALID, "null out");
    if (base < 2 || base > 128) return cpu_fail(NICE_ERR_INVALID, "base must be in 2..=128");
    const u128 s = mk(start_lo, start_hi), e = mk(end_lo, end_hi);
    if (s >= e) return cpu_fail(NICE_ERR_INVALID, "range is empty or inverted");
    const u128 size = e - s;
    if (size > ((u128)1 << 32)) return cpu_fail(NICE_ERR_INVALID, "more than 2^32 numbers: map the range in pieces");
    if ((u128)cap < size) return cpu_fail(NICE_ERR_CAPACITY, "the map needs end - start bytes");
    return with_base(base, [&](const auto &bp) {
        const int nt = nthreads(threads, size);
        auto piece = [&](int i) {
            const u128 a = size / nt * i + std::min<u128>(i, size % nt);
            const u128 b = size / nt * (i + 1) + std::min<u128>(i + 1, size % nt);
            for (u128 k = a; k < b; k++) out[(size_t)k] = (uint8_t)unique_digits(s + k, bp);
        };
        std::vector<std::thread> ws;
        for (int i = 0; i + 1 < nt; i++) ws.emplace_back(piece, i);
        piece(nt - 1);  // the caller's thread
        for (auto &w : ws) w.join();
        return (int)NICE_OK;
    });
}

// The batched-ranges call on the host cores: the CPU path range by range.
extern "C" int nice_cpu_process_ranges_detailed(uint32_t base, const uint64_t *bounds, size_t n_ranges,
                                                uint32_t flags, int32_t threads, uint64_t *hist,
                                                nice_number *out, uint32_t *out_range, size_t cap,
                                                size_t *n_out) {
    if (!bounds || !hist || !n_out || (cap && !out)) return cpu_fail(NICE_ERR_INVALID, "null argument");
    if (base < 2 || base > 128) return cpu_fail(NICE_ERR_INVALID, "base must be in 2..128");
    if (flags > NICE_RANGES_SUM) return cpu_fail(NICE_ERR_INVALID, "bad flags");
    if (n_ranges == 0 || n_ranges > ((size_t)1 << 20))
        return cpu_fail(NICE_ERR_INVALID, "n_ranges must be in 1..2^20");
    for (size_t i = 0; i < n_ranges; i++)
        if (mk(bounds[4 * i], bounds[4 * i + 1]) >= mk(bounds[4 * i + 2], bounds[4 * i + 3]))
            return cpu_fail(NICE_ERR_INVALID, ("range " + std::to_string(i) + " is empty or inverted").c_str());
    const bool sum = flags == NICE_RANGES_SUM;
    const size_t nb = base + 1;
    std::vector<uint64_t> row(nb);
    std::vector<nice_number> list, one;
    std::vector<uint32_t> idx;
    if (sum) std::fill(hist, hist + nb, 0);
    for (size_t i = 0; i < n_ranges; i++) {
        const uint64_t *b = bounds + 4 * i;
        size_t n = 0;
        int rc = nice_cpu_process_range_detailed(b[0], b[1], b[2], b[3], base, threads, row.data(), one.data(),
                                                 one.size(), &n);
        if (rc == NICE_ERR_CAPACITY) {
            one.resize(n);
            rc = nice_cpu_process_range_detailed(b[0], b[1], b[2], b[3], base, threads, row.data(), one.data(),
                                                 one.size(), &n);
        }
        if (rc) return rc;
        for (size_t u = 0; u < nb; u++) {
            if (sum) hist[u] += row[u];
            else hist[i * nb + u] = row[u];
        }
        list.insert(list.end(), one.begin(), one.begin() + n);
        idx.insert(idx.end(), n, (uint32_t)i);
    }
    *n_out = list.size();
    if (list.size() > cap) return cpu_fail(NICE_ERR_CAPACITY, "output capacity too small (n_out = required)");
    for (size_t j = 0; j < list.size(); j++) {
        out[j] = list[j];
        if (out_range) out_range[j] = idx[j];
    }
    return NICE_OK;
}

// nice_process_ranges_niceonly_ex on the host cores: no MSD filter, every stride
// candidate of every range (stride_filter.rs:139-155) through get_is_nice --
// with the prefix test on, after that test on the ranges the GPU call runs it on.
extern "C" int nice_cpu_process_ranges_niceonly_ex(uint32_t base, const uint64_t *bounds, size_t n_ranges,
                                                   const nice_ranges_niceonly_opts *opts, int32_t threads,
                                                   uint64_t *candidates, uint32_t *square_ok,
                                                   uint64_t *prefix_rejected, nice_number *out, uint32_t *out_range,
                                                   size_t cap, size_t *n_out) {
    if (!bounds || !n_out || (cap && !out)) return cpu_fail(NICE_ERR_INVALID, "null argument");
    const nice_ranges_niceonly_opts o = opts ? *opts : nice_ranges_niceonly_opts{};
    if (o.prefix_test > NICE_RANGES_PREFIX_ON)
        return cpu_fail(NICE_ERR_INVALID, "prefix_test must be NICE_RANGES_PREFIX_OFF or NICE_RANGES_PREFIX_ON");
    if (o.reserved[0] || o.reserved[1]) return cpu_fail(NICE_ERR_INVALID, "reserved option words must be zero");
    const uint32_t k = o.stride_k ? o.stride_k : 2;
    if (const char *why = nice::nice_ranges_check(base, n_ranges, k)) return cpu_fail(NICE_ERR_INVALID, why);
    for (size_t i = 0; i < n_ranges; i++)
        if (nice::range_at(bounds, i, 0) >= nice::range_at(bounds, i, 1))
            return cpu_fail(NICE_ERR_INVALID, ("range " + std::to_string(i) + " is empty or inverted").c_str());
    std::vector<RangeAnswer> ans(n_ranges);
    if (!nice::residue_filter(base).empty()) {  // else: all-zero counts, no list
        const nice::StrideTable table(base, k);
        if (!table.residues.empty()) {
            for (size_t i = 0; i < n_ranges; i++)
                if (table.index_of(nice::range_at(bounds, i, 1)) - table.index_of(nice::range_at(bounds, i, 0)) >
                    nice::kNiceRangeCandMax)
                    return cpu_fail(NICE_ERR_INVALID,
                                    ("range " + std::to_string(i) + " holds more than 2^40 candidates: use a field")
                                        .c_str());
            with_base(base, [&](const auto &bp) {
                ranges_niceonly_cpu(bp, table, bounds, n_ranges, k, o.prefix_test == NICE_RANGES_PREFIX_ON, threads,
                                    ans);
                return 0;
            });
        }
    }
    size_t total = 0;
    for (size_t i = 0; i < n_ranges; i++) {
        if (candidates) candidates[i] = ans[i].candidates;
        if (square_ok) square_ok[i] = ans[i].square_ok;
        if (prefix_rejected) prefix_rejected[i] = ans[i].prefix_rejected;
        total += ans[i].nice.size();
    }
    *n_out = total;
    if (total > cap) return cpu_fail(NICE_ERR_CAPACITY, "output capacity too small (n_out = required)");
    size_t q = 0;
    for (size_t i = 0; i < n_ranges; i++)
        for (u128 n : ans[i].nice) {
            out[q] = nice_number{(uint64_t)n, (uint64_t)(n >> 64), base, 0};
            if (out_range) out_range[q] = (uint32_t)i;
            q++;
        }
    return NICE_OK;
}

extern "C" int nice_cpu_process_ranges_niceonly(uint32_t base, const uint64_t *bounds, size_t n_ranges,
                                                uint32_t stride_k, int32_t threads, uint64_t *candidates,
                                                uint32_t *square_ok, nice_number *out, uint32_t *out_range,
                                                size_t cap, size_t *n_out) {
    const nice_ranges_niceonly_opts o{stride_k, NICE_RANGES_PREFIX_OFF, {0, 0}};
    return nice_cpu_process_ranges_niceonly_ex(base, bounds, n_ranges, &o, threads, candidates, square_ok, nullptr,
                                               out, out_range, cap, n_out);
}

// nice_msd_ranges on the host cores: the host recursion root by root.
extern "C" int nice_cpu_msd_ranges(uint32_t base, const uint64_t *roots, size_t n_roots, uint64_t floor_size,
                                   uint32_t filter, int32_t threads, uint64_t *out, uint32_t *out_root,
                                   uint64_t *counts, size_t cap, size_t *n_out) {
    if (!roots || !n_out || (cap && !out)) return cpu_fail(NICE_ERR_INVALID, "null argument");
    if (filter > NICE_FILTER_SOUND)
        return cpu_fail(NICE_ERR_INVALID, "filter must be NICE_FILTER_REFERENCE or NICE_FILTER_SOUND");
    {
        const std::string why = nice::msd_ranges_check(base, roots, n_roots, floor_size);
        if (!why.empty()) return cpu_fail(NICE_ERR_INVALID, why.c_str());
    }
    const std::unique_ptr<nice::MsdRunner> msd = nice::make_msd(base);
    std::vector<std::vector<std::pair<u128, u128>>> ans(n_roots);
    std::atomic<size_t> next{0};
    auto run = [&] {
        for (size_t i; (i = next.fetch_add(1)) < n_roots;)
            msd->ranges(nice::range_at(roots, i, 0), nice::range_at(roots, i, 1), floor_size, ans[i],
                        filter == NICE_FILTER_SOUND);
    };
    const int nt = nthreads(threads, n_roots);
    std::vector<std::thread> ws;
    for (int i = 0; i + 1 < nt; i++) ws.emplace_back(run);
    run();  // the caller's thread
    for (auto &w : ws) w.join();
    size_t total = 0;
    for (size_t i = 0; i < n_roots; i++) {
        if (counts) counts[i] = ans[i].size();
        total += ans[i].size();
    }
    *n_out = total;
    if (total > cap) return cpu_fail(NICE_ERR_CAPACITY, "output capacity too small (n_out = required)");
    size_t q = 0;
    for (size_t i = 0; i < n_roots; i++)
        for (const auto &r : ans[i]) {
            out[4 * q] = (uint64_t)r.first, out[4 * q + 1] = (uint64_t)(r.first >> 64);
            out[4 * q + 2] = (uint64_t)r.second, out[4 * q + 3] = (uint64_t)(r.second >> 64);
            if (out_root) out_root[q] = (uint32_t)i;
            q++;
        }
    return NICE_OK;
}

extern "C" int nice_cpu_process_range_niceonly_ex(uint64_t start_lo, uint64_t start_hi, uint64_t end_lo,
                                                  uint64_t end_hi, uint32_t base, uint32_t stride_k,
                                                  int32_t threads, uint32_t filter, nice_number *out,
                                                  size_t cap, size_t *n_out) {
    if (filter > NICE_FILTER_SOUND) return cpu_fail(NICE_ERR_INVALID, "bad filter");
    if (!n_out || (cap && !out)) return cpu_fail(NICE_ERR_INVALID, "null output pointer");
    if (base < 2 || base > 128) return cpu_fail(NICE_ERR_INVALID, "base must be in 2..128");
    const uint32_t k = stride_k ? stride_k : 2;
    uint64_t bk = 1;
    for (uint32_t i = 0; i < k; i++) bk *= base;
    if (k > 4 || (base - 1) * bk > (1ull << 32)) return cpu_fail(NICE_ERR_INVALID, "stride table too large (k)");
    const u128 s = mk(start_lo, start_hi), e = mk(end_lo, end_hi);
    if (e < s) return cpu_fail(NICE_ERR_INVALID, "range end before start");
    *n_out = 0;
    if (s == e) return NICE_OK;
    const bool sound = filter == NICE_FILTER_SOUND;
    return with_base(base, [&](const auto &bp) { return niceonly_cpu(s, e, bp, k, threads, sound, out, cap, n_out); });
}

extern "C" int nice_cpu_process_range_niceonly(uint64_t start_lo, uint64_t start_hi, uint64_t end_lo,
                                               uint64_t end_hi, uint32_t base, uint32_t stride_k,
                                               int32_t threads, nice_number *out, size_t cap,
                                               size_t *n_out) {
    return nice_cpu_process_range_niceonly_ex(start_lo, start_hi, end_lo, end_hi, base, stride_k, threads,
                                              NICE_FILTER_REFERENCE, out, cap, n_out);
}
