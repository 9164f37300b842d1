// fd2_detailed.hip -- host side of the production FD detailed kernel: the
// limb-count cuts of each base's range, the per-segment dispatch to the
// per-base launchers (fd2_part*.hip) and the entry points of kernels.h.
#include <stdlib.h>

#include <map>
#include <mutex>

#include "fd2_combos.h"
#include "fd2_launch.hpp"
#include "fd2_map_kernel.hpp"
#include "unique_map.h"

namespace nice {
namespace fd2 {

NICE_PROBE_ONLY(u64 *g_stamps = nullptr; u64 g_last_launch[6] = {};)  // phase stamps, last launch (probe build)
std::atomic<uint32_t> g_force_sib_stride{0};  // nice_debug_force_sib_stride
std::atomic<uint32_t> g_force_sib_pers[2] = {{0}, {0}};  // nice_debug_force_sib_persistent: mode, workgroup cap

// ---------------------------------------------------------------------------
// Host: limb counts per segment.  For a segment [a, e) the last FD state a
// lane builds is for n = e (one step past its last number), so D1(e) = 2e+1,
// E1(e) = 3e^2+3e+1 and E2(e) = 6e+6 must fit ND, NE, NE2 radix-b^2 limbs.
// ---------------------------------------------------------------------------
struct Combo {
    int nd, ne, ne2;
};

static int limbs_of(const Nat &x, const std::vector<Nat> &pw) {
    int k = 0;
    while (k < (int)pw.size() && x.cmp(pw[k]) >= 0) k++;
    return k;  // smallest k with x < B^k
}

static Combo combo_at(uint32_t base, u128 e, const std::vector<Nat> &pw) {
    Nat n = Nat::from(e);
    Nat d1 = n;
    d1.mul_small(2);
    Nat one = Nat::from(1);
    auto add = [](Nat a, const Nat &b) {
        a.l.resize(std::max(a.l.size(), b.l.size()) + 1, 0);
        uint64_t c = 0;
        for (size_t i = 0; i < a.l.size(); i++) {
            uint64_t t = (uint64_t)a.l[i] + (i < b.l.size() ? b.l[i] : 0) + c;
            a.l[i] = (uint32_t)t;
            c = t >> 32;
        }
        a.trim();
        return a;
    };
    d1 = add(d1, one);
    Nat n3 = n;
    n3.mul_small(3);
    Nat e1 = add(add(n3.mul(n), n3), one);  // 3n^2 + 3n + 1
    Nat e2 = n;
    e2.mul_small(6);
    e2 = add(e2, Nat::from(6));
    (void)base;
    return Combo{limbs_of(d1, pw), limbs_of(e1, pw), limbs_of(e2, pw)};
}

struct BaseThresholds {
    std::vector<Nat> pw;       // B^k
    std::vector<u128> cuts;    // n where the combo changes, ascending, inside the range
    std::vector<Combo> combos; // combos[i]: segments ending in (cuts[i-1], cuts[i]]
};

static const BaseThresholds &thresholds(uint32_t base) {
    static std::mutex mu;
    static BaseThresholds cache[129];
    static bool have[129] = {};
    std::lock_guard<std::mutex> g(mu);
    BaseThresholds &t = cache[base];
    if (have[base]) return t;
    const uint32_t B = base * base;
    for (int k = 0; k < 40; k++) t.pw.push_back(Nat::pow(B, k));
    u128 rs = 0, re = 0;
    base_range(base, rs, re);
    // Walk the range: binary-search each change of combo_at.
    u128 a = rs;
    Combo cur = combo_at(base, a + 1, t.pw);
    t.combos.push_back(cur);
    while (true) {
        Combo last = combo_at(base, re, t.pw);
        if (last.nd == cur.nd && last.ne == cur.ne && last.ne2 == cur.ne2) break;
        u128 lo = a + 1, hi = re;  // smallest e in (a, re] whose combo differs
        while (lo < hi) {
            u128 mid = lo + (hi - lo) / 2;
            Combo c = combo_at(base, mid, t.pw);
            if (c.nd == cur.nd && c.ne == cur.ne && c.ne2 == cur.ne2) lo = mid + 1;
            else hi = mid;
        }
        // Segments ending at e <= lo - 1 use `cur`; the cut is at n = lo - 1
        // (a segment [x, lo-1) ends at e = lo - 1).
        t.cuts.push_back(lo - 1);
        a = lo - 1;
        cur = combo_at(base, lo, t.pw);
        t.combos.push_back(cur);
    }
    have[base] = true;
    return t;
}

// Per-base launchers, one object per part (fd2_part.hip).
hipError_t launch_part0(const DetailedLaunch &, int, int, int, bool, int, hipStream_t);
hipError_t launch_part1(const DetailedLaunch &, int, int, int, bool, int, hipStream_t);
hipError_t launch_part2(const DetailedLaunch &, int, int, int, bool, int, hipStream_t);
hipError_t launch_part3(const DetailedLaunch &, int, int, int, bool, int, hipStream_t);
hipError_t launch_part4(const DetailedLaunch &, int, int, int, bool, int, hipStream_t);
hipError_t launch_part5(const DetailedLaunch &, int, int, int, bool, int, hipStream_t);
static_assert(FD2_NPARTS == 6, "launch_part declarations");

// c: the limb counts of the segment's cut interval (cached in thresholds(),
// no bignum work per launch).
static hipError_t launch_segment(const DetailedLaunch &p, const Combo &c, int num_cus, hipStream_t s) {
    const int probe = (int)probe_knob("NICE_FD2_PROBE", 0);
#include NICE_PROBE_INC("fd2_detailed_probe_dispatch.inc")
    // Fields too small to fill the chip keep 512-thread workgroups (the
    // per-workgroup table build dominates there: b80 1e6 kernel 30 vs 38 us);
    // probe 20 forces them for b80 comparisons.
    const bool force512 = probe_knob("NICE_FD2_WG512", 0) != 0;
    const u64 small = probe_knob("NICE_FD2_SMALL", 10000000ull);  // probe: small-field threshold
    const bool wg512 = force512 || p.count < small || (probe == 20 && p.base == 80);
    using Fn = hipError_t (*)(const DetailedLaunch &, int, int, int, bool, int, hipStream_t);
    static const Fn parts[FD2_NPARTS] = {launch_part0, launch_part1, launch_part2,
                                         launch_part3, launch_part4, launch_part5};
    const hipError_t e = parts[fd2_part_of((int)p.base)](p, c.nd, c.ne, c.ne2, wg512, num_cus, s);
    return e == hipErrorNotFound ? hipErrorInvalidValue : e;
}

}  // namespace fd2

void fd2_force_sib_stride(uint32_t L) { fd2::g_force_sib_stride.store(L, std::memory_order_relaxed); }
void fd2_force_sib_persistent(uint32_t mode, uint32_t max_workgroups) {
    fd2::g_force_sib_pers[1].store(max_workgroups, std::memory_order_relaxed);
    fd2::g_force_sib_pers[0].store(mode, std::memory_order_relaxed);
}

bool fd2_supported(uint32_t base) {
    switch (base) {
#define X(b) case b:
        FD2_BASES(X)
#undef X
        return true;
    default: return false;
    }
}

bool fd2_window(uint32_t base, uint32_t *w0, uint32_t *w) {
    switch (base) {
#define X(b) case b: *w0 = fd2::window_w0(b), *w = fd2::window_w(b); return true;
        FD2_BASES(X)
#undef X
    default: return false;
    }
}

size_t fd2_cuts(uint32_t base, unsigned __int128 *out, size_t cap) {
    if (!fd2_supported(base)) return 0;
    const fd2::BaseThresholds &t = fd2::thresholds(base);
    for (size_t i = 0; i < t.cuts.size() && i < cap; i++) out[i] = t.cuts[i];
    return t.cuts.size();
}

// In-range segment [start, start + count): split at the limb-count cuts, one
// launch (plus a tail launch) per piece.
hipError_t launch_detailed_fd2(const DetailedLaunch &p, int num_cus, hipStream_t s) {
    if (!fd2_supported(p.base)) return hipErrorInvalidValue;
    const fd2::BaseThresholds &t = fd2::thresholds(p.base);
    u128 a = ((u128)p.start_hi << 64) | p.start_lo;
    const u128 e = a + p.count;
    DetailedLaunch q = p;
    // p.hist_copies: the same for every launch of the field (enqueue_detailed)
    if (p.hist_copies < kHistCopies) q.hist_copies = (uint32_t)probe_knob("NICE_FD2_COPIES", p.hist_copies);
    if (q.hist_copies < 1 || q.hist_copies > kHistCopies) q.hist_copies = kHistCopies;
    for (size_t i = 0; i <= t.cuts.size() && a < e; i++) {
        u128 stop = i < t.cuts.size() && t.cuts[i] < e ? t.cuts[i] : e;
        if (stop <= a) continue;
        q.start_lo = (uint64_t)a;
        q.start_hi = (uint64_t)(a >> 64);
        q.count = (uint64_t)(stop - a);
        q.fin = stop == e ? p.fin : FieldFinish{nullptr, nullptr, 0, 0};  // finish with the last launch
        hipError_t err = fd2::launch_segment(q, t.combos[i], num_cus, s);
        if (err != hipSuccess) return err;
        a = stop;
    }
    return hipSuccess;
}

// ---------------------------------------------------------------------------
// Batched ranges.
// ---------------------------------------------------------------------------
namespace fd2 {
using BatchFn = hipError_t (*)(const BatchLaunch &, int, int, int, const void *, uint32_t, hipStream_t);
hipError_t launch_batch_part0(const BatchLaunch &, int, int, int, const void *, uint32_t, hipStream_t);
hipError_t launch_batch_part1(const BatchLaunch &, int, int, int, const void *, uint32_t, hipStream_t);
hipError_t launch_batch_part2(const BatchLaunch &, int, int, int, const void *, uint32_t, hipStream_t);
hipError_t launch_batch_part3(const BatchLaunch &, int, int, int, const void *, uint32_t, hipStream_t);
hipError_t launch_batch_part4(const BatchLaunch &, int, int, int, const void *, uint32_t, hipStream_t);
hipError_t launch_batch_part5(const BatchLaunch &, int, int, int, const void *, uint32_t, hipStream_t);
static_assert(FD2_NPARTS == 6, "launch_batch_part declarations");
}  // namespace fd2

uint32_t fd2_batch_wg(uint32_t base) { return (uint32_t)fd2::small_wg((int)base); }  // BatchCfg::WG

// The base's TCHUNK (Cfg), made odd as rounds_chunk makes its chunks: odd
// chunks spread a wave's low-digit entries over distinct bank pairs, and are
// never a multiple of 16 (the bases without a low-digit table).
uint32_t fd2_batch_chunk(uint32_t base) { return (uint32_t)fd2::tchunk_of((int)base) + 1; }

void fd2_batch_plan(uint32_t base, u128 a, u128 e, uint32_t row, std::vector<BatchUnit> &out) {
    const fd2::BaseThresholds &t = fd2::thresholds(base);
    const u64 wg = fd2_batch_wg(base), tchunk = fd2_batch_chunk(base);
    for (size_t i = 0; i <= t.cuts.size() && a < e; i++) {
        const u128 stop = i < t.cuts.size() && t.cuts[i] < e ? t.cuts[i] : e;
        if (stop <= a) continue;
        const u128 cnt = stop - a;
        const fd2::BatchTile tile = fd2::batch_tile(cnt, wg, tchunk);
        const u64 chunk = tile.chunk, tail = tile.tail;
        u128 units = tile.units;
        u128 n = a;
        while (units) {
            const u64 lanes = units < wg ? (u64)units : wg;
            out.push_back(BatchUnit{(u64)n, (u64)(n >> 64), (uint32_t)lanes, (uint32_t)chunk, row, (uint32_t)i});
            n += (u128)lanes * chunk;
            units -= lanes;
        }
        if (tail) out.push_back(BatchUnit{(u64)n, (u64)(n >> 64), (uint32_t)tail, 1u, row, (uint32_t)i});
        a = stop;
    }
}

namespace fd2 {
// Whether the batch-configuration kernels' (batch, map) init_at reads a
// descriptor's xs (Cfg::N64, C64).
static bool unit_reads_digits(uint32_t base) {
    return fd2_supported(base) && reads_host_digits((int)base, small_wg((int)base));
}
// A descriptor's xs: zeros, or (`read`) the radix-b^2 digits of its first n.
static void unit_digits(uint32_t base, bool read, u64 lo, u64 hi, u32 *xs) {
    for (int k = 0; k < kXDigits; k++) xs[k] = 0;
    if (read) host_digits(((u128)hi << 64) | lo, base * base, xs, cdiv(digits_of((int)base).dn, 2));  // Cfg::B, NX
}
}  // namespace fd2

hipError_t launch_detailed_fd2_batch(const BatchLaunch &p, hipStream_t s) {
    if (!fd2_supported(p.base) || !p.n_units || p.n_units > 0x7fffffffull) return hipErrorInvalidValue;
    const fd2::BaseThresholds &t = fd2::thresholds(p.base);
    const size_t nc = t.combos.size();
    const bool digits = fd2::unit_reads_digits(p.base);
    // descriptors grouped by combo (a counting sort: the order within a combo
    // is the plan's, ascending n within a range)
    std::vector<size_t> first(nc + 1, 0);
    for (size_t i = 0; i < p.n_units; i++) {
        if (p.units[i].combo >= nc) return hipErrorInvalidValue;
        first[p.units[i].combo + 1]++;
    }
    for (size_t c = 0; c < nc; c++) first[c + 1] += first[c];
    std::vector<size_t> at(first.begin(), first.end() - 1);
    fd2::Fd2Unit *h = (fd2::Fd2Unit *)p.h_desc;
    static_assert(sizeof(fd2::Fd2Unit) == kBatchDescBytes, "descriptor size");
    for (size_t i = 0; i < p.n_units; i++) {
        const BatchUnit &u = p.units[i];
        fd2::Fd2Unit &d = h[at[u.combo]++];
        d.lo = u.lo;
        d.hi = u.hi;
        d.lanes = u.lanes;
        d.chunk = u.chunk;
        d.row = u.row;
        d.pad = 0;
        fd2::unit_digits(p.base, digits, u.lo, u.hi, d.xs);
    }
    hipError_t err = hipMemcpyAsync(p.d_desc, p.h_desc, p.n_units * kBatchDescBytes, hipMemcpyHostToDevice, s);
    if (err != hipSuccess) return err;
    static const fd2::BatchFn parts[FD2_NPARTS] = {fd2::launch_batch_part0, fd2::launch_batch_part1,
                                                   fd2::launch_batch_part2, fd2::launch_batch_part3,
                                                   fd2::launch_batch_part4, fd2::launch_batch_part5};
    for (size_t c = 0; c < nc; c++) {
        const size_t n = first[c + 1] - first[c];
        if (!n) continue;
        const fd2::Combo &cb = t.combos[c];
        err = parts[fd2_part_of((int)p.base)](p, cb.nd, cb.ne, cb.ne2,
                                              (const fd2::Fd2Unit *)p.d_desc + first[c], (uint32_t)n, s);
        if (err != hipSuccess) return err == hipErrorNotFound ? hipErrorInvalidValue : err;
    }
    return hipSuccess;
}

// ---------------------------------------------------------------------------
// Unique-count map (fd2_map_kernel.hpp; the launchers in fd2_map_part.hip).
// ---------------------------------------------------------------------------
namespace fd2 {
using MapFn = hipError_t (*)(uint32_t, int, int, int, const void *, uint32_t, unsigned char *, hipStream_t);
hipError_t launch_map_part0(uint32_t, int, int, int, const void *, uint32_t, unsigned char *, hipStream_t);
hipError_t launch_map_part1(uint32_t, int, int, int, const void *, uint32_t, unsigned char *, hipStream_t);
hipError_t launch_map_part2(uint32_t, int, int, int, const void *, uint32_t, unsigned char *, hipStream_t);
hipError_t launch_map_part3(uint32_t, int, int, int, const void *, uint32_t, unsigned char *, hipStream_t);
hipError_t launch_map_part4(uint32_t, int, int, int, const void *, uint32_t, unsigned char *, hipStream_t);
hipError_t launch_map_part5(uint32_t, int, int, int, const void *, uint32_t, unsigned char *, hipStream_t);
static_assert(FD2_NPARTS == 6, "launch_map_part declarations");
}  // namespace fd2

// The map kernel is the batch kernel's configuration (MapCfg): its workgroup
// size and its odd target chunk.
MapBase map_base(uint32_t base) {
    MapBase b;
    u128 rs = 0, re = 0;
    if (!fd2_supported(base) || base_range_cached(base, rs, re) != 1) return b;
    b.fd = true;
    b.rs = rs;
    b.re = re;
    b.cuts = fd2::thresholds(base).cuts;
    b.wg = fd2_batch_wg(base);
    b.tchunk = fd2_batch_chunk(base);
    return b;
}

hipError_t launch_unique_map(const MapLaunch &p, hipStream_t s) {
    const bool fd = fd2_supported(p.base);
    const fd2::BaseThresholds *t = fd ? &fd2::thresholds(p.base) : nullptr;
    const bool digits = fd2::unit_reads_digits(p.base);
    fd2::Fd2MapUnit *h = (fd2::Fd2MapUnit *)p.h_desc;
    static_assert(sizeof(fd2::Fd2MapUnit) == kMapDescBytes, "descriptor size");
    size_t nu = 0;
    for (size_t i = 0; i < p.n_recs; i++) {
        const MapRec &r = p.recs[i];
        if (r.kind != kMapFd) continue;
        if (!fd || r.combo >= t->combos.size()) return hipErrorInvalidValue;
        fd2::Fd2MapUnit &d = h[nu++];
        d.lo = r.lo;
        d.hi = r.hi;
        d.off = r.off;
        d.lanes = r.lanes;
        d.chunk = r.chunk;
        fd2::unit_digits(p.base, digits, r.lo, r.hi, d.xs);
    }
    hipError_t err;
    if (nu && (err = hipMemcpyAsync(p.d_desc, p.h_desc, nu * kMapDescBytes, hipMemcpyHostToDevice, s)) != hipSuccess)
        return err;
    static const fd2::MapFn parts[FD2_NPARTS] = {fd2::launch_map_part0, fd2::launch_map_part1,
                                                 fd2::launch_map_part2, fd2::launch_map_part3,
                                                 fd2::launch_map_part4, fd2::launch_map_part5};
    size_t at = 0;  // FD records before record i
    for (size_t i = 0; i < p.n_recs;) {
        const MapRec &r = p.recs[i];
        if (r.kind != kMapFd) {
            if ((err = launch_generic_map(r.lo, r.hi, r.count, p.base, p.out + r.off, s)) != hipSuccess) return err;
            i++;
        } else {
            size_t j = i;  // the run of FD records of this limb layout
            while (j < p.n_recs && p.recs[j].kind == kMapFd && p.recs[j].combo == r.combo) j++;
            if (j - i > 0x7fffffffull) return hipErrorInvalidValue;
            const fd2::Combo &cb = t->combos[r.combo];
            err = parts[fd2_part_of((int)p.base)](p.base, cb.nd, cb.ne, cb.ne2,
                                                  (const fd2::Fd2MapUnit *)p.d_desc + at, (uint32_t)(j - i), p.out, s);
            if (err != hipSuccess) return err == hipErrorNotFound ? hipErrorInvalidValue : err;
            at += j - i;
            i = j;
        }
        if (p.launches) ++*p.launches;
    }
    return hipSuccess;
}

}  // namespace nice

#include NICE_PROBE_INC("fd2_detailed_probe_exports.inc")
