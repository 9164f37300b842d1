// fd2_plan.hpp -- how a segment of an FD detailed field is cut into launches
// and how each launch is shaped: the chunk rule, the regular (rounds /
// persistent-grid) launch, the sibling-lane decision with its lane-stride
// pickers, and the sibling launch.  Pure arithmetic templated on the kernel
// configuration (fd2_cfg.hpp Cfg): no GPU runtime, no globals, no environment,
// so every rule here can be checked on a CPU (tests/test_fd2_plan.py).  The
// launchers (fd2_launch.hpp) read the knobs, ask for a plan and fill the
// kernel arguments from it.
#pragma once

#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <vector>

#include "layout.h"

namespace nice {
namespace fd2 {

// Radix-B digits of n, least significant first (Fd2Args::xs / xt).
static inline void host_digits(u128 n, u32 B, u32 *out, int nx) {
    for (int i = 0; i < nx; i++) {
        out[i] = (u32)(n % B);
        n /= B;
    }
}

// ---------------------------------------------------------------------------
// Lane stride from a bank-conflict model.  A wave's lanes sit `L` numbers
// apart (one chunk each), so the value of a HIGH limb across the lanes is an
// arithmetic progression whose step is f'(n) L / B^q (f = n^2, n^3).  A
// table lookup costs, per pass of 32 lanes (8-byte entries) or 16 lanes
// (16-byte entries), the largest number of distinct entries that share a
// bank slot (entry mod 32 / mod 16): 1-2 for a progression with an odd step,
// up to 32 for a step that is a multiple of 32 -- e.g. b40's top C limb
// steps ~32 per lane at L = 125 from the range start (modelled 91 against
// 63 LDS cycles per wave-step, measured 2.35 against 1.86 ms per 1e9 in the
// sibling kernel), and L = 81 hits the same 10 % into the range (2.37 vs
// 1.90 ms; profiles/r05/sib_chunk_sweep.log).  The low limbs' values are
// effectively random whatever L is, so the model counts only the limbs
// whose value f / B^q stays below 2^60 (long double keeps their integer
// part), at a few points of the segment and of the chunk, and the launch
// takes the candidate stride with the smallest modelled cost.
// ---------------------------------------------------------------------------
// Cost of one lookup pass (`slots` lanes on `slots` bank slots) whose lane
// values are floor(a + d l) mod B, as a function of the step d at a
// resolution of 1/64, averaged over the offset a: max distinct values per
// slot.  The pattern of slots depends on d mod slots, but whether lanes
// share a value (a broadcast, free) only on d itself, so the table covers
// d in [0, 2 slots): steps >= slots are looked up at slots + d mod slots.
// Simulated once per process.
static const std::vector<float> &progression_cost(int slots) {
    static std::mutex mu;
    static std::map<int, std::vector<float>> tab;
    std::lock_guard<std::mutex> g(mu);
    auto it = tab.find(slots);
    if (it != tab.end()) return it->second;
    std::vector<float> t((size_t)slots * 128);
    for (size_t k = 0; k < t.size(); k++) {
        const double d = (double)k / 64;
        double sum = 0;
        for (int ai = 0; ai < 16; ai++) {
            const double a = ai / 16.0 + 0.03125;
            // the lane values floor(a + d l) never decrease with l, so a
            // value repeats only in consecutive lanes (a broadcast)
            int cnt[32] = {};
            int best = 0;
            long prev = -1;
            for (int l = 0; l < slots; l++) {
                const long v = (long)(a + d * l);  // a + d l >= 0: truncation is floor
                if (v == prev) continue;
                prev = v;
                const int sl = (int)(v & (slots - 1));  // slots: 16 or 32
                best = std::max(best, ++cnt[sl]);
            }
            sum += best;
        }
        t[k] = (float)(sum / 16);
    }
    return tab.emplace(slots, std::move(t)).first->second;
}

// Modelled LDS cycles of a wave-step's lookups of the limbs whose lane
// values progress (the high looked-up limbs of S = n^2 and C = n^3 from
// first_limb on, where the lanes' quadratic drift stays under half a unit)
// at lane stride L, averaged over the segment's start, middle and end.  The
// other limbs' values are effectively random whatever L is and are left out.
// Per limb and point the lane step is c L and the drift k L^2 (c = f'(n) /
// B^q, k = f''(n) 64^2 / 2 / B^q), so the strides of one pick share them.
template <class P>
struct ConflictModel {
    static constexpr int SLOTS = P::ES == 16 ? 16 : 32;
    static constexpr int NPASS = 64 / SLOTS;
    int n = 0;
    double c[3 * (P::SL + P::CL)], k[3 * (P::SL + P::CL)];
    const std::vector<float> *tab;
    ConflictModel(long double n0, long double span, int first_limb) : tab(&progression_cost(SLOTS)) {
        for (int pt = 0; pt < 3; pt++) {
            const long double x = n0 + span * (long double)pt / 2;
            for (int cube = 0; cube < 2; cube++) {
                const int hi = cube ? P::CL : P::SL;
                long double bq = 1;
                for (int q = 0; q < first_limb; q++) bq *= (long double)P::B;
                for (int q = first_limb; q < hi; q++, bq *= (long double)P::B) {
                    if (cube ? P::vd_c(q) : P::vd_s(q)) continue;
                    const long double f1 = cube ? 3 * x * x : 2 * x;  // f'(n)
                    const long double f2 = cube ? 6 * x : 2;          // f''(n)
                    c[n] = (double)(f1 / bq);
                    k[n] = (double)(f2 * 4096 / 2 / bq);
                    n++;
                }
            }
        }
    }
    double cost(u64 L) const {
        double sum = 0;
        const double l = (double)L;
        for (int i = 0; i < n; i++) {
            if (k[i] * l * l >= 0.5) continue;  // drifting: effectively random
            // the lane step in limb units: < 2^24 for every limb that passes
            // the drift test, so double keeps its fraction
            const double d = c[i] * l;
            const double r = d < SLOTS ? d : SLOTS + (d - SLOTS * std::floor(d / SLOTS));
            sum += NPASS * (*tab)[std::min<size_t>(tab->size() - 1, (size_t)(r * 64))];
        }
        return sum / 3;
    }
};

// The odd stride in [lo, hi] with the lowest modelled cost at the segment
// [start, start + count); among the strides within `tol` modelled cycles of
// the best, the one closest to target (a lane's init amortises over its
// chunk).  A few hundred table lookups: cheap enough for every launch.
// (A rounds-aware pick -- the stride whose units fill whole rounds of the
// resident lanes, times L plus init steps -- chose L ~ 130-160 and lost on
// small fields: b40 1e8 0.261 ms against 0.227 at L = 65, and did not gain at
// 1e9; profiles/r05/picker_rounds.log.)
template <class P>
static u64 pick_lane_stride(u128 start, u64 count, u64 lo, u64 hi, u64 target, int first_limb,
                            double tol = 0.5) {
    const ConflictModel<P> m((long double)start, (long double)count, first_limb);
    double cost[512];
    int nc = 0;
    double min_cost = 1e30;
    for (u64 L = lo | 1; L <= hi && nc < 512; L += 2, nc++) {
        cost[nc] = m.cost(L);
        min_cost = std::min(min_cost, cost[nc]);
    }
    u64 best = target | 1, best_d = ~0ull;
    nc = 0;
    for (u64 L = lo | 1; L <= hi && nc < 512; L += 2, nc++) {
        const u64 d = L > target ? L - target : target - L;
        if (cost[nc] <= min_cost + tol && d < best_d) {
            best = L;
            best_d = d;
        }
    }
    return best;
}

// The stride for fields of a few rounds (fewer than 3 at the target
// stride): among the odd L in [lo, hi] the model does not flag, the one
// whose units fill the fewest whole rounds of the resident lanes per step of
// work, ceil(Q (ceil(D / L) - 1) / lanes) (L + init).  A part-filled last
// round costs a whole one there: b40 1e8 (13 super-blocks) takes 0.227 ms at
// L = 65 (1.95 rounds), 0.270 at L = 63 (2.01) and 0.259 at 61 (2.08); 9e7 is
// best at 61 (1.76 rounds; profiles/r05/sib_small_L.log).  Sets `rounds`.
template <class P>
static u64 pick_small_stride(u128 start, u64 count, u64 lo, u64 hi, int first_limb, u64 Q, u64 lanes, u64 D,
                             double &rounds, double init = 6, double tol = 6) {
    const ConflictModel<P> m((long double)start, (long double)count, first_limb);
    double cost[512];
    int nc = 0;
    double min_cost = 1e30;
    for (u64 L = lo | 1; L <= hi && nc < 512; L += 2, nc++) {
        cost[nc] = m.cost(L);
        min_cost = std::min(min_cost, cost[nc]);
    }
    u64 best = lo | 1;
    double best_t = 1e300;
    rounds = 0;
    nc = 0;
    for (u64 L = lo | 1; L <= hi && nc < 512; L += 2, nc++) {
        if (cost[nc] > min_cost + tol) continue;
        const u64 units = Q * ((D + L - 1) / L - 1);
        const double t = (double)((units + lanes - 1) / lanes) * ((double)L + init);
        if (t < best_t) {
            best_t = t;
            best = L;
            rounds = (double)units / (double)lanes;
        }
    }
    return best;
}

// ---------------------------------------------------------------------------
// Launch plans.  Small structs returned by value: nothing on the launch path
// allocates (small fields are bound by host latency).
// ---------------------------------------------------------------------------

// What the probe build's environment knobs override (NICE_FD2_TCHUNK,
// NICE_FD2_MINCHUNK, NICE_FD2_SIBCHUNK, NICE_FD2_SIBROUNDS); the product
// passes none.
template <class P>
struct PlanKnobs {
    // Target numbers per lane.  Short chunks put a wave's 64 lanes on nearby n,
    // so the top stepped limbs (and the cached ones) of neighbouring lanes are
    // equal or close and their lookups stop conflicting; a chunk still pays
    // one init (radix-B conversion and products, ~10 steps).  Without PERS
    // each lane takes one chunk and the grid is many rounds of workgroups:
    // with two or more workgroups per CU, workgroups at different phases
    // (table DMA, init, steps, draining) share a CU (b40 1e9 round 1: 2.49 ms
    // persistent with static lane assignment at chunk 637, 2.31 at ~80,
    // 2.19-2.21 in rounds, profiles/r01/fd2_chunk_sweep.log).
    u64 tchunk = (u64)P::TCHUNK;
    // Chunk floor for fields too small to fill the chip: a lane's init costs
    // about ten steps, but with idle CUs latency wins (b40 1e6: kernel 25 us at
    // a floor of 32, 14 us at 4; scripts/small_fields.py).
    u64 min_chunk = 4;
    u64 sib_chunk = 0;    // a sibling lane stride instead of the pickers' (0: none)
    u64 sib_rounds = 15;  // tenths of a round below which a small field leaves the sibling kernel
    // Persistent sibling grid (Cfg::SIBPERS, plan_sib_pers): a segment takes
    // it at or above sib_pers_min tenths of a wave batch per resident wave;
    // the grid is sib_pers_k rounds of resident workgroups (1: one round).
    u64 sib_pers_min = 40;
    u64 sib_pers_k = 1;
    // the test hook's (nice_debug_force_sib_persistent): mode 1 = on for every
    // sibling segment, with at most sib_pers_max_wg workgroups when nonzero;
    // mode 2 = never
    u32 sib_pers_mode = 0, sib_pers_max_wg = 0;
};

// Rounds of one chunk per lane: `cnt` numbers over whole rounds of `lanes`
// resident lanes, chunks <= the target and <= cap (the low-digit table's
// reach), at least `floor` where the numbers allow.
//
// odd: the chunk is made odd.  Lane l of a wave then sits at n mod B = r0 +
// chunk * l, so its low-digit entries fall on 32 distinct bank pairs per
// half-wave (B is a multiple of 32 for the LSD bases).  Otherwise (no
// low-digit table, b80) limb 0 of n^2 and n^3 is looked up in the pair table,
// and a chunk divisible by 16 puts a 16-lane group on ONE bank quad for those
// lookups (n^2 mod 16 equal on every lane): b80 1e9 at chunk 2544 took 11.8
// ms, at 2545 9.3; so there the chunk only avoids the multiples of 16.
//
// (The bank-conflict model that picks the sibling kernel's lane stride,
// pick_lane_stride, did not help the persistent-grid kernels of the wider
// bases: re-picking their chunk where it modelled a pathology moved b45..80
// by -5 .. +9 %, profiles/r05/model_sweep.log, model_sweep2.log.)
static inline u64 rounds_chunk(u64 cnt, u64 lanes, u64 tchunk, u64 floor, bool odd, u64 cap) {
    u64 rounds = (cnt + tchunk * lanes - 1) / (tchunk * lanes);
    if (rounds < 1) rounds = 1;
    u64 chunk = (cnt + rounds * lanes - 1) / (rounds * lanes);
    if (chunk < floor) chunk = cnt < floor ? cnt : floor;
    if (chunk < 1) chunk = 1;
    if (chunk > 1 && (odd ? chunk % 2 == 0 : chunk % 16 == 0)) chunk++;
    if (chunk > cap) chunk = cap % 2 ? cap : cap - 1;
    return chunk;
}

// The batch kernel's tiling of one piece of a range (fd2_batch_plan): whole
// workgroups of chunks <= the base's target, as rounds_chunk's whole rounds:
// the fewest workgroups that hold the piece, then the chunk that fills them
// (so the last main workgroup is nearly full).  A piece of <= WG numbers is
// one workgroup of one number per lane (a lane's steps are the latency of a
// small range).  No floor and no cap: tchunk is odd and <= B.
struct BatchTile {
    u64 chunk;   // numbers per lane of the main workgroups
    u128 units;  // lanes of `chunk` numbers
    u64 tail;    // numbers left over (< chunk): one tail workgroup, one per lane
};
static inline BatchTile batch_tile(u128 cnt, u64 wg, u64 tchunk) {
    const u128 nwg = (cnt + (u128)wg * tchunk - 1) / ((u128)wg * tchunk);
    u64 chunk = (u64)((cnt + nwg * wg - 1) / (nwg * wg));
    if (chunk > 1 && chunk % 2 == 0) chunk++;  // <= tchunk, which is odd
    const u128 units = cnt / chunk;
    return BatchTile{chunk, units, (u64)(cnt - units * chunk)};
}

// The persistent grid pays off where ONE workgroup fills a CU and the
// segment needs at least two rounds of them; otherwise (a device with other
// occupancy, short segments) the same kernel in rounds (Cfg::NoPers).
// per_cu_q: the runtime's occupancy answer, unclamped.
template <class P>
static bool pers_suits(u64 count, int num_cus, int per_cu_q, const PlanKnobs<P> &k = PlanKnobs<P>{}) {
    return per_cu_q == 1 && count >= 2 * k.tchunk * ((u64)num_cus * P::WG);
}

// One regular launch (Cfg::SIB == 1): the first `cnt` of the `left` numbers.
// Blocks [0, main_blocks) walk nunits chunks of `chunk` numbers, the blocks
// after them the `tail` < chunk numbers left over, one per lane.
struct RegularPlan {
    bool ok;  // false: no launch of this shape holds even one number (invalid value)
    u64 cnt, chunk, nunits, tail, grid, main_blocks;
    u32 wave_cap;  // persistent grid: batches one wave may take (its lanes' u16 counters hold them)
};
template <class P>
static RegularPlan plan_regular(u64 left, int num_cus, int per_cu, const PlanKnobs<P> &k = PlanKnobs<P>{}) {
    // Resident lanes (one "round" of workgroups).
    const u64 lanes = (u64)num_cus * per_cu * P::WG;
    // Launch size bound (nunits fits 32 bits).  A lane takes ONE chunk per
    // launch, so its window counters count at most chunk <= TCHUNK numbers
    // (u16 halves; u8 quarters need chunk <= 255, checked below).
    const u64 max_count = lanes * 60000ull;
    const u64 nw = P::WG / 64;
    RegularPlan pl{};
    pl.cnt = left < max_count ? left : max_count;
    for (;;) {
        pl.chunk = rounds_chunk(pl.cnt, lanes, k.tchunk, k.min_chunk, P::LSD, P::B);
        if (P::HQ == 4 && pl.chunk > 255) return pl;
        pl.nunits = pl.cnt / pl.chunk;
        pl.tail = pl.cnt - pl.nunits * pl.chunk;  // < chunk <= B: one number per lane
        bool fits = pl.nunits <= 0xffffffffull;
        if constexpr (P::PERS) {
            // one round of resident workgroups (fewer when the batches
            // run out); the batch count stays in 32 bits and every
            // workgroup's batches fit its waves' caps (u16 counters)
            const u64 nb = (pl.nunits + 63) / 64 + (pl.tail + 63) / 64;
            pl.grid = std::min<u64>((u64)num_cus * per_cu, (nb + nw - 1) / nw);
            fits = fits && pl.nunits <= 0xffffffc0ull && (nb + pl.grid - 1) / pl.grid <= nw * (65535 / pl.chunk);
        } else {
            pl.grid = (pl.nunits + P::WG - 1) / P::WG + (pl.tail + P::WG - 1) / P::WG;
        }
        if (fits) break;
        // Too much for one launch of this shape: split the segment (the
        // finish rides on the last launch, so any split is exact).
        if (pl.cnt < 2) return pl;
        pl.cnt /= 2;
    }
    pl.main_blocks = (pl.nunits + P::WG - 1) / P::WG;  // one chunk per lane
    pl.wave_cap = (u32)(65535 / pl.chunk);
    pl.ok = true;
    return pl;
}

// Sibling lanes (Cfg::SIB = M > 1).  A segment [a, a + count) is
// Q super-blocks of M B^2 numbers plus a remainder R < M B^2.  Super-block q
// is walked by units (q, k): a lane takes the numbers a + q M B^2 + j B^2 +
// k L + i (j < M, i < L) for k < B^2 / L, and the last L' = B^2 mod L (or L)
// numbers of each B^2 block are the edge units (one per super-block, chunk
// L'); the remainder R runs as the regular main + tail parts of the same
// launch.  Launches are split so unit counts stay 32-bit; the field's finish
// rides on the last.
//
// The decision for a segment: the kernel without siblings (Cfg::NoSib), an
// invalid value, or the lane stride L with the split of a B^2 block it gives.
struct SibShape {
    enum Kind { kNoSib, kError, kSib } kind;
    u64 L;          // lane stride = sibling chunk (odd)
    u64 U, upb, r;  // units per B^2 block: upb full ones of L numbers, and the edge unit of r (when r != L)
    bool has_edge;
    u64 qmax;       // super-blocks per launch
    // persistent sibling grid (plan_sib_pers; pers false: rounds)
    bool pers;
    u64 pers_grid;  // workgroups of a launch's sibling part, at most
    u32 wave_cap;   // batches one wave may take: wave_cap M L <= 65535
};
// Too short for the sibling walk to pay (fewer than 4 super-blocks): the same
// base without siblings.  The launcher asks this first, before it builds the
// sibling kernel's tables.
template <class P>
static bool sib_too_short(u64 count) {
    return count < 4 * ((u64)P::SIB * P::B * P::B);
}
// forced: the test hook's stride (0: none).
template <class P>
static SibShape plan_sib(u128 seg_start, u64 count, int num_cus, int per_cu, bool overlapped, u64 forced,
                         const PlanKnobs<P> &k = PlanKnobs<P>{}) {
    constexpr u64 D = (u64)P::B * P::B, SB = (u64)P::SIB * D;
    const u64 lanes = (u64)num_cus * per_cu * P::WG;
    SibShape sh{};
    sh.kind = SibShape::kNoSib;
    if (sib_too_short<P>(count)) return sh;
    // Sibling chunk L: odd, so limb 0's low-digit lookups of a half-wave hit
    // 32 distinct bank pairs (as rounds_chunk's chunks).
    u64 L = k.sib_chunk;
    // a stride forced by the test hook also skips the small-field fallback
    // below (every stride the pickers can return is then reachable on a
    // field of >= 4 super-blocks)
    if (!L) L = forced;
    // Fields of fewer than 6 rounds of the resident lanes' units at the
    // target stride: the part-filled last round of the 4-wave grid decides,
    // so the stride fills rounds (pick_small_stride over [60, 100]), and
    // below ~1.5 rounds the regular kernel's finer grid wins (b40 1e8:
    // sibling 0.227-0.239 ms at L = 65 against 0.242-0.265 regular, 1.25e8
    // 0.263-0.289 against 0.282-0.307; 9e7 ties; profiles/r05/
    // sib_small_L.log; the 4- and 8-way shards of the bench field,
    // shard_projection.log).
    // A field that overlaps a running one (pipelined submits) shares the chip
    // with it, so no round is part-filled and the per-number cost decides:
    // the large-field pick.  The 8-way shard of the bench field (1.25e8),
    // pipelined: 0.2412 ms per step at L = 105, 0.2422 at 81, 0.2481 at the
    // small-field pick (79 / 81 / 65 by shard); 2.5e8 0.486 / 0.494 / 0.500,
    // 5e7 0.110 / 0.113 / 0.112, 1e8 0.1940 / 0.1938 / 0.1952, and L = 125
    // 20-25 % slower everywhere (profiles/r06/exchange/small_L_pipe.log).
    const u64 Q0 = count / SB;
    if (!L && !overlapped && 10 * Q0 * (D / P::TCHUNK) < 60 * lanes) {
        double rounds = 0;
        L = pick_small_stride<P>(seg_start, count, P::TCHUNK * 3 / 4, P::TCHUNK * 5 / 4, P::LO + 1, Q0, lanes, D,
                                 rounds);
        // (the persistent grid forced on by the test hook keeps such a field)
        if (10 * rounds < (double)k.sib_rounds && k.sib_pers_mode != 1) return sh;
    }
    // Target stride: TCHUNK, or 140 for the pipelined walk (LG >= 100), which
    // fills and drains its lookup pipeline once per unit and so gains from
    // longer units.  b40 bench field (pipelined, stride swept over odd L in
    // [61, 255] against the pick, profiles/r06/stride/): target 80 picked
    // 65 at 1e9 (1.917 ms per field), target 140 picks 143 (-2.5 %) there and
    // 159 at 1.25e8 (-2.7 %); a quarter into the range -0.6 / -2.8 %.  The
    // per-sibling-lookup kernels (LG 1, b40 beyond the first limb layout and
    // b42..55) gain nothing consistent from longer targets (b42 1.25e8 +14 %
    // at 140), so they keep TCHUNK.
    constexpr u64 T = P::LG >= 100 ? 140 : (u64)P::TCHUNK;
    // A lone field of the pipelined walk (a synchronous caller, the reference
    // client's pattern: nothing overlaps its last round) picks over the same
    // range by whole rounds, as the small-field path does: b40 1e9 alone
    // 1875-1887 us at L = 159 (7.99 rounds) against 1890-1947 at the model's
    // 143 (8.9 rounds), 5e8 953 against 973-1012 (profiles/r06/stride/
    // iso_L.log).  Pipelined fields keep the model's pick (no last round).
    if (!L && P::LG >= 100 && !overlapped) {
        double rounds = 0;
        L = pick_small_stride<P>(seg_start, count, T * 3 / 4, T * 3 / 2, P::LO + 1, Q0, lanes, D, rounds);
    }
    if (!L) L = pick_lane_stride<P>(seg_start, count, T * 3 / 4, T * 3 / 2, T, P::LO + 1);
    // chunks reach low-digit entries n mod B + i < LDE (Cfg::LDE)
    constexpr u64 LMAX = (u64)P::LDE - P::B;
    if (L % 2 == 0) L++;
    if (L > D / 4) L = (D / 4) | 1;
    if (L > LMAX) L = LMAX % 2 ? LMAX : LMAX - 1;
    sh.L = L;
    sh.U = (D + L - 1) / L;
    sh.r = D - (sh.U - 1) * L;
    sh.has_edge = sh.r != L;
    sh.upb = sh.has_edge ? sh.U - 1 : sh.U;
    // the lanes' u16 window counters hold M L numbers
    if ((u64)P::SIB * L > 65535) {
        sh.kind = SibShape::kError;
        return sh;
    }
    // Launch bound: unit counts in 32 bits and, as plan_regular's, 60 000
    // numbers per resident lane -- counted at the regular kernel's 2048 lanes
    // per CU, so a b40 launch still takes up to 3.1e10 numbers whatever the
    // sibling kernel's own occupancy.
    sh.qmax = std::max<u64>(1, std::min<u64>(0xffffffffull / sh.upb, ((u64)num_cus * 2048 * 60000ull) / SB));
    sh.kind = SibShape::kSib;
    return sh;
}

// One sibling launch: the first `cnt` of the `left` numbers as Q super-blocks
// and, on the segment's last launch only, the remainder R as regular main +
// tail parts (rounds of one chunk per lane, chunks within the sibling
// kernel's low-digit table).
struct SibLaunchPlan {
    u64 Q, cnt, R;
    u64 chunk, nunits, tail;  // the remainder's parts
    u64 sib_units, sib_blocks, edge_units, edge_blocks, main_blocks, grid;
    // persistent sibling grid (sh.pers): the launch's 64-unit batches (the
    // sibling units', then the edge units'), walked by sib_blocks workgroups
    // whose waves take at most wave_cap each; edge_blocks is 0
    u64 batches;
    u32 wave_cap;
};

// Whether a sibling segment takes the persistent grid (Cfg::SIBPERS), and its
// shape: sets sh.pers, sh.pers_grid, sh.wave_cap.  One round of resident
// workgroups (k.sib_pers_k rounds: each workgroup then lives 1 / k of the
// field, which lets another stream's launch in sooner); a wave stops after
// wave_cap batches, so its lanes' u16 window counters, which count M L
// numbers per unit, cannot overflow.  A launch takes as many super-blocks as
// the grid's caps cover (plan_sib_launch).
//
// Production takes it for a field that overlaps another (pipelined submits)
// with at least k.sib_pers_min / 10 batches per resident wave.  In rounds a
// workgroup's eight waves finish far apart -- the b40 1e9 field's wave 0 waits
// 21 % of its workgroup's life at the end-of-walk barrier -- and the CU's
// slot refills only when the last is done; on the persistent grid a wave that
// finishes a batch starts the next.  Pipelined, b40 at the range start,
// rounds -> persistent per step: 1e9 (8.9 batches per resident wave) 1.865 ->
// 1.818 ms, 5e8 (4.4) 0.930 -> 0.915, 2.5e8 (2.2) 0.4712 -> 0.4709, so the
// threshold sits at 4.  A lone field loses: nothing fills the CUs while the
// one round of workgroups drains its last batches (1e9 kernel 1.882 -> 1.970
// ms, 5e8 0.950 -> 0.967), so it keeps rounds and its whole-rounds stride.
// Grids of 2 and 4 rounds of shorter-lived workgroups, which would let the
// niceonly stream's launches in sooner, measured slower than one (bench step
// 1.835 / 1.868 / 1.883 ms at k = 1 / 2 / 4 against 1.879 in rounds;
// profiles/sib_persistent/).
template <class P>
static void plan_sib_pers(SibShape &sh, u64 count, int num_cus, int per_cu, bool overlapped,
                          const PlanKnobs<P> &k = PlanKnobs<P>{}) {
    constexpr u64 SB = (u64)P::SIB * P::B * P::B, NW = P::WG / 64;
    sh.pers = false;
    sh.pers_grid = 0;
    sh.wave_cap = 0;
    if (sh.kind != SibShape::kSib || k.sib_pers_mode == 2) return;
    const u64 resident = (u64)num_cus * per_cu, Q = count / SB;
    const u64 nb = (Q * sh.upb + 63) / 64 + (sh.has_edge ? (Q + 63) / 64 : 0);
    if (k.sib_pers_mode != 1 && (!overlapped || 10 * nb < k.sib_pers_min * resident * NW)) return;
    u64 G = resident * std::max<u64>(1, k.sib_pers_k);
    if (k.sib_pers_mode == 1 && k.sib_pers_max_wg) G = std::min<u64>(G, k.sib_pers_max_wg);
    const u64 cap = 65535 / ((u64)P::SIB * sh.L);
    // not even one super-block's batches under the grid's caps: rounds
    if (cap < 1 || (sh.upb + 63) / 64 + 1 > G * NW * cap) return;
    sh.pers = true;
    sh.pers_grid = G;
    sh.wave_cap = (u32)cap;
}

template <class P>
static SibLaunchPlan plan_sib_launch(u64 left, const SibShape &sh, int num_cus, int per_cu,
                                     const PlanKnobs<P> &k = PlanKnobs<P>{}) {
    constexpr u64 SB = (u64)P::SIB * P::B * P::B, LMAX = (u64)P::LDE - P::B, NW = P::WG / 64;
    const u64 lanes = (u64)num_cus * per_cu * P::WG;
    SibLaunchPlan pl{};
    pl.Q = left / SB;
    pl.cnt = left;
    u64 qmax = sh.qmax;
    if (sh.pers) {
        // Q super-blocks are at most Q (upb + 1) / 64 + 2 batches; workgroup g
        // takes every pers_grid-th, so the launch fits while its batches are at
        // most pers_grid NW wave_cap.  (64 b + lane stays in 32 bits.)
        const u64 room = sh.pers_grid * NW * sh.wave_cap;
        const u64 per = sh.upb + (sh.has_edge ? 1 : 0);
        qmax = std::min<u64>(qmax, std::max<u64>(1, room > 2 ? (room - 2) * 64 / per : 0));
        qmax = std::min<u64>(qmax, std::max<u64>(1, 0xffffffc0ull / sh.upb));
    }
    if (pl.Q > qmax) {
        pl.Q = qmax;
        pl.cnt = pl.Q * SB;
    }
    pl.R = pl.cnt - pl.Q * SB;
    pl.chunk = 1;
    if (pl.R) {
        pl.chunk = rounds_chunk(pl.R, lanes, k.tchunk, 4, true, LMAX);
        pl.nunits = pl.R / pl.chunk;
        pl.tail = pl.R - pl.nunits * pl.chunk;
    }
    pl.sib_units = pl.Q * sh.upb;
    pl.sib_blocks = (pl.sib_units + P::WG - 1) / P::WG;
    pl.edge_units = sh.has_edge ? pl.Q : 0;
    pl.edge_blocks = (pl.edge_units + P::WG - 1) / P::WG;
    if (sh.pers) {
        pl.batches = (pl.sib_units + 63) / 64 + (pl.edge_units + 63) / 64;
        pl.sib_blocks = std::min<u64>(sh.pers_grid, (pl.batches + NW - 1) / NW);
        pl.edge_blocks = 0;
        pl.wave_cap = sh.wave_cap;
    }
    pl.main_blocks = (pl.nunits + P::WG - 1) / P::WG;
    pl.grid = pl.sib_blocks + pl.edge_blocks + pl.main_blocks + (pl.tail + P::WG - 1) / P::WG;
    return pl;
}

}  // namespace fd2
}  // namespace nice
