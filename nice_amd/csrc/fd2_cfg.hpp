// fd2_cfg.hpp -- the FD detailed kernel's compile-time rules: the per-base
// histogram windows, the VD flags (namespace vd), the LDS layout and occupancy
// model, Cfg -- the configuration every fd2 kernel, launcher and launch plan
// is templated on -- and which Cfg production runs (SmallCfg, BigCfg, BatchCfg).
// Plain constexpr C++ (no GPU runtime header): fd2_kernel.hpp holds the device
// code, fd2_plan.hpp the launch planning, fd2_launch.hpp the launchers.
#pragma once

#include <algorithm>
#include <type_traits>

#include "layout.h"

namespace nice {
namespace fd2 {

constexpr int log2ceil(unsigned v) { int t = 0; while ((1u << t) < v) t++; return t; }
constexpr int ilog2(unsigned v) { int t = 0; while ((2u << t) <= v) t++; return t; }
constexpr int mask_words(int base) { return (base + 31) / 32; }  // 32-bit words of a digit mask

// Exactness of the digit split q = mulhi(ES v, m) = v / b over v < b^2.
constexpr bool split_exact(unsigned base, unsigned es, unsigned long long m) {
    for (unsigned v = 0; v < base * base; v++)
        if (((unsigned long long)es * v * m) >> 32 != v / base) return false;
    return true;
}

// Tuning / bottleneck-probe knobs read from the environment exist only in
// the probe build (make -C nice_amd probe -> libnice_hip_probe.so, used by
// scripts/); the product library ignores the environment and always runs the
// production configuration.

// Histogram window [W0, W0 + W) per base: where the unique-count
// distribution of in-range n lives (scripts/fd2_windows.py, 40 000 samples
// per base: at most 6e-4 of n fall outside; b40/50/80 keep their measured
// production windows).  W0 + W <= cutoff + 1: every near-miss is outside.
constexpr int window_w(int b) {
    return b == 40 ? 15 : b == 50 ? 18 : b == 80 ? 28 : b <= 45 ? 15 : b <= 61 ? 18 : b <= 70 ? 20 : 28;
}
constexpr int window_w0(int b) {
    switch (b) {
    case 40: return 18;
    case 42: return 19;
    case 43: return 20;
    case 44: case 45: case 47: return 21;
    case 48: return 22;
    case 49: return 23;
    case 50: return 21;
    case 52: return 24;
    case 53: return 25;
    case 54: case 55: return 26;
    case 57: return 27;
    case 58: return 28;
    case 59: case 60: return 29;
    case 62: case 63: return 30;
    case 64: return 31;
    case 65: return 32;
    case 67: return 33;
    case 68: return 34;
    case 80: return 33;
    default: return b * 61 / 100 - window_w(b) / 2;
    }
}

// Digit counts of n^2, n^3 and n inside a base's valid range
// (base_range.rs:14-32).
struct Digits {
    int d2, d3, dn;
};
constexpr Digits digits_of(int base) {
    const int k = base / 5, r5 = base % 5;
    return Digits{r5 == 0 ? 2 * k : (r5 == 4 ? 2 * k + 2 : 2 * k + 1),
                  r5 == 0 ? 3 * k : (r5 == 2 ? 3 * k + 1 : 3 * k + 2), r5 == 0 ? k : k + 1};
}

// Target chunk (numbers per lane), see plan_regular: a lane's init costs a
// few steps, more for wider bases.
constexpr int tchunk_of(int base) { return base <= 45 ? 80 : (base <= 58 ? 160 : 240); }

// Waves per SIMD whose VGPR budget (512 / waves) holds a base's lane state
// without spilling in the step loop: the stepped and cached limbs of n^2, n^3,
// 2n+1, 3n+1 plus the mask words, R = NS + NC + 2 NX + 1 + MW registers, and
// about as many temporaries.  b40 (R = 31) just fits 64 VGPRs (8 waves);
// R = 35..38 (b42..50) needs ~80 (6 waves), R <= 46 (b52..60) ~96 (5),
// wider bases 128 (4).
constexpr int state_regs(int base) {
    const Digits d = digits_of(base);
    return (d.d2 + 1) / 2 + (d.d3 + 1) / 2 + 2 * ((d.dn + 1) / 2) + 1 + mask_words(base);
}
constexpr int state_waves(int base) {
    const int r = state_regs(base);
    return r <= 31 ? 8 : (r <= 38 ? 6 : (r <= 46 ? 5 : 4));
}

// In-range n fits 64 bits: BASE^DN <= 2^64 (DN digits).
constexpr bool fits64(unsigned base, int digits) {
    unsigned long long v = 1;
    for (int i = 0; i < digits; i++) {
        if (v > ~0ull / base) return false;
        v *= base;
    }
    return true;
}

// The bits of Cfg's VD_ template argument.  The values are part of every
// kernel's mangled name (tests/test_abi.py, scripts/isa/kernel_diff.py key on
// it) and of the probe scripts' NICE_FD2_VD / NICE_FD2_SIB knobs: they stay.
namespace vd {
// VALU-decoded limbs (no table lookup): the top k stepped C limbs and the top
// k stepped S limbs, k < 16.  Their two digits come from one multiply-high by
// MAGIC_D = ceil(2^32 / (ES b)) and set their bits with 64-bit shifts, trading
// VALU work (~6 ops at MW = 2, ~15 at MW = 3) for one data-random
// (bank-conflicting) LDS read.
constexpr int c(int k) { return k; }
constexpr int s(int k) { return 16 * k; }
constexpr int LIMBS = c(15) | s(15);
constexpr int count_c(int v) { return v % 16; }
constexpr int count_s(int v) { return v / 16 % 16; }
// (no low-digit table only): limb 0 of S and of C by VALU too -- n^2 mod B and
// n^3 mod B of a wave's lanes keep few residues mod 16, so their lookups pile
// onto few bank quads
constexpr int LIMB0 = 256;
// (three mask words, b65..68 / b80): the digit-pair masks split into X1,
// 8-byte entries of the digits 0..63 (ds_read_b64), and X2, 4-byte entries of
// the digits 64.. (ds_read_b32), each table at its own entry size, so both
// spread a lane group over all 64 banks: the stored limb (scaled by 8)
// addresses X1 directly and X2 after one shift.  Probe only: on the kernel's
// own b80 index pattern b64 + b32 costs 11.9 LDS cycles per wave-lookup
// against 11.45 for one b128 of a 16-byte entry (the scripts/ubench/lds_trace
// microbenchmark, profiles/r04/lds_trace.log), and the kernel is 7 % slower
// with it.
constexpr int SPLIT = 512;
// (b59..64: word 1 of the low-digit entry is all digit bits): the low-digit
// table with the carries and wrap flags in a side table of bytes (bit 0 the S
// carry, bits 1-3 the C carry, bit 6 / 7 the D1 / N3 wraps), read at rc = TK +
// n mod B + i; r8 then holds TL too (TL can pass the 16-bit immediate offset).
constexpr int SIDE = 1024;
// the VALU-decoded limbs sit just BELOW the top stepped limb instead of at
// it.  The top stepped limb only takes carries, so its value is nearly the
// same in every lane of a wave and its lookup is nearly a broadcast (4 LDS
// cycles on b80's index pattern), while the limbs below it cost 11-12
// (scripts/ubench/lds_trace_gen.py).
constexpr int BELOW = 2048;
// the VALU-decoded limbs are the LOWEST ones above the low-digit table's limb
// (LO + 1 ...): the most data-random indices, whose lookups bank-conflict the
// most (sibling lanes, which have VALU to spare)
constexpr int LOWEST = 4096;
// (small fields): no low-digit table, limb 0 stepped like the others (a
// 12.8 KB instead of a 38.4 KB table image at b40)
constexpr int NOLOW = 16384;
// (small fields): no table image at all -- every limb decoded by VALU, limb 0
// included -- so no per-workgroup table DMA (the table loads of a small
// field's hundreds of workgroups are fetched through the fabric: b40 1e6
// spends a median 1.5 us, b80 1e6 4.6 us, of each workgroup's life on its
// state and tables; profiles/r06/stamps_r06.log)
constexpr int NOTAB = 32768;
// (probe A/B): the round-5 init -- init_digits on the 128-bit n and u64
// columns -- also on the 512-thread kernels of the bases whose n passes 64
// bits; the persistent-grid probe configurations at 512 threads (PERS_ = 1)
// take it too, their init being the round-5 one
constexpr int OLDINIT = 65536;
// sibling lanes: the sibling parts on a persistent grid (Cfg::SIBPERS:
// workgroup g of G walks the strided 64-unit batches g, g + G, ... of the
// sibling and edge units, its waves pulling them from an LDS counter; the
// remainder's regular parts stay rounds of the same launch, so PERS -- the
// regular parts' grid -- stays off)
constexpr int SIBPERS = 131072;
// the step's carry adds and limb reductions on the f32 FMA pipe (fma_bits,
// fd2_kernel.hpp): exact while every operand and result is an integer in
// [0, 2^24] and no FMA operand has wrapped below zero.  In the step's order
// (c the carry, 0..4, travelling unscaled):
//   t1 = ES c + C        FMA; C a state limb, < DC + 4 ES (the top stepped
//                        limb before rare()), never negative
//   t  = 3 S + t1 + N3   integer (v_mad_u32_u24, the 3 an inline constant;
//                        N3's offset limbs wrap on purpose); the true sum
//                        is in [0, TMAX]: a C-limb sum is < 5B + 4
//   C  = t - c DC        FMA; c = t / DC, so the result is in [0, DC)
//   t  = ES c + (S + D1) FMA; S biased, so t in [ES BT, 2^(SH+1))
//   S  = t - c DC        FMA; c = [t >= 2^SH], and 2^SH >= DC = ES B
// (3.0 as a third VGPR constant, or or_valu's -BASE as a fourth, spilled.)
// The off state is the integer form (v_lshl_add_u32 / v_mad_i32_i24).
constexpr int FMA = 262144;
constexpr int ALL = LIMBS | LIMB0 | SPLIT | SIDE | BELOW | LOWEST | NOLOW | NOTAB | OLDINIT | SIBPERS | FMA;
}  // namespace vd

// Limbs decoded by VALU instead of a table lookup (vd::c / vd::s), per base
// where the lookups' bank conflicts outweigh the VALU work: the best of VD
// 0/1/2/3/17 on the 1e9 field at the range start (scripts/vd_sweep_all.py,
// profiles/r02/vd_sweep_all.log), kept where it gains over ~1 %; without a
// low-digit table also limb 0 (vd::LIMB0, profiles/r02/vd_sweep_low.log).
// b64: 6.31 -> 4.25 ms (its table index n^2 mod 4096 keeps few residues mod
// 32, so lookups pile onto few banks);
// b45 2.60 -> 2.41; b60 3.79 -> 3.41; b63 3.96 -> 3.70; b68 7.42 -> 6.87;
// b80 8.22 -> 7.46; b40 neutral (r01).  Re-swept on the persistent grid
// (profiles/r03/vd_sweep_persistent.log): b55 0 -> 1 (2.91 -> 2.87 ms), b58
// 1 -> 2 (3.08 -> 3.00); every other base within ~1 % of its choice.
constexpr int valu_limbs(int base) {
    switch (base) {
    case 43: case 44: case 45: case 48: case 50: case 54: case 55: return vd::c(1);
    case 53: case 58: case 65: return vd::c(2);
    case 67: case 68: case 80: return vd::LIMB0;
    // b59..64: the low-digit table with its carries in a side table (vd::SIDE,
    // Cfg::LSDX), then the best top limbs by VALU: b59 3.31 -> 3.01 ms,
    // b60 3.39 -> 3.18, b62 3.49 -> 3.35, b63 3.71 -> 3.59, b64 4.17 -> 4.13
    // (profiles/r03/lsdx_sweep.log)
    case 59: case 63: case 64: return vd::SIDE | vd::c(2);
    case 60: return vd::SIDE | vd::s(1) | vd::c(1);
    case 62: return vd::SIDE | vd::c(1);
    default: return 0;
    }
}
// The low-digit side-table bases: their tables leave room for one workgroup
// per CU, so they run 1024 threads at every field size (4 waves per SIMD
// instead of 2), small fields and batches included.
constexpr bool side_table_base(int base) { return (valu_limbs(base) & vd::SIDE) != 0; }

// Fields of >= 1e7 on the three-mask-word bases (b65..80, the persistent
// 1024-thread kernel): limb 0 by VALU and the VALU-decoded C limbs just BELOW
// the top stepped one (vd::BELOW, Cfg::VDB).  The top stepped limb only takes
// carries, so across a wave its lookup is nearly a broadcast (4 LDS cycles on
// b80's index pattern against 11-12 for the limbs below it,
// scripts/ubench/lds_trace_gen.py), and decoding it by VALU saved little;
// decoding the limbs below it saves full-price lookups.  How many: per limb
// layout (the segment's ND, NE), from interleaved A/B sweeps over 1e9 fields
// at several points of each range with the select-free decode of or_valu and
// the one-multiply C carry (profiles/r04/vd_below_top.log): three, four where
// b80's n^3 has 17 limbs.  Against the round-3 kernels: b80 1e9 6.84 -> 6.24
// ms at the range start, b65 5.97 -> 5.43, b67 5.94 -> 5.64, b68 6.48 -> 5.57.
// The two-word bases (co-bound by VALU and LDS) move their VALU-decoded
// limbs below the top where that measured faster at both points of the
// range: b50 -1.1 / -2.2 %, b53 -1.1 / -1.4, b60 -1.2 / -1.7 (same VALU work,
// cheaper lookups); elsewhere within +-1 % or mixed, unchanged.  b40 (no
// VALU-decoded limbs before) decodes one C limb below the top on its 8-limb
// n^3 layouts (the first ~45 % of the range, the extra-large benchmark field
// among them): 2.03 -> 1.98 ms at the range start, 2.74 -> 2.62 at 0.1, 2.22
// -> 2.17 at 0.3, and it beats one or two more decoded limbs at every point
// checked in 0.02..0.35; on the 9-limb layout it lost 0-2 % and stays as it
// was (profiles/r04/vd_b40.log).
constexpr int valu_limbs_big(int base, int nd, int ne) {
    if (base == 40) return ne == 8 ? vd::BELOW | vd::c(1) : 0;
    if (base == 50 || base == 53 || base == 60) return valu_limbs(base) | vd::BELOW;
    if (mask_words(base) != 3) return valu_limbs(base);
    if (base == 80 && ne == 17) return vd::LIMB0 | vd::BELOW | vd::c(4);
    return vd::LIMB0 | vd::BELOW | vd::c(3);
}

// The low-digit entry's word 1 has room for the carries and flags beside its
// digit bits [0, DB) (Cfg::LSD_W1; two mask words: 33 <= base, so DB >= 1).
constexpr bool lsd_w1_fits(int base) {
    const int db = base - 32;
    return mask_words(base) == 2 && db + (db > 20 ? 4 : 10) <= 30;
}

constexpr int kLdsBytes = 160 * 1024;  // a CU's LDS
constexpr int kHistQ = 2;              // window counters per dword (Cfg::HQ)
constexpr int kImm16 = 1 << 16;        // LDS immediate offsets are unsigned 16-bit
constexpr int pad16(int v) { return (v + 15) / 16 * 16; }

// The LDS layout of a kernel, for Cfg (whose members of the same names take
// these values) and for the host's occupancy model (lds_bytes), which asks
// before any Cfg is chosen.  sib, ncold: Cfg's SIB and NCOLD.
//
// Default: [window rows | out-of-window bins (OUTL) | tables].  The digit-pair
// table needs at least EBT below it: S limbs are stored biased by EBT and
// looked up at (TB - EBT) + S, an unsigned immediate offset (b65-68: EBT
// exceeds the histogram region, so the table starts later).  SPLIT: [OUTL |
// pad | X2 at T2 | X1 at TB | window rows]: S limbs (biased by EBT) are looked
// up at (TB - EBT) + S in X1 and at (T2 - EBT / 2) + S / 2 in X2, C limbs at
// TB + C and T2 + C / 2, all unsigned 16-bit immediate offsets.  Regions are
// padded to 16 bytes: the image is copied in with 16-byte accesses.
struct Layout {
    bool SPLIT, NOTAB, LSD_W1, LSDX;
    int ES, HIST_BYTES, T2, TB0, TB, TC0, TL, LDE, TK, TEND, HB, COLD_BYTES, LDS_BYTES;
};
constexpr Layout layout(int base, int wg, int flags, int sib, int ncold) {
    const int mw = mask_words(base), b2 = base * base, nbins = base + 1;
    Layout l{};
    l.SPLIT = mw == 3 && (flags & vd::SPLIT) != 0;
    l.NOTAB = (flags & vd::NOTAB) != 0;
    l.LSD_W1 = lsd_w1_fits(base) && (flags & (vd::NOLOW | vd::NOTAB)) == 0;
    l.LSDX = mw == 2 && !l.LSD_W1 && (flags & vd::SIDE) != 0;
    l.ES = mw == 1 ? 4 : (mw == 2 || l.SPLIT ? 8 : 16);  // table entry stride (bytes)
    const int ebt = l.ES * ((1 << log2ceil(b2)) - b2);   // Cfg::EBT
    l.HIST_BYTES = window_w(base) * (wg / kHistQ) * 4;   // the window rows
    l.T2 = l.SPLIT ? std::max(pad16(4 * nbins), pad16(ebt / 2)) : 0;
    l.TB0 = l.SPLIT ? pad16(l.T2 + 4 * b2) : pad16(l.HIST_BYTES + 4 * nbins);
    l.TB = l.NOTAB || l.TB0 >= ebt ? l.TB0 : pad16(ebt);
    l.TC0 = (l.SPLIT ? l.T2 : l.TB) / 16 * 16;       // the table image starts here (16-byte copy)
    l.TL = l.TB + (l.NOTAB ? 0 : pad16(b2 * l.ES));  // low-digit table (LDE entries)
    // Low-digit entries: a lane whose chunk starts at n reads n mod B + i, i <
    // chunk <= B, so 2B cover any chunk.  The sibling kernels of b46+ keep
    // B + 256 (their chunks are capped at 256, plan_sib): the table then
    // leaves room for two 512-thread workgroups per CU.
    l.LDE = sib > 1 && base >= 46 ? b2 + 256 : 2 * b2;
    l.TK = l.TL + (l.LSD_W1 || l.LSDX ? pad16(l.LDE * l.ES) : 0);  // LSDX: carry bytes
    l.TEND = l.SPLIT ? pad16(l.TB + b2 * l.ES) : l.TK + (l.LSDX ? pad16(2 * b2) : 0);
    l.HB = l.SPLIT ? l.TEND : 0;  // SPLIT: window rows
    l.COLD_BYTES = pad16(sib * ncold * wg * 2);
    l.LDS_BYTES = l.SPLIT ? l.HB + l.HIST_BYTES : l.TEND + l.COLD_BYTES;
    return l;
}

// LDS bytes of a base's regular kernel at a workgroup size.
constexpr int lds_bytes(int base, int wg) { return layout(base, wg, valu_limbs(base), 1, 0).LDS_BYTES; }
// Waves per SIMD the LDS allows: whole workgroups per CU, each putting its
// wg / 64 waves on the 4 SIMDs.
constexpr int lds_waves(int lds, int wg) { return (kLdsBytes / lds) * (wg / 64) / 4; }
// Waves per SIMD actually resident: the LDS and VGPR caps, in whole
// workgroups (a workgroup puts wg / 256 waves on each SIMD).
constexpr int waves_at(int base, int wg) {
    const int cap = std::min(lds_waves(lds_bytes(base, wg), wg), state_waves(base));
    return cap / (wg / 256) * (wg / 256);
}
// Workgroup size for fields >= 1e7 in rounds of workgroups: the kernels are
// bound by LDS lookups and want as many in flight as fit, so the size with
// more waves per SIMD under the LDS budget wins, 512 on a tie.  Measured on
// the first three bases: b40 two 1024-thread workgroups per CU (8 waves/SIMD)
// 2.38 ms vs 2.43 for three 512-thread ones (6 waves,
// profiles/r01/fd2_wg_sweep2.log); b80 one 1024-thread workgroup (4 waves)
// 8.47 ms vs 9.37 at 512 (2 waves, profiles/r01/b80_wg_sweep.log); b50 4
// waves either way, 512 kept.
constexpr int rounds_wg(int base) { return waves_at(base, 1024) > waves_at(base, 512) ? 1024 : 512; }
// With the persistent grid (Cfg::PERS) a tie goes to 1024: one 1024-thread
// workgroup per CU walking strided batches beats two 512-thread ones in
// rounds on every such base (b42..50 -3..-10 %, b59..64 -2..-5 % per 1e9,
// profiles/r03/pers_sweep_wg1024.log).
constexpr int big_wg(int base) { return waves_at(base, 1024) >= waves_at(base, 512) ? 1024 : 512; }

// Persistent grid by default where the kernel holds ONE workgroup per CU
// (b52..58, b65..68, b80 at 1024 threads): with two or more, a workgroup's
// draining tail overlaps another's steps, and rounds of workgroups win
// (profiles/r03/pers_sweep_all.log: b52..58 -12..-15 %, b65..68 / b80 -6..-10 %
// per 1e9; b42..50 and b59..64, two workgroups per CU, +1..+6 %).
constexpr bool one_wg_per_cu(int base, int wg) { return waves_at(base, wg) == wg / 256; }

// Sibling lanes (Cfg::SIB = M > 1): registers per wave for M lanes' state
// (the shared limb-1 state once, the upper limbs of every sibling).
constexpr int sib_waves(int base, int m) { return m <= 1 ? state_waves(base) : (m <= 3 ? 6 : 5); }

// init's products in u64 columns: the 1024-thread kernels of the bases whose
// n passes 64 bits (the register allocation that spills least), and the
// kernels with the round-5 init (`wide`: vd::OLDINIT, or a forced persistent
// grid).  Elsewhere u32 columns (every FD base's column sums fit 32 bits:
// static_assert in Cfg), normalised by 32-bit multiply-highs.  The u32 kernels
// of the bases whose n passes 64 bits read n's radix-b^2 digits from the host
// (Fd2Args::xs, a descriptor's xs): this rule, for Cfg and the host alike.
constexpr bool reads_host_digits(int base, int wg, bool wide = false) {
    return !fits64(base, digits_of(base).dn) && wg < 1024 && !wide;
}

template <int BASE_, int ND_, int NE_, int NE2_, int PROBE_ = 0, int WG_ = 512, int VD_ = 0, int LG_ = -1,
          int PERS_ = -1, int SIB_ = 1>
struct Cfg;
// The regular (no sibling lanes) kernel of fields >= 1e7.
template <int B_, int ND_, int NE_, int NE2_, int PROBE_ = 0>
using RegularBig = Cfg<B_, ND_, NE_, NE2_, PROBE_, big_wg(B_), valu_limbs_big(B_, ND_, NE_)>;

template <int BASE_, int ND_, int NE_, int NE2_, int PROBE_, int WG_, int VD_, int LG_, int PERS_, int SIB_>
struct Cfg {
    static constexpr int BASE = BASE_;
    // Bottleneck probes (timing experiments only, results are wrong): 1 = no
    // table lookups (limb words OR-ed directly), 2 = no LDS histogram add,
    // 4 = no limb-1 lookups of S and C.
    static constexpr int PROBE = PROBE_;
    static constexpr int ND = ND_, NE = NE_, NE2 = NE2_;
    // Digit counts inside the valid range.
    static constexpr int D2 = digits_of(BASE).d2, D3 = digits_of(BASE).d3, DN = digits_of(BASE).dn;
    static constexpr bool N64 = fits64(BASE, DN);  // init's u64 path
    static constexpr bool OLDINIT = (VD_ & vd::OLDINIT) != 0;
    // init's products in u64 columns (reads_host_digits)
    static constexpr bool C64 = !N64 && !reads_host_digits(BASE, WG_, OLDINIT || PERS_ > 0);
    static constexpr int NS = cdiv(D2, 2), NC = cdiv(D3, 2), NX = cdiv(DN, 2);
    static constexpr int SL = ND + 1, CL = NE + 1, EL = NE2 + 1;  // per-step limbs
    static constexpr int S_TOPD = D2 - 2 * (NS - 1), C_TOPD = D3 - 2 * (NC - 1);
    static constexpr u32 B = (u32)BASE * BASE;
    static constexpr int T = log2ceil(B);
    static constexpr u32 BT = (1u << T) - B;
    static constexpr int MW = mask_words(BASE);
    static constexpr int SIB = SIB_;
    // Sibling lanes (see below): each sibling's cached C limbs [CL, NC) -- read and
    // written only on the rare path -- as u16 per thread in LDS instead of
    // VGPRs (slot (j, k) of thread t at COLD + 2 ((j NCOLD + k) WG + t)).
    static constexpr int NCOLD = SIB_ > 1 ? NC - CL : 0;
    // The LDS layout (layout(), above) in plain members: device code names
    // those, never the LAYOUT object.
    static constexpr Layout LAYOUT = layout(BASE_, WG_, VD_, SIB_, NCOLD);
    static constexpr bool SPLIT = LAYOUT.SPLIT, NOTAB = LAYOUT.NOTAB, LSD_W1 = LAYOUT.LSD_W1, LSDX = LAYOUT.LSDX;
    static constexpr int ES = LAYOUT.ES, HIST_BYTES = LAYOUT.HIST_BYTES, T2 = LAYOUT.T2, TB0 = LAYOUT.TB0;
    static constexpr int TB = LAYOUT.TB, TC0 = LAYOUT.TC0, TL = LAYOUT.TL, LDE = LAYOUT.LDE, TK = LAYOUT.TK;
    static constexpr int TEND = LAYOUT.TEND, HB = LAYOUT.HB, COLD_BYTES = LAYOUT.COLD_BYTES, LDS_BYTES = LAYOUT.LDS_BYTES;
    static constexpr int SH = T + ilog2(ES);  // carry bit of a scaled limb
    static constexpr u32 ESB = ES * B, EBT = ES * BT;
    static constexpr int WG = WG_;
    static constexpr int TCHUNK = tchunk_of(BASE);
    static constexpr int NBINS = BASE + 1;
    // Histogram window [W0, W0 + W): per-thread counters (u32, or u16 halves
    // shared by threads t and t + WG/2 when LDS is tight).
    static constexpr int W = window_w(BASE);
    static constexpr int W0 = window_w0(BASE);
    // Window counters: HQ per dword (u16 halves shared by threads t and
    // t + WG/2).
    static constexpr int HQ = kHistQ;
    static constexpr int HROW = WG / HQ;  // counters per window row
    // (A branch-free window count -- every count to row min(uw, W), a dummy
    // row W, out-of-window counts recorded behind one wave-uniform branch --
    // measured 1 % slower on the b40 sibling kernel; skipping the
    // out-of-window work altogether, wrong by design, only 3 % faster:
    // profiles/r06/occupancy_ab.txt, bfw_uniform_branch_ab.log.)
    static constexpr int OUTL = SPLIT ? 0 : HIST_BYTES;  // per-workgroup histogram of out-of-window counts
    // Low-digit entry, word 1: digit bits [0, DB), then the carries and flags
    // of the step n -> n+1, all functions of n mod B (limb 0 of S, C, D1, N3
    // is never stored): the carry out of S limb 0 of S += D1 and the carry
    // (0..4) out of C limb 0 of C += 3S + N3; bit 30: D1 limb-0 wrap, bit 31:
    // N3 limb-0 wrap (top bits, so "any flag" is one compare).  Up to b52 the
    // carries sit pre-scaled by ES = 8 (a 4-bit field at F0 holding 8 * carry,
    // a 6-bit field at FC holding 8 * carry: one v_bfe each gives the scaled
    // carry); b53..58 leave room only for the bare carries (1 + 3 bits, one
    // extra multiply-add per step); wider bases have no low-digit table, or
    // keep the carries in a side table (vd::SIDE).
    static constexpr int DB = BASE - 32;
    static constexpr bool TIGHT = DB > 20;
    static constexpr bool LSD = LSD_W1 || LSDX;
    static constexpr int COLD = TEND;
    static constexpr int TAB_BYTES = TEND - TC0;  // table image copied in per workgroup
    static constexpr int ZA = SPLIT ? TC0 : TB;   // zeroed per workgroup: [0, ZA) and [HB, LDS_BYTES)
    static constexpr int LO = LSD ? 1 : 0;  // first stored / looked-up limb
    static constexpr u32 DMASK = (1u << (DB > 0 && DB < 32 ? DB : 0)) - 1;
    static constexpr u32 FLAG_D1 = LSDX ? 1u << 6 : 1u << 30, FLAG_N3 = LSDX ? 1u << 7 : 1u << 31;  // any flag: w1 >= FLAG_D1
    static constexpr int F0 = LSDX ? 0 : TIGHT ? DB : (DB + 3) / 4 * 4;
    static constexpr int FC = LSDX ? 1 : TIGHT ? DB + 1 : F0 + 4;
    static constexpr int F0W = TIGHT ? 1 : 4, FCW = TIGHT ? 3 : 6;  // field widths
    // C += 3S + N3 (N3 = 3n + 1, NN limbs).  A C limb sum is < 5B, so its
    // carry (0..4) is a multiply-high by MAGIC = ceil(2^32 / (ES B)) (exact
    // over the range: static_assert).
    static constexpr int NN = NX + 1;
    static constexpr u32 DC = ES * B;
    static constexpr u32 MAGIC = (u32)(((1ull << 32) + DC - 1) / DC);
    static constexpr unsigned long long TMAX = (unsigned long long)ES * (5ull * B + 4);
    // One multiply-high by MAGIC is exact because t is a multiple of ES:
    // with t = ES u, u = qB + r and ES B MAGIC = 2^32 + e, the product is
    // q + r / B + u e / (B 2^32), whose floor is q while u e < 2^32 (b80:
    // u <= 5B + 4 = 32004, e = 98304).  Where even that fails, divide t / ES
    // first.  (Rounds 1-3 bounded t e < 2^32 instead, which sent the
    // 16-byte-entry bases b65..80 down the extra shift per C limb.)
    static constexpr bool C1 = ((unsigned long long)MAGIC * DC - (1ull << 32)) * (TMAX / ES) < (1ull << 32);
    static constexpr u32 MAGICB = (u32)(((1ull << 32) + B - 1) / B);
    // VALU-decoded limbs: the flags of namespace vd.
    static constexpr int VD = VD_;
    static constexpr int VDC = vd::count_c(VD), VDS = vd::count_s(VD);
    static constexpr int VDB = (VD & vd::BELOW) ? 1 : 0;
    static constexpr bool VDLOW = (VD & vd::LOWEST) != 0;
    static constexpr bool vd_s(int q) {
        if (NOTAB) return true;
        return VDLOW ? (q > LO && q <= LO + VDS && q < SL) : (q >= SL - VDB - VDS && q < SL - VDB);
    }
    static constexpr bool vd_c(int q) {
        if (NOTAB) return true;
        return VDLOW ? (q > LO && q <= LO + VDC && q < CL) : (q >= CL - VDB - VDC && q < CL - VDB);
    }
    // Lookup groups: a scheduling barrier after every LG table lookups of a
    // step (0: none), so the compiler cannot hoist all of a step's LDS reads
    // ahead of their ORs -- with SPLIT's b64 + u16 pairs that held ~75 VGPRs
    // of loaded words at once and spilled the 1024-thread b80 kernel at its
    // 128-VGPR budget; the 16-byte layout spilled 52-64 bytes per lane there
    // too, and LG 8 removes it (b80 1e9 7.45 -> 7.31 ms, lg_sweep.log).
    // -1: the per-base default.
    // (sibling lanes: LG >= 100 -- the default -- pipelines the siblings'
    // lookups with the arithmetic, walk_sib_pipe; below 100 LG != 0 ends a
    // group after each sibling's lookups, LG > 1 after every LG of them too)
    static constexpr int LG = LG_ >= 0 ? LG_ : (SIB_ > 1 ? 100 : (MW == 3 && WG >= 1024 ? 8 : 0));
    // Persistent grid: one round of resident workgroups, each walking a
    // contiguous range of 64-unit batches that its waves pull from an LDS
    // counter as they finish (instead of one chunk per lane and many rounds
    // of workgroups, where a workgroup's CU idles down while its slowest
    // wave finishes: b54 1e9, one 1024-thread workgroup per CU, waited 61 us
    // of a 134 us workgroup life for it, profiles/r03/fd2_stamps_b54.log).
    // -1: the per-base default.
    // Sibling lanes: M = SIB numbers n0 + j B^2 per lane, in lock step.  n and
    // n + j B^2 agree mod B^2, so limbs 0 and 1 of n^2, n^3, 2n + 1 and 3n + 1
    // (radix B) are the same for all of them and so is the carry out of limb
    // 1 of every chain: the low-digit lookup, limb 1's two lookups and limb 1's
    // carry chains run once for the M numbers (walk_sib).  Rounds, or with
    // vd::SIBPERS the sibling parts on a persistent grid.
    static constexpr bool SIBPERS = SIB_ > 1 && (VD_ & vd::SIBPERS) != 0;
    static constexpr bool PERS = SIB_ > 1 ? false : PERS_ >= 0 ? PERS_ != 0 : (WG >= 1024 && one_wg_per_cu(BASE, WG));
    // the persistent twin of a sibling rounds kernel, where one is built: the
    // b40 pipelined walk on the ND = 4 layouts (plan_sib_pers decides per
    // segment whether it runs)
    using SibPers = Cfg<BASE_, ND_, NE_, NE2_, PROBE_, WG_, VD_ | vd::SIBPERS, LG_, PERS_, SIB_>;
    static constexpr bool HAS_SIBPERS =
        SIB_ > 1 && (VD_ & vd::SIBPERS) == 0 && PROBE_ == 0 && BASE_ == 40 && ND_ == 4 && LG >= 100;
    // the same kernel with rounds of workgroups (launch_cfg falls back to it
    // when the runtime occupancy or the field size does not suit PERS), at
    // the workgroup size rounds prefer
    using NoPers = Cfg<BASE_, ND_, NE_, NE2_, PROBE_, (PERS_ < 0 ? rounds_wg(BASE_) : WG_), VD_, LG_, 0>;
    // the production kernel without sibling lanes (segments shorter than a
    // few M B^2): the big-field workgroup size and VALU-decoded limbs; b46+
    // keep the persistent-grid default of their regular kernel (b52..55 1e8
    // fields: rounds of workgroups +8..+10 %, profiles/r05/sib_short_table_ab.log)
    using NoSib = std::conditional_t<(BASE_ >= 46), RegularBig<BASE_, ND_, NE_, NE2_, PROBE_>,
                                     Cfg<BASE_, ND_, NE_, NE2_, PROBE_, rounds_wg(BASE_), valu_limbs_big(BASE_, ND_, NE_), -1, 0>>;
    // lookup groups of walk_chunk (the sibling kernel's regular parts: none)
    static constexpr int LGW = SIB_ > 1 ? 0 : (LG_ >= 0 ? LG_ : (MW == 3 && WG_ >= 1024 ? 8 : 0));
    static constexpr bool VDL = ((VD & vd::LIMB0) != 0 || NOTAB) && !LSD;
    static constexpr u32 MAGIC_D = (u32)(((1ull << 32) + ES * BASE - 1) / (ES * BASE));
    // vd::FMA: the operand bounds of the f32-pipe limb arithmetic
    static constexpr bool FMA = (VD_ & vd::FMA) != 0;
    static constexpr unsigned long long FMA_LIM = 1ull << 24;
    static constexpr unsigned long long FMA_T1 = 4ull * ES + DC + 4ull * ES;  // max ES c + C
    static constexpr unsigned long long FMA_TS = 2ull << SH;                  // S-limb sum bound
    static_assert(!FMA || (TMAX <= FMA_LIM && FMA_T1 <= FMA_LIM && 5ull * DC <= FMA_LIM && FMA_TS <= FMA_LIM),
                  "f32-pipe limb arithmetic: operands and results within 2^24");
    // the reductions' results are non-negative: C's carry is t / DC (exact:
    // the carry-magic assert below), S's is one DC taken off t >= 2^SH >= DC
    static_assert(!FMA || (TMAX / DC <= 5 && (1ull << SH) >= DC),
                  "f32-pipe limb arithmetic: no reduction below zero");
    static_assert(VD == 0 || (MW >= 2 && split_exact(BASE, ES, MAGIC_D)), "VALU digit split");
    static_assert(VDC <= NE + 1 - (MW <= 2 ? 1 : 0) && VDS <= ND + 1 && (VD & ~vd::ALL) == 0 &&
                      ((VD & vd::SIDE) == 0 || LSDX),
                  "VALU-decoded limbs");
    // Waves per SIMD: what the LDS allows, capped by what the lane state
    // needs in VGPRs (the register budget is set to match, see state_waves).
    static constexpr int WPE0 = lds_waves(LDS_BYTES, WG);
    // (the small-field variants -- no low-digit table / no table -- at a
    // 128-VGPR budget: a field below 1e7 puts only a few waves on each SIMD)
    // (three mask words without a table: 256 VGPRs)
    static constexpr int WREG = NOTAB && MW == 3 ? 2 : (VD_ & (vd::NOLOW | vd::NOTAB)) ? 4 : sib_waves(BASE, SIB);
    static constexpr int WPE1 = WPE0 < WREG ? WPE0 : WREG;
    // in whole workgroups: k = the workgroups a CU holds at WPE1 waves per
    // SIMD (a workgroup's WG / 64 waves spread over the 4 SIMDs), then the
    // waves per SIMD those k workgroups need (640-thread workgroups: 2.5 each)
    static constexpr int WGK = WPE1 * 256 / WG;
    static constexpr int WPE = WGK > 0 ? (WGK * (WG / 64) + 3) / 4 : (WG / 64 + 3) / 4;
    static_assert(WPE >= 1, "LDS: not even one workgroup fits");
    static_assert(SL < NS && CL < NC && EL <= NE, "FD layout needs cached high limbs");
    static_assert(ND <= NX + 1 && NE2 <= NX + 1 && NE <= NS + 1, "difference limb counts");
    static_assert(S_TOPD >= 1 && C_TOPD >= 1, "top limb");
    static_assert((NOTAB || TB >= (int)EBT) && (NOTAB || TB - (int)EBT < kImm16) && (!LSD || LSDX || TL < kImm16),
                  "LDS offsets");
    static_assert(!NOTAB || (!LSD && !SPLIT && SIB_ == 1), "table-free kernel: regular lanes, no low-digit table");
    static_assert(!PERS || N64 || C64, "persistent grid: init() only (init_at is the rounds path's)");
    static_assert(!SPLIT || (T2 >= (int)EBT / 2 && T2 < kImm16 && T2 + 4 * (int)B <= TB && 4 * NBINS <= TC0 &&
                             ES == 8 && TB < kImm16),
                  "split layout");
    static_assert(LDS_BYTES <= kLdsBytes, "LDS");
    static_assert(TB % 16 == 0 && TAB_BYTES % 16 == 0 && HB % 16 == 0, "16-byte table copy");
    static_assert(W0 >= 0 && W0 + W <= NBINS, "window");
    static_assert(!LSD || (ES == 8 && (LSDX ? TIGHT && FC + FCW <= 6 : FC + FCW <= 30)), "low-digit entry layout");
    static_assert(C1 || ((unsigned long long)MAGICB * B - (1ull << 32)) * (TMAX / ES) < (1ull << 32),
                  "C-limb carry magic");
    static_assert(NN <= SL && NE >= NS, "C += 3S + N3 layout");
    static_assert(3 * ES <= 64, "inline-constant multiplier");
    static_assert(SIB == 1 || (LSD && MW == 2 && LO == 1 && SL >= 3 && CL >= 3 && ND >= 2 && NN >= 2),
                  "sibling lanes share limb 1: low-digit-table bases only");
    static_assert((unsigned long long)NX * B * B + 2ull * B < (1ull << 32), "32-bit init columns");
};

// What production runs for a (base, combo) is said here alone: the per-base
// launchers dispatch to SmallCfg / BigCfg / BatchCfg, the host code asks
// small_wg and reads_host_digits, tests/ and scripts/ubench take the aliases.

// Fields too small to fill the chip (< 1e7 numbers) and the batch kernels: 512
// threads (the per-workgroup table build dominates there: b80 1e6 kernel 30
// vs 38 us) and the base's valu_limbs, except on the side-table bases.
constexpr int small_wg(int base) { return side_table_base(base) ? big_wg(base) : 512; }
constexpr int small_vd(int base, int nd, int ne) {
    return side_table_base(base) ? valu_limbs_big(base, nd, ne) : valu_limbs(base);
}
template <int B_, int ND_, int NE_, int NE2_>
using SmallCfg = Cfg<B_, ND_, NE_, NE2_, 0, small_wg(B_), small_vd(B_, ND_, NE_)>;

// The batch kernel's configuration: SmallCfg's, with rounds of workgroups.
// LG_ and PERS_ are spelled out at the values those kernels default to (two
// mask words or 512 threads: no lookup groups), which makes the type -- and
// with it every device function instantiated for it -- the batch kernel's own:
// sharing the instantiations with fd2_kernel<P> of the same P moved that
// kernel's register allocation by a VGPR or two
// (profiles/ranges/build_and_resources.txt).
template <int B_, int ND_, int NE_, int NE2_>
using BatchCfg = Cfg<B_, ND_, NE_, NE2_, 0, small_wg(B_), small_vd(B_, ND_, NE_), 0, 0>;

// Fields of >= 1e7 numbers: sibling lanes (Cfg::SIB, fd2_kernel.hpp) on the
// bases up to b55, 512 threads; elsewhere the regular kernel at valu_limbs_big.
// plan_sib falls back to the regular kernel (Cfg::NoSib) below ~1.5 rounds of
// sibling units.
// b40..45: three lanes.  b42..45, 1e9 at the range start and half-way: b42 -11
// / -8 %, b43 -12 / -14, b44 -10 / -11, b45 -6 / -3 against their regular
// kernels (profiles/r05/sib_bases_ab.log).
// b47..55: two lanes over the short low-digit table (Layout::LDE, two
// 512-thread workgroups per CU; with the full 2B table and three lanes they
// held one and lost +1..+25 %): 1e9 at the range start and half-way -2..-9 %,
// b50 / b53 half-way -2 / -0.6 % (profiles/r05/sib_short_table_ab.log)
constexpr int sib_lanes(int base) { return base >= 40 && base <= 45 ? 3 : (base >= 47 && base <= 55 ? 2 : 1); }
// b40 on its first limb layout (ND = 4: the range's first ~29 %, the benchmark
// fields): pipelined (LG 100), with the lowest C limb above the shared one
// decoded by VALU; elsewhere per-sibling lookup groups (LG 1), no VALU decode
// (profiles/r05/sib_sweep_range.log).  The pipelined one has a persistent-grid
// twin (Cfg::SibPers), which launch_sib picks for long pipelined segments
// (plan_sib_pers).
// All of b40's with the limb chains' carry adds and reductions on the f32 FMA
// pipe (vd::FMA): interleaved against the integer form on 1e9 fields,
// 1.74-1.76 vs 1.84-1.85 ms at the range start, 1.75 vs 1.89 at 0.1, 1.85 vs
// 1.95 at 0.25 (pipelined), 1.91 vs 2.00 at 0.35 and 1.94 vs 2.02 at 0.5
// (profiles/fma/sib_fma_ab.txt).  The other bases keep the integer form; their
// A/B: profiles/fma/bases_fma_ab.txt.
constexpr bool sib_pipelined(int base, int nd) { return base == 40 && nd == 4; }
constexpr int sib_vd(int base, int nd) {
    return (sib_pipelined(base, nd) ? vd::LOWEST | vd::c(1) : 0) | (base == 40 ? vd::FMA : 0);
}
template <int B_, int ND_, int NE_, int NE2_>
using BigCfg = std::conditional_t<(sib_lanes(B_) > 1),
                                  Cfg<B_, ND_, NE_, NE2_, 0, 512, sib_vd(B_, ND_), (sib_pipelined(B_, ND_) ? 100 : 1), 0, sib_lanes(B_)>,
                                  RegularBig<B_, ND_, NE_, NE2_>>;

}  // namespace fd2
}  // namespace nice
