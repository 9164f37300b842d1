// fd2_kernel.hpp -- production finite-difference detailed kernel (gfx950):
// the device code.  Its compile-time configuration is fd2_cfg.hpp, the
// launch planning fd2_plan.hpp, the per-instantiation launchers
// fd2_launch.hpp.  Instantiated per base by fd2_part*.hip (compiled in
// parallel), driven by fd2_detailed.hip.
//
// Computes exactly what process_range_detailed does (common/src/
// client_process.rs:150-191: per n the unique-digit count of n^2 and n^3 in
// base b, histogrammed, plus the near-miss list) for segments inside a base's
// valid range, where n^2 and n^3 have fixed digit counts D2 + D3 = b.  It
// replaces the reference's detailed_kernel (common/src/cuda/nice_kernels.cu:
// 486-531); the design is MI355X-first, not a translation:
//
//  * Each lane walks a contiguous chunk n0 .. n0+len-1 (len <= B = b^2).
//    n^2 and n^3 live in radix-B limbs (one limb = two base-b digits) and step
//    by finite differences, never dividing:
//        S = n^2 += D1,            D1 = 2n + 1 += 2
//        C = n^3 += 3 S + N3,      N3 = 3n + 1 += 3
//    (the cube's increment 3n^2 + 3n + 1 is rebuilt from the square's limbs,
//    so no second-order difference state is carried).  A C-limb sum is < 5B:
//    its carry (0..4) is one multiply-high (two for b80).
//  * Limb counts are template parameters picked by the host per segment
//    (ND, NE = limbs of D1 = 2e+1 and E1 = 3e^2+3e+1 at the segment's end,
//    NE2 of 6e+6 kept for the layout checks), so a step touches exactly the
//    limbs that can change: S limbs [0, ND], C limbs [0, NE].  Carries out of
//    those (probability ~1/B per step) and the limb-0 wraps of D1 / N3 take a
//    rare, wave-uniform branch.
//  * The per-step limbs are stored SCALED by the mask-table entry size ES and
//    BIASED by 2^T - B: the stored word is directly the LDS byte address of the
//    limb's digit-pair mask (no address arithmetic), and the radix-B carry is
//    bit T + log2(ES) of the sum (one shift, one v_mad_i32_i24 to reduce).
//  * n^2 mod B and n^3 mod B depend only on n mod B, so limb 0 of S and of C
//    share ONE lookup in a low-digit table indexed by r = n0 mod B + i (< 2B:
//    the table has 2B entries, so r never wraps inside a chunk).
//  * Histogram: per-thread counters in LDS for a window of W unique counts
//    around the distribution's bulk (b40: 17..32 holds all but 7e-5 of n); the
//    rare counts outside the window (and every near-miss, which always lies
//    above the window) take a divergent branch to a per-workgroup LDS
//    histogram and the global near-miss list.  One flush per workgroup.
//
//  * Grid: rounds of workgroups, one chunk per lane, where two or more
//    workgroups share a CU (b40); one round of resident 1024-thread
//    workgroups whose waves pull strided 64-unit batches where one workgroup
//    fills a CU (Cfg::PERS, b42..80 fields of >= 2 rounds).  The b40 sibling
//    kernel's pipelined fields of >= 4 batches per resident wave run their
//    sibling parts on such a grid too (Cfg::SIBPERS, two 512-thread
//    workgroups per CU; fd2_plan.hpp plan_sib_pers).
//
//  * Cfg::FMA (b40's sibling kernels): the step's shift-adds and limb
//    reductions (C + ES c, t - c DC; 3 S + t keeps its integer multiply-add,
//    whose 3 is an inline constant: a third VGPR constant spilled) run on the f32 FMA
//    pipe on the limbs' bit patterns (fma_bits: a small integer's pattern is
//    a subnormal, and the FMA of such patterns is exact), the carries of both
//    chains travelling unscaled from limb to limb.  On gfx950 a v_fma_f32 of
//    VGPRs issues in ~2.6 cycles, the integer forms in ~4.4 (and anything
//    with an SGPR operand in ~4.3, hence the constants in VGPRs).  The
//    kernels must keep f32 subnormals (the compiler's default mode).
//
// The kernel is issue-bound on VALU and LDS together: b40 per n is 13 random
// 8-byte LDS lookups (≈5 LDS cycles each per wave) and ≈78 VALU instructions
// per wave-step; see DESIGN.md §3.1 for the cycle model and the measured
// roofline.
#pragma once
#include "fd2_cfg.hpp"
#include "kernels.h"
#include "nice_device.hpp"
#include "probe.hpp"

namespace nice {
namespace fd2 {
// v_mad_u32_u24 with an inline-constant multiplier (LLVM otherwise splits it
// into v_mul_u32_u24 + v_add3_u32).
template <u32 K>
__device__ __forceinline__ u32 mad_u24(u32 a, u32 c) {
    static_assert(K <= 64, "inline constant");
    u32 r;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "n"(K), "v"(c));
    return r;
}

// v_mad_i32_i24 with a scalar multiplier: a * K + c on 24-bit signed a, K
// (LLVM otherwise turns c - a * K into a v_mad_u64_u32, which does not issue
// at the full rate).
template <int K>
__device__ __forceinline__ u32 mad_i24s(u32 a, u32 c) {
    u32 r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(K), "v"(c));
    return r;
}

// a * K + c on the f32 FMA pipe, for integers: returns the bits of the integer
// a K + c (Cfg::FMA).  A u32 bit pattern x <= 2^24 read as an IEEE f32 is
// exactly x 2^-149 -- a subnormal below 2^23, and the first normal binade
// continues the same line -- so with a true float K the FMA of two such
// patterns is (a K + c) 2^-149: exact in every rounding mode, nothing being
// rounded, while a, c and a K + c are integers in [0, 2^24] (Cfg's
// static_asserts; the kernels keep f32 subnormals, the compiler's default,
// see the Makefile).  An integer that wrapped below zero is a NaN pattern
// here: such terms (N3's offset limbs, -3 ES BT) are added after the FMAs,
// as integers.  No conversion anywhere: the same register is still the limb's
// LDS byte offset and a multiply-high's operand.  K sits in a VGPR: on gfx950
// a v_fma_f32 of VGPRs (or an inline constant) issues in ~2.6 cycles against
// ~4.4 for the integer multiply-adds and shift-adds it replaces, but ANY
// instruction with an SGPR operand in ~4.3 (profiles/fma/isa_issue_rates.log).
template <int K>
__device__ __forceinline__ u32 fma_bits(u32 a, u32 c) {
    u32 r;
    const float k = (float)K;
    asm("v_fma_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(k), "v"(c));
    return r;
}

// v_bcnt_u32_b32 with a scalar accumulator: popcount(x) + acc.
__device__ __forceinline__ u32 bcnt_acc(u32 x, u32 acc) {
    u32 r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "s"(acc));
    return r;
}

template <class P>
struct State {
    u32 S[P::NS];    // n^2: limbs [0, SL) scaled+biased, [SL, NS) plain
    u32 C[P::NC];    // n^3: same with CL
    u32 D1[P::ND];   // scaled, plain
    u32 N3[P::NN];   // 3n + 1, scaled, limb i < SL offset by -3 ES BT
    u32 r8;          // low-digit table byte offset: ES * (n mod B + i) (LSDX: + TL)
    u32 rc;          // LSDX: carry byte address TK + n mod B + i
    u32 hi[P::MW];   // mask of the cached (rarely changing) limbs of S and C
};

template <class P>
__device__ __forceinline__ void or_entry(const unsigned char *p, u32 (&m)[P::MW]) {
    if constexpr (P::MW == 1) {
        m[0] |= *(const u32 *)p;
    } else if constexpr (P::MW == 2 || P::SPLIT) {
        uint2 v = *(const uint2 *)p;
        m[0] |= v.x;
        m[1] |= v.y;
    } else {
        uint4 v = *(const uint4 *)p;
        m[0] |= v.x;
        m[1] |= v.y;
        m[2] |= v.z;
        // Keep the 4th (zero) dword live so the load stays ds_read_b128: LLVM
        // would shrink it to ds_read_b96, which gfx950 serves in 8 lane groups
        // over 32 banks (8 cycles per wave) instead of 4 groups over 64 (4).
        asm volatile("" ::"v"(v.w));
    }
}

// OR the digit-pair mask of a stored limb into m: X1 (or the one table) at
// smem + OFF1 + stored; SPLIT also X2 at smem + OFF2 + stored / 2.
template <class P, int OFF1, int OFF2>
__device__ __forceinline__ void or_lookup(const unsigned char *smem, u32 stored, u32 (&m)[P::MW]) {
    or_entry<P>(smem + OFF1 + stored, m);
    if constexpr (P::SPLIT) m[2] |= *(const u32 *)(smem + OFF2 + (stored >> 1));
}

// End of a lookup group (Cfg::LG): the group's ORs are pinned here (the mask
// words pass through an empty asm, so LLVM cannot re-associate every OR of a
// step into one tree at its end) and no instruction crosses the point, so
// the group's loaded words are dead before the next group's reads issue.
template <class P>
__device__ __forceinline__ void lookup_group_end(u32 (&m)[P::MW]) {
#pragma unroll
    for (int w = 0; w < P::MW; w++) asm volatile("" : "+v"(m[w]));
    __builtin_amdgcn_sched_barrier(0);
}

// Digit bits of a scaled limb (vs = ES v, v < B) by VALU: the high digit by
// one multiply-high, the low one by a multiply-subtract, each bit set with a
// 64-bit shift (digits >= 64 land in mask word 2 at MW = 3).
template <class P>
__device__ __forceinline__ void or_valu(u32 vs, u32 (&m)[P::MW]) {
    const u32 q = __umulhi(vs, P::MAGIC_D);                        // high digit
    const u32 r = mad_i24s<-P::BASE>(q, vs / (u32)P::ES);          // low digit
    if constexpr (P::MW == 2) {
        const u64 bits = (1ull << q) | (1ull << r);
        m[0] |= (u32)bits;
        m[1] |= (u32)(bits >> 32);
    } else {
        // Digit d < 96 without compares or selects: a 64-bit shift by d
        // (the hardware takes d mod 64) is right in words 0 and 1 for d < 64,
        // and for d >= 64 leaves bit d - 64 in word 0 and nothing in word 1;
        // word 2's bit is bit 6 of d shifted by d mod 32, which is exactly that
        // stray bit, so XOR-ing it out of word 0 leaves every word right.
        const u64 bq = 1ull << (q & 63), br = 1ull << (r & 63);
        const u32 wq = __builtin_amdgcn_ubfe(q, 6, 1) << (q & 31), wr = __builtin_amdgcn_ubfe(r, 6, 1) << (r & 31);
        m[0] |= ((u32)bq ^ wq) | ((u32)br ^ wr);
        m[1] |= (u32)(bq >> 32) | (u32)(br >> 32);
        m[2] |= wq | wr;
    }
}

template <class P>
__device__ __forceinline__ void or_plain(const unsigned char *smem, u32 v, int digits, u32 (&m)[P::MW]) {
    if (digits == 2) {
        if constexpr (P::NOTAB) or_valu<P>(v * P::ES, m);
        else or_lookup<P, P::TB, P::T2>(smem, v * P::ES, m);
    } else {
#pragma unroll
        for (int w = 0; w < P::MW; w++) m[w] |= (v >> 5) == (u32)w ? 1u << (v & 31) : 0u;
    }
}

template <class P>
__device__ __forceinline__ void recompute_hi(State<P> &st, const unsigned char *smem) {
#pragma unroll
    for (int w = 0; w < P::MW; w++) st.hi[w] = 0;
#pragma unroll
    for (int i = P::SL; i < P::NS; i++) or_plain<P>(smem, st.S[i], i == P::NS - 1 ? P::S_TOPD : 2, st.hi);
#pragma unroll
    for (int i = P::CL; i < P::NC; i++) or_plain<P>(smem, st.C[i], i == P::NC - 1 ? P::C_TOPD : 2, st.hi);
}

// Radix-B normalisation of u64 column sums into M limbs (the value fits by the
// host's choice of limb counts; a carry past limb M-1 is dropped).
template <class P, int N, int M>
__device__ __forceinline__ void normalize64(const u64 (&acc)[N], u32 (&out)[M]) {
    u64 cy = 0;
#pragma unroll
    for (int t = 0; t < M; t++) {
        u64 v = (t < N ? acc[t] : 0) + cy;
        out[t] = (u32)(v % P::B);
        cy = v / P::B;
    }
}

// Radix-B normalisation of column sums into M limbs (the value fits by the
// host's choice of limb counts; a carry past limb M-1 is dropped).  A is u32
// where every column sum fits 32 bits (static_assert in init), else u64.
template <class P, class A, int N, int M>
__device__ __forceinline__ void normalize(const A (&acc)[N], u32 (&out)[M]) {
    A cy = 0;
#pragma unroll
    for (int t = 0; t < M; t++) {
        const A v = (t < N ? acc[t] : (A)0) + cy;
        cy = v / P::B;
        out[t] = (u32)(v - cy * P::B);
    }
}

// Radix-B digits X of n.
template <class P>
__device__ __forceinline__ void init_digits(u32 (&X)[P::NX], u64 n_lo, u64 n_hi) {
    constexpr u32 B = P::B;
    if constexpr (P::N64) {
        // In-range n fits 64 bits (b40 < 2^43, b50 < 2^57): two radix-B digits
        // per u64 division by B^2, the rest in 32 bits.
        (void)n_hi;
        constexpr u64 B2 = (u64)B * B;
        u64 v = n_lo;
#pragma unroll
        for (int j = 0; j < P::NX; j += 2) {
            const u64 q = v / B2;
            const u32 r = (u32)(v - q * B2);
            X[j] = r % B;
            if (j + 1 < P::NX) X[j + 1] = r / B;
            v = q;
        }
    } else {
        u32 w[4] = {(u32)n_lo, (u32)(n_lo >> 32), (u32)n_hi, (u32)(n_hi >> 32)};
#pragma unroll
        for (int j = 0; j < P::NX; j++) {
            u64 rem = 0;
#pragma unroll
            for (int q = 3; q >= 0; q--) {
                u64 cur = (rem << 32) | w[q];
                w[q] = (u32)(cur / B);
                rem = cur % B;
            }
            X[j] = (u32)rem;
        }
    }
}

// Plain (unscaled, unbiased) limbs of S = n^2, C = n^3, D1 = 2n + 1 and
// N3 = 3n + 1 from n's digits X, and the low-digit offsets.
template <class P>
__device__ __forceinline__ void init_plain(State<P> &st, const u32 (&X)[P::NX]) {
    // Column sums: at most min(NS, NX) products < B^2 plus a carry: 32 bits
    // (Cfg static_assert).
    using A = u32;
    if constexpr (P::C64) {
        // wide bases (b80: the 1024-thread kernel at the 128-VGPR cap): u64
        // columns, the layout whose register allocation spills least.
        st.r8 = X[0] * P::ES + (P::LSDX ? (u32)P::TL : 0u);
        st.rc = X[0] + (u32)P::TK;
        {
            u64 acc[2 * P::NX];
#pragma unroll
            for (int t = 0; t < 2 * P::NX; t++) acc[t] = 0;
#pragma unroll
            for (int i = 0; i < P::NX; i++)
#pragma unroll
                for (int j = 0; j < P::NX; j++) acc[i + j] += (u64)X[i] * X[j];
            normalize64<P>(acc, st.S);
        }
        {
            u64 acc[P::NS + P::NX];
#pragma unroll
            for (int t = 0; t < P::NS + P::NX; t++) acc[t] = 0;
#pragma unroll
            for (int i = 0; i < P::NS; i++)
#pragma unroll
                for (int j = 0; j < P::NX; j++) acc[i + j] += (u64)st.S[i] * X[j];
            normalize64<P>(acc, st.C);
        }
        {
            u64 acc[P::NX];
#pragma unroll
            for (int t = 0; t < P::NX; t++) acc[t] = 2ull * X[t] + (t == 0 ? 1 : 0);
            normalize64<P>(acc, st.D1);
        }
        {
            u64 acc[P::NX];
#pragma unroll
            for (int t = 0; t < P::NX; t++) acc[t] = 3ull * X[t] + (t == 0 ? 1 : 0);
            normalize64<P>(acc, st.N3);
        }
    } else {
        st.r8 = X[0] * P::ES + (P::LSDX ? (u32)P::TL : 0u);
        st.rc = X[0] + (u32)P::TK;
        {  // S = X^2
            A acc[2 * P::NX];
#pragma unroll
            for (int t = 0; t < 2 * P::NX; t++) acc[t] = 0;
#pragma unroll
            for (int i = 0; i < P::NX; i++)
#pragma unroll
                for (int j = 0; j < P::NX; j++) acc[i + j] += (A)X[i] * X[j];
            normalize<P>(acc, st.S);
        }
        {  // C = S * X
            A acc[P::NS + P::NX];
#pragma unroll
            for (int t = 0; t < P::NS + P::NX; t++) acc[t] = 0;
#pragma unroll
            for (int i = 0; i < P::NS; i++)
#pragma unroll
                for (int j = 0; j < P::NX; j++) acc[i + j] += (A)st.S[i] * X[j];
            normalize<P>(acc, st.C);
        }
        {  // D1 = 2n + 1
            A acc[P::NX];
#pragma unroll
            for (int t = 0; t < P::NX; t++) acc[t] = 2 * (A)X[t] + (t == 0 ? 1 : 0);
            normalize<P>(acc, st.D1);
        }
        {  // N3 = 3n + 1
            A acc[P::NX];
#pragma unroll
            for (int t = 0; t < P::NX; t++) acc[t] = 3 * (A)X[t] + (t == 0 ? 1 : 0);
            normalize<P>(acc, st.N3);
        }
    }
}

// Plain limbs -> the stepped representation (scaled by the entry stride,
// biased; limb 0 from the low-digit table where there is one).
template <class P>
__device__ __forceinline__ void init_scale(State<P> &st) {
    if constexpr (P::LSD) st.S[0] = st.C[0] = st.D1[0] = st.N3[0] = 0;  // from the table
#pragma unroll
    for (int i = 0; i < P::SL; i++) st.S[i] = (st.S[i] + P::BT) * P::ES;
#pragma unroll
    for (int i = 0; i < P::CL; i++) st.C[i] *= P::ES;  // unbiased: carries by multiply-high
#pragma unroll
    for (int i = 0; i < P::ND; i++) st.D1[i] *= P::ES;
#pragma unroll
    for (int i = 0; i < P::NN; i++) st.N3[i] = st.N3[i] * P::ES - (i < P::SL ? 3 * P::EBT : 0u);
}

// Lane state at n (every limb but the cached mask, which needs the tables:
// recompute_hi after them).
template <class P>
__device__ __forceinline__ void init(State<P> &st, u64 n_lo, u64 n_hi) {
    u32 X[P::NX];
    init_digits<P>(X, n_lo, n_hi);
    init_plain<P>(st, X);
    init_scale<P>(st);
}

// Radix-B digits of n = base + off from the host's digits of the launch part's
// first n (Fd2Args::xs / xt) and the lane's offset off < B^4: one u64
// division by B^2 and two u32 splits, then a carried add -- instead of the
// 128-bit n's NX x 4 u64 divisions by B (init_digits on the bases whose n
// passes 64 bits, where the radix conversion was most of a lane's init).
template <class P>
__device__ __forceinline__ void digits_plus(u32 (&X)[P::NX], const u32 *xb, u64 off) {
    constexpr u32 B = P::B;
    constexpr u64 B2 = (u64)B * B;
    const u64 q = off / B2;
    const u32 r = (u32)(off - q * B2), qq = (u32)q;
    const u32 o[4] = {r % B, r / B, qq % B, qq / B};
    u32 c = 0;
#pragma unroll
    for (int i = 0; i < P::NX; i++) {
        const u32 t = xb[i] + (i < 4 ? o[i] : 0u) + c;
        c = t >= B ? 1u : 0u;
        X[i] = t - c * B;
    }
}

// init at base + off (base: the launch part whose digits the host passed).
// Bases whose in-range n fits 64 bits keep init(): their conversion is two
// u64 divisions.  So do the 1024-thread kernels (u64 columns): there the
// digits path measured 1.3 % slower on b80 1e9 (6.29 vs 6.21 ms), while the
// 512-thread small-field kernel gained 3.5 % on b80 1e6 (19.2 vs 19.9 us in
// the A/B harness; profiles/r06/init_ab_b80.log).
template <class P>
__device__ __forceinline__ void init_at(State<P> &st, const u32 *xb, u64 off, u64 n_lo, u64 n_hi) {
    if constexpr (P::N64 || P::C64) {
        (void)xb;
        (void)off;
        init<P>(st, n_lo, n_hi);
    } else {
        (void)n_lo;
        (void)n_hi;
        u32 X[P::NX];
        digits_plus<P>(X, xb, off);
        init_plain<P>(st, X);
        init_scale<P>(st);
    }
}

// +ES into scaled plain limbs [from, N) (rare path).
template <class P, int N>
__device__ __forceinline__ void carry_scaled(u32 (&x)[N], int from) {
    u32 c = 1;
#pragma unroll
    for (int i = 0; i < N; i++) {
        if (i < from) continue;
        u32 v = x[i] + c * P::ES;
        c = v >= P::ESB;
        x[i] = c ? 0u : v;
    }
}
// +1 into plain limbs [from, N) (rare path).
template <class P, int N>
__device__ __forceinline__ void carry_plain(u32 (&x)[N], int from) {
    u32 c = 1;
#pragma unroll
    for (int i = 0; i < N; i++) {
        if (i < from) continue;
        u32 v = x[i] + c;
        c = v == P::B;
        x[i] = c ? 0u : v;
    }
}

// +ES into N3 limbs [1, NN) (offset limbs, rare path).
template <class P>
__device__ __forceinline__ void carry_n3(State<P> &st) {
    u32 c = 1;
#pragma unroll
    for (int i = 1; i < P::NN; i++) {
        const u32 off = i < P::SL ? 3 * P::EBT : 0u;
        u32 v = st.N3[i] + off + c * P::ES;
        c = v >= P::ESB;
        st.N3[i] = (c ? 0u : v) - off;
    }
}

// Rare path: a limb-0 wrap of D1 / N3, or a carry out of the top stepped
// limb of S (tS >= 2^SH, biased) or C (tC >= ES B).  The top stepped limbs
// are left unreduced by step(): they only take carries, so they need
// reducing only here.
template <class P>
__device__ __forceinline__ void rare(State<P> &st, const unsigned char *smem, u32 d1w, u32 n3w, bool cS,
                                     bool cC) {
    if (d1w) carry_scaled<P>(st.D1, 1);
    if (n3w) carry_n3<P>(st);
    if (cS) {
        st.S[P::SL - 1] -= P::ESB;
        carry_plain<P>(st.S, P::SL);
    }
    if (cC) {
        st.C[P::CL - 1] -= P::DC;
        carry_plain<P>(st.C, P::CL);
    }
    if (cS | cC) recompute_hi<P>(st, smem);
}

// The two arithmetics of a limb chain (Cfg::FMA), in three places each: the
// carry coming in, a bare carry being scaled, and the limb's reduction, which
// returns the carry in the form the chain passes on -- the integer form c * ES
// (S: the bit itself, 0 or ES), the f32 form c unscaled (ES B = DC reduces
// both chains).  Everything between them is the same code for both.
template <class P>
__device__ __forceinline__ u32 carry_in(u32 c, u32 x) {
    if constexpr (P::FMA) return fma_bits<P::ES>(c, x);
    else return x + c;
}
template <class P>
__device__ __forceinline__ u32 scale_in(u32 c, u32 x) {  // x + ES c, c bare
    if constexpr (P::FMA) return fma_bits<P::ES>(c, x);
    else return mad_u24<P::ES>(c, x);
}
template <class P>
__device__ __forceinline__ u32 c_reduce(u32 &limb, u32 t) {
    const u32 c = P::C1 ? __umulhi(t, P::MAGIC) : __umulhi(t / P::ES, P::MAGICB);
    if constexpr (P::FMA) {
        limb = fma_bits<-(int)P::DC>(c, t);
        return c;
    } else {
        limb = t - c * P::DC;
        return c * P::ES;
    }
}
template <class P>
__device__ __forceinline__ u32 s_reduce(u32 &limb, u32 t) {
    if constexpr (P::FMA) {
        const u32 c = t >> P::SH;  // t < 2^(SH+1): the bit alone
        limb = fma_bits<-(int)P::DC>(c, t);
        return c;
    } else {
        const u32 c = (t >> P::T) & P::ES;
        limb = t - c * P::B;
        return c;
    }
}

// One FD step n -> n+1.  w1 = word 1 of the low-digit entry of n (LSD bases):
// limb 0 of every quantity lives in the table, so the chains start at limb 1
// with the table's carries.  The carry leaves each limb as c8 = ES * carry,
// (t >> T) & ES; the limb is reduced with one v_mad_i32_i24.  The top stepped
// limb of S and of C only ever receives a carry (D1 and 3S + N3 are shorter),
// so it is just compared: a carry out of it (~1/B per step) goes to rare().
template <class P>
__device__ __forceinline__ void step(State<P> &st, const unsigned char *smem, u32 w1) {
    constexpr u32 ES = P::ES;
    constexpr int L0 = P::LO;  // LSD bases: limb 0 lives in the low-digit table
    constexpr int CT = P::CL - 1, ST = P::SL - 1;  // top stepped limbs
    static_assert(CT >= P::NS && CT >= P::NN && ST >= P::ND, "top limbs take carries only");
    static_assert(CT > L0 && ST > L0, "a stepped limb below the top one: its carry is in the chain's form");
    // C += 3S + N3 (old S), limbs L0 .. CL-1.  Unbiased scaled limbs; a limb
    // sum is < 5B, its carry (0..4) is a multiply-high.
    u32 cC = 0;
    if constexpr (P::LSD) cC = __builtin_amdgcn_ubfe(w1, P::FC, P::FCW);  // TIGHT: bare carry
#pragma unroll
    for (int i = L0; i < CT; i++) {
        u32 t;
        if (P::TIGHT && i == L0) t = scale_in<P>(cC, st.C[i]);  // scale the bare carry
        else if (i == L0) t = st.C[i] + cC;  // the table's carry: pre-scaled (or none)
        else t = carry_in<P>(cC, st.C[i]);
        // Past limb L0 the carry is c * ES from a multiply-high: keep C + c*ES
        // one v_lshl_add_u32 and add N3 with a plain v_add_u32 (LLVM would
        // otherwise emit v_lshlrev_b32 + v_add3_u32, ~2 issue cycles more).
        if (i > L0 && i < P::NN) asm("" : "+v"(t));
        if (i < P::NN) t += st.N3[i];
        else if (i < P::SL) t -= 3 * P::EBT;
        // + 3S as one v_mad_u32_u24 (limbs < 2^24)
        if (i < P::SL) t = mad_u24<3>(st.S[i], t);
        else if (i < P::NS) t = mad_u24<3 * ES>(st.S[i], t);
        cC = c_reduce<P>(st.C[i], t);
    }
    st.C[CT] = carry_in<P>(cC, st.C[CT]);  // < DC + 4 ES: a carry out is at most 1
    // S += D1, limbs L0 .. SL-1 (biased: carry = bit T of t >> log2 ES).
    u32 cS = 0;
    if constexpr (P::LSD) cS = __builtin_amdgcn_ubfe(w1, P::F0, P::F0W);  // TIGHT: bare carry
#pragma unroll
    for (int i = L0; i < ST; i++) {
        u32 t;
        if (P::TIGHT && i == L0) t = scale_in<P>(cS, st.S[i] + (i < P::ND ? st.D1[i] : 0u));
        else if (i == L0) t = st.S[i] + (i < P::ND ? st.D1[i] : 0u) + cS;
        else t = carry_in<P>(cS, st.S[i] + (i < P::ND ? st.D1[i] : 0u));
        cS = s_reduce<P>(st.S[i], t);
    }
    st.S[ST] = carry_in<P>(cS, st.S[ST]);
    st.r8 += ES;
    if constexpr (P::LSDX) st.rc += 1;
    const bool topS = st.S[ST] >= (1u << P::SH), topC = st.C[CT] >= P::DC;
    if constexpr (P::LSD) {
        if (w1 >= P::FLAG_D1 || topS || topC)
            rare<P>(st, smem, w1 & P::FLAG_D1, w1 & P::FLAG_N3, topS, topC);
    } else {
        // limb 0 of D1 (+2) and N3 (+3, stored offset by -3 ES BT) step here
        st.D1[0] += 2 * ES;
        st.N3[0] += 3 * ES;
        const u32 d1w = st.D1[0] >= P::ESB, n3w = st.N3[0] + 3 * P::EBT >= P::ESB;
        if (d1w || n3w || topS || topC) {
            if (d1w) st.D1[0] -= P::ESB;
            if (n3w) st.N3[0] -= P::ESB;
            rare<P>(st, smem, d1w, n3w, topS, topC);
        }
    }
}

// Table image (the LDS bytes from TB on): digit-pair table, entry e = d1*b +
// d0 marks d0 and d1; low-digit table (LSD bases), entry r < 2B marks the two
// low digits of r^2 and of r^3 (mod B) plus the limb-0 carries and wraps.
template <class P>
__global__ void fd2_tables_kernel(unsigned char *tb) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= P::B) return;
    u32 v[4] = {0, 0, 0, 0};
    auto mark = [&](u32 x) {
        u32 d0 = x % P::BASE, d1 = x / P::BASE;
        v[d0 >> 5] |= 1u << (d0 & 31);
        v[d1 >> 5] |= 1u << (d1 & 31);
    };
    auto put = [&](unsigned char *p) {
        if constexpr (P::ES == 4) *(u32 *)p = v[0];
        else if constexpr (P::ES == 8) *(uint2 *)p = make_uint2(v[0], v[1]);
        else *(uint4 *)p = make_uint4(v[0], v[1], v[2], v[3]);
    };
    mark(e);
    put(tb + (P::TB - P::TC0) + e * P::ES);
    if constexpr (P::SPLIT) *(u32 *)(tb + (P::T2 - P::TC0) + 4 * e) = v[2];  // X2: digits 64..
    if constexpr (P::LSD) {
        v[0] = v[1] = v[2] = v[3] = 0;
        const u32 B = P::B;
        const u32 s0 = (u32)((u64)e * e % B), c0 = (u32)((u64)s0 * e % B);
        mark(s0);
        mark(c0);
        const u32 d1 = (2 * e + 1) % B, n3 = (3 * e + 1) % B;
        u32 f = 0;
        f |= d1 + 2 >= B ? P::FLAG_D1 : 0u;                   // D1 limb-0 wrap
        f |= n3 + 3 >= B ? P::FLAG_N3 : 0u;                   // N3 limb-0 wrap
        const u32 sc = s0 + d1 >= B ? 1u : 0u, cc = (c0 + 3 * s0 + n3) / B;
        f |= (P::TIGHT ? sc : P::ES * sc) << P::F0;            // S  += D1 carry
        f |= (P::TIGHT ? cc : P::ES * cc) << P::FC;            // C += 3S + N3 carry
        if constexpr (P::LSDX) {
            tb[(P::TK - P::TC0) + e] = (unsigned char)f;
            tb[(P::TK - P::TC0) + e + P::B] = (unsigned char)f;
        } else {
            v[1] |= f;
        }
        put(tb + (P::TL - P::TC0) + e * P::ES);
        if ((int)(e + P::B) < P::LDE) put(tb + (P::TL - P::TC0) + (e + P::B) * P::ES);
    }
}

// One launch covers a whole segment: blocks [0, main_blocks) walk `nunits`
// chunks of `chunk` numbers from `start`; the blocks after them take the
// < chunk numbers left over, one per lane, from `tail` (same code, chunk 1:
// every parameter stays wave-uniform, and no second launch is serialised
// behind the first).  With fin.out set, the launch also finishes the field:
// the last workgroup to retire sums the kHistCopies histogram copies into
// the caller's mapped result words and re-zeroes the state block, so a field
// is ONE launch instead of main + tail + epilogue (under several fields in
// flight each small launch waited for free CUs: 25-60 us apiece).
// Probe build: per-workgroup phase stamps (scripts/fd2_stamps.py).  When
// g_stamps (host, fd2_launch.hpp, set by nice_probe_fd2_stamps) is non-null, thread 0 of each
// workgroup b < kStampGroups writes kStampWords words at stamps + kStampWords b:
// for each phase k the constant 100 MHz real-time counter (word 2k) and the
// shader clock (word 2k + 1).  The stamps go only to that buffer; nothing
// reads them on the device.  Phases 7..9 are the finishing workgroup's
// field finish.  (Product build: kProbes is false and Fd2Args::stamps null, so
// a stamp compiles to nothing.)
constexpr u32 kStampGroups = 65536, kStampWords = 32;
#define FD2_STAMP_P(p, k)                                                                        \
    do {                                                                                         \
        if (kProbes && (p) && threadIdx.x == 0 && blockIdx.x < kStampGroups) {                   \
            (p)[kStampWords * (u64)blockIdx.x + 2 * (k)] = __builtin_amdgcn_s_memrealtime();     \
            (p)[kStampWords * (u64)blockIdx.x + 2 * (k) + 1] = __builtin_amdgcn_s_memtime();     \
        }                                                                                        \
    } while (0)
#define FD2_STAMP(a, k) FD2_STAMP_P((a).stamps, k)
// The sibling parts stamp phases 14 (barrier passed) and 15 (thread 0's steps
// done), and lane 0 of wave w < 8 the shader clock at the end of the wave's
// steps into word 20 + w (the spread of a workgroup's wave finish times).
#define FD2_WAVE_STAMP(a)                                                                        \
    do {                                                                                         \
        if (kProbes && (a).stamps && (threadIdx.x & 63) == 0 && threadIdx.x < 512 &&             \
            blockIdx.x < kStampGroups)                                                           \
            (a).stamps[kStampWords * (u64)blockIdx.x + 20 + (threadIdx.x >> 6)] =                \
                __builtin_amdgcn_s_memtime();                                                    \
    } while (0)

struct Fd2Args {
    u64 *stamps;  // probe build: phase stamps (null in the product build)
    u64 start_lo, start_hi;
    u64 tail_lo, tail_hi;
    u32 nunits, chunk;
    u32 tail_count, main_blocks;
    u32 cutoff;
    u32 ncopies;        // histogram copies in use (<= kHistCopies), the same for every launch of a field
    u32 wave_cap;       // persistent grid: batches one wave may take (its lanes' u16 counters hold them)
    // Cfg::SIB > 1: blocks [0, sib_blocks) walk sibling units (q, k) -> n0 =
    // sib + q M B^2 + k sib_chunk, k < sib_upb; blocks [sib_blocks,
    // sib_blocks + edge_blocks) the edge units q -> edge + q M B^2 (chunk
    // edge_chunk: the rest of each B^2 block); the regular parts follow.
    u64 sib_lo, sib_hi, edge_lo, edge_hi;
    u32 sib_chunk, sib_upb, sib_units, sib_blocks;
    u32 edge_chunk, edge_units, edge_blocks;
    // radix-B digits of start (xs) and tail (xt), least significant first,
    // for init_at (bases whose n passes 64 bits; kXDigits >= NX)
    u32 xs[12], xt[12];
    u64 *hist;          // kHistCopies x kHistBins bins
    NumOut out;
    const uint4 *tabs;
    FieldFinish fin;    // fin.out_mapped == nullptr: no in-kernel finish
};

// Last-workgroup finish (see Fd2Args).  smem is reused as scratch (>= 1 KB).
// Hand-off without any L2 write-back (MI355X_MICROARCH.md, inter-workgroup
// visibility: agent atomics both sides, the last arriver told by its add's
// return value): every wave waits for its own histogram atomics
// (vmcnt(0)), a barrier, ONE agent-scope add per workgroup; the last
// workgroup reads the copies with agent-scope (sc1) loads.  A __threadfence()
// here would write back and invalidate the XCD's whole L2 once per
// workgroup: 12 000 of them made the b40 1e9 field 1.8x slower.
template <int WG>
__device__ __forceinline__ void field_finish(const FieldFinish &fin, u64 *hist, u32 ncopies, u32 nbins, u32 *count,
                                             unsigned char *smem, u64 *stamps) {
    (void)stamps;
    __shared__ u32 last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) last = last_block_arrive(fin.done);
    __syncthreads();
    if (!last) return;
    FD2_STAMP_P(stamps, 7);  // the last workgroup: arrival known
    unsigned long long *acc = (unsigned long long *)smem;
    for (u32 b = threadIdx.x; b < kHistBins; b += WG) acc[b] = 0;
    __syncthreads();
    // All of a lane's loads issued before the first is used: one L2 round
    // trip for the copies instead of one per copy row.  Only bins < nbins
    // (base + 1) are read: the field's launches touch no other bin, and every
    // finish leaves the bins it read at zero (the generic kernel's finish
    // kernel zeroes all of them).
    constexpr u32 PER = (kHistCopies * kHistBins + WG - 1) / WG;
    const u32 NE = ncopies * nbins;
    const u32 nmiss = threadIdx.x == 0 ? __hip_atomic_load(count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    u64 v[PER];
    u32 at[PER];
#pragma unroll
    for (u32 k = 0; k < PER; k++) {
        const u32 e = threadIdx.x + k * WG;
        const u32 c = e / nbins, b = e - c * nbins;
        at[k] = c * kHistBins + b;
        v[k] = e < NE ? __hip_atomic_load(&hist[at[k]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    }
#pragma unroll
    for (u32 k = 0; k < PER; k++) {
        if (v[k]) {
            atomicAdd(&acc[at[k] % kHistBins], (unsigned long long)v[k]);
            __hip_atomic_store(&hist[at[k]], (u64)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    FD2_STAMP_P(stamps, 8);  // copies read and summed
    done_reset(fin.done);
    if (fin.tag) {
        // tagged words (FieldFinish::tag): no store-completion wait, no
        // sequence word; the kernel's end orders the re-zeroing for the slot's
        // next field
        const u64 t = (u64)fin.tag << 32;
        for (u32 b = threadIdx.x; b < nbins; b += WG) fin.out_mapped[b] = t | (u32)acc[b];
        if (threadIdx.x == 0) {
            fin.out_mapped[kFinCount] = t | nmiss;
            __hip_atomic_store(count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        FD2_STAMP_P(stamps, 9);
        return;
    }
    for (u32 b = threadIdx.x; b < kHistBins; b += WG) fin.out_mapped[b] = acc[b];
    if (threadIdx.x == 0) {
        fin.out_mapped[kFinCount] = nmiss;
        __hip_atomic_store(count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // Publish: every lane's mapped stores complete, then one system-scope
    // release store of the sequence number (once per field, so its L2
    // write-back costs nothing measurable).
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    FD2_STAMP_P(stamps, 9);  // mapped stores complete
    if (threadIdx.x == 0)
        __hip_atomic_store(&fin.out_mapped[kFinSeq], fin.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// One lane's chunk: `chunk` numbers from n0 (the state at n0 built by init;
// the cached high limbs' mask is built here, it needs the tables).
template <class P>
__device__ __forceinline__ void walk_chunk(State<P> &st, const unsigned char *smem, u32 chunk, u64 n0_lo,
                                           u64 n0_hi, u32 hbase, u32 hinc, u32 *outl, u32 cutoff,
                                           const NumOut &out, u32 &probe_acc) {
    recompute_hi<P>(st, smem);
    const u32 r80 = st.r8;
    for (u32 i = 0; i < chunk; i++) {
        u32 m[P::MW], w1 = 0;
#pragma unroll
        for (int w = 0; w < P::MW; w++) m[w] = st.hi[w];
        if constexpr (P::PROBE & 1) {
            m[0] |= st.r8;
            w1 = st.r8 & 0xff;
#pragma unroll
            for (int q = P::LO; q < P::SL; q++) m[q & 1] |= st.S[q];
#pragma unroll
            for (int q = P::LO; q < P::CL; q++) m[q & 1] |= st.C[q];
        } else {
            if constexpr (P::LSD) {
                const uint2 v = *(const uint2 *)(smem + (P::LSDX ? 0 : P::TL) + st.r8);
                m[0] |= v.x;
                if constexpr (P::LSDX) {
                    m[1] |= v.y;
                    w1 = smem[st.rc];
                } else {
                    m[1] |= v.y & P::DMASK;
                    w1 = v.y;
                }
            }
#pragma unroll
            for (int q = P::LO; q < P::SL; q++) {
                if ((P::PROBE & 4) && q == 1) { m[0] |= st.S[q] & 0xffu; continue; }  // probe: no limb-1 lookups
                if (P::vd_s(q) || (P::VDL && q == 0)) or_valu<P>(st.S[q] - P::EBT, m);
                else or_lookup<P, P::TB - (int)P::EBT, P::T2 - (int)P::EBT / 2>(smem, st.S[q], m);
                if (P::LGW && (q - P::LO + 1) % P::LGW == 0) lookup_group_end<P>(m);
            }
#pragma unroll
            for (int q = P::LO; q < P::CL; q++) {
                if ((P::PROBE & 4) && q == 1) { m[1] |= st.C[q] & 0xffu; continue; }
                if (P::vd_c(q) || (P::VDL && q == 0)) or_valu<P>(st.C[q], m);
                else or_lookup<P, P::TB, P::T2>(smem, st.C[q], m);
                if (P::LGW && (P::SL + q - 2 * P::LO + 1) % P::LGW == 0) lookup_group_end<P>(m);
            }
        }
        // uw = unique count - W0: the bias rides in the first v_bcnt's
        // accumulator operand (an SGPR; LLVM would add it separately).
        u32 uw = bcnt_acc(m[0], (u32)(-P::W0));
#pragma unroll
        for (int w = 1; w < P::MW; w++) uw += __popc(m[w]);
        if (uw < (u32)P::W) {
            if constexpr (P::PROBE & 2) probe_acc++;
            else atomicAdd((u32 *)(smem + uw * (P::HROW * 4) + hbase), hinc);
        } else {
            const u32 u = uw + P::W0;
            atomicAdd(&outl[u], 1u);
            if (u > cutoff) {
                u64 lo = n0_lo, hi = n0_hi;
                add_u128(lo, hi, (st.r8 - r80) / P::ES);  // = i (keeps i scalar)
                u32 pos = atomicAdd(out.count, 1u);
                if (pos < out.cap) {
                    out.n[2 * (u64)pos] = lo;
                    out.n[2 * (u64)pos + 1] = hi;
                    out.u[pos] = u;
                }
            }
        }
        step<P>(st, smem, w1);
    }
}

// ---------------------------------------------------------------------------
// Sibling lanes (Cfg::SIB = M > 1).  A lane steps the M numbers n + j B^2
// (j < M) together.  They agree mod B^2, so limbs 0 and 1 of n^2, n^3, D1 =
// 2n + 1 and N3 = 3n + 1 are equal for all of them, and so is every chain's
// carry out of limb 1: the low-digit entry (limb 0 of S and C, with the
// carries and wrap flags), the two limb-1 lookups and limb 1's carry chains
// are done once per step for M numbers.  Sibling 0's State holds the shared
// limbs (its S[1], C[1], D1[1], N3[1], r8); the other siblings' copies of
// them are never read.  Limbs >= 2, the cached high limbs and their mask are
// each sibling's own.  Per n: b40 M = 2 goes from 12 lookups and ~266 VALU
// cycles per wave-step to 10.5 and ~240.
// ---------------------------------------------------------------------------

// One C limb i > LO of C += 3S + N3 (old S) with the carry-in cC in the
// chain's form (c_reduce); returns the carry out (step() does the same inline).  The cached S
// limbs [SL, NS) of a sibling are held as K = 3 ES S (they change only on the
// rare path), so their term is one add.
template <class P>
__device__ __forceinline__ u32 c_limb(State<P> &st, int i, u32 cC) {
    u32 t = carry_in<P>(cC, st.C[i]);
    if (i < P::NN) asm("" : "+v"(t));
    if (i < P::NN) t += st.N3[i];
    else if (i < P::SL) t -= 3 * P::EBT;
    if (i < P::SL) t = mad_u24<3>(st.S[i], t);
    else if (i < P::NS) t += st.S[i];
    // (The scaled carry straight from one multiply-high, mulhi(t, ES MAGIC) &
    // -ES, prices 18 cycles fewer per step in the issue budget but measured
    // 0.6-2.2 % slower, interleaved A/B: profiles/r05/carry_c8_ab.log.)
    return c_reduce<P>(st.C[i], t);
}

// One S limb i > LO of S += D1 (biased) with the carry-in cS in the chain's form.
template <class P>
__device__ __forceinline__ u32 s_limb(State<P> &st, int i, u32 cS) {
    return s_reduce<P>(st.S[i], carry_in<P>(cS, st.S[i] + (i < P::ND ? st.D1[i] : 0u)));
}

// A sibling's cold C limb k (C[CL + k]) in LDS.
template <class P>
__device__ __forceinline__ unsigned short *cold_slot(const unsigned char *smem, int j, int k) {
    return (unsigned short *)(smem + P::COLD) + ((u32)(j * P::NCOLD + k) * P::WG + threadIdx.x);
}

// recompute_hi for a sibling: cached S limbs in K form, cached C limbs in LDS.
template <class P>
__device__ __forceinline__ void sib_hi(State<P> &st, int j, const unsigned char *smem) {
#pragma unroll
    for (int w = 0; w < P::MW; w++) st.hi[w] = 0;
#pragma unroll
    for (int i = P::SL; i < P::NS; i++)
        or_plain<P>(smem, st.S[i] / (3 * P::ES), i == P::NS - 1 ? P::S_TOPD : 2, st.hi);
#pragma unroll
    for (int k = 0; k < P::NCOLD; k++)
        or_plain<P>(smem, *cold_slot<P>(smem, j, k), P::CL + k == P::NC - 1 ? P::C_TOPD : 2, st.hi);
}

// Plain limbs of sibling j (n + j B^2) from sibling 0's plain limbs and n's
// digits X: (n + j B^2)^2 = S + 2 j n B^2 + j^2 B^4 and (n + j B^2)^3 = C +
// 3 j S B^2 + 3 j^2 n B^4 + j^3 B^6 -- column adds and one normalisation
// instead of sibling j's own radix conversion and products (~1/3 of a
// lane's init each).
template <class P>
__device__ __forceinline__ void sib_derive(State<P> &sj, const State<P> &s0, const u32 (&X)[P::NX], u32 j) {
    {
        u32 acc[P::NS];
#pragma unroll
        for (int t = 0; t < P::NS; t++)
            acc[t] = s0.S[t] + (t >= 2 && t - 2 < P::NX ? 2 * j * X[t - 2] : 0u) + (t == 4 ? j * j : 0u);
        normalize<P>(acc, sj.S);
    }
    {
        u32 acc[P::NC];
#pragma unroll
        for (int t = 0; t < P::NC; t++)
            acc[t] = s0.C[t] + (t >= 2 && t - 2 < P::NS ? 3 * j * s0.S[t - 2] : 0u) +
                     (t >= 4 && t - 4 < P::NX ? 3 * j * j * X[t - 4] : 0u) + (t == 6 ? j * j * j : 0u);
        normalize<P>(acc, sj.C);
    }
    {
        u32 acc[P::ND];
#pragma unroll
        for (int t = 0; t < P::ND; t++) acc[t] = s0.D1[t] + (t == 2 ? 2 * j : 0u);
        normalize<P>(acc, sj.D1);
    }
    {
        u32 acc[P::NN];
#pragma unroll
        for (int t = 0; t < P::NN; t++) acc[t] = s0.N3[t] + (t == 2 ? 3 * j : 0u);
        normalize<P>(acc, sj.N3);
    }
    sj.r8 = s0.r8;
    sj.rc = s0.rc;
}

// Sibling state after init: cached S limbs to K form, cached C limbs to LDS.
template <class P>
__device__ __forceinline__ void sib_park(State<P> &st, int j, const unsigned char *smem) {
#pragma unroll
    for (int i = P::SL; i < P::NS; i++) st.S[i] *= 3 * P::ES;
#pragma unroll
    for (int k = 0; k < P::NCOLD; k++) *cold_slot<P>(smem, j, k) = (unsigned short)st.C[P::CL + k];
}

// Rare path of step_sib: limb-0 wraps of D1 / N3 (one event for all
// siblings: the shared limb 1, then each sibling's upper limbs) and carries
// out of each sibling's top stepped limbs (rare()'s work per sibling).
template <class P>
__device__ __forceinline__ void rare_sib(State<P> (&st)[P::SIB], const unsigned char *smem,
                                      const bool (&cS)[P::SIB], const bool (&cC)[P::SIB]) {
    constexpr int L = P::LO;
    // limb L of the shared D1 / N3 reached B (sib_shared_step stepped it):
    // wrap it and carry into every sibling's limbs above
    if (st[0].D1[L] >= P::ESB) {
        st[0].D1[L] -= P::ESB;
#pragma unroll
        for (int j = 0; j < P::SIB; j++) carry_scaled<P>(st[j].D1, L + 1);
    }
    {
        const u32 off1 = L < P::SL ? 3 * P::EBT : 0u;
        if (st[0].N3[L] + off1 >= P::ESB) {
            st[0].N3[L] -= P::ESB;
#pragma unroll
            for (int j = 0; j < P::SIB; j++) {
                u32 cc = 1;
#pragma unroll
                for (int i = L + 1; i < P::NN; i++) {
                    const u32 off = i < P::SL ? 3 * P::EBT : 0u;
                    const u32 w = st[j].N3[i] + off + cc * P::ES;
                    cc = w >= P::ESB;
                    st[j].N3[i] = (cc ? 0u : w) - off;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < P::SIB; j++) {
        if (cS[j]) {
            st[j].S[P::SL - 1] -= P::ESB;
            u32 c = 1;  // +1 into the cached limbs (K form: 3 ES per unit)
#pragma unroll
            for (int i = P::SL; i < P::NS; i++) {
                const u32 v = st[j].S[i] + c * 3 * P::ES;
                c = v >= 3 * P::ESB;
                st[j].S[i] = c ? 0u : v;
            }
        }
        if (cC[j]) {
            st[j].C[P::CL - 1] -= P::DC;
            u32 c = 1;
#pragma unroll
            for (int k = 0; k < P::NCOLD; k++) {
                unsigned short *slot = cold_slot<P>(smem, j, k);
                const u32 v = *slot + c;
                c = v == P::B;
                *slot = (unsigned short)(c ? 0u : v);
            }
        }
        if (cS[j] | cC[j]) sib_hi<P>(st[j], j, smem);
    }
}

template <class P>
__device__ __forceinline__ void sib_shared_step(State<P> &s0, u32 w1, u32 &cC, u32 &cS, bool &wrap);

// One FD step of all siblings (step() restated with the shared limb 1).
template <class P>
__device__ __forceinline__ void step_sib(State<P> (&st)[P::SIB], const unsigned char *smem, u32 w1) {
    constexpr int L = P::LO;
    constexpr int CT = P::CL - 1, ST = P::SL - 1;
    u32 cC, cS;
    bool any;
    sib_shared_step<P>(st[0], w1, cC, cS, any);
    bool topS[P::SIB], topC[P::SIB];
#pragma unroll
    for (int j = 0; j < P::SIB; j++) {
        u32 c = cC;
#pragma unroll
        for (int i = L + 1; i < CT; i++) c = c_limb<P>(st[j], i, c);
        st[j].C[CT] = carry_in<P>(c, st[j].C[CT]);
        u32 cs = cS;
#pragma unroll
        for (int i = L + 1; i < ST; i++) cs = s_limb<P>(st[j], i, cs);
        st[j].S[ST] = carry_in<P>(cs, st[j].S[ST]);
        topS[j] = st[j].S[ST] >= (1u << P::SH);
        topC[j] = st[j].C[CT] >= P::DC;
        any |= topS[j] | topC[j];
    }
    if (any) rare_sib<P>(st, smem, topS, topC);
}

// step_sib in pieces for the pipelined walk: the shared limb L (returns the
// carries into limb L + 1 of C and S, in the chains' form) ...
template <class P>
__device__ __forceinline__ void sib_shared_step(State<P> &s0, u32 w1, u32 &cC, u32 &cS, bool &wrap) {
    constexpr u32 ES = P::ES;
    constexpr int L = P::LO;
    static_assert(L < P::ND && L < P::NN && P::FLAG_D1 == (1u << 30) && P::FLAG_N3 == (1u << 31),
                  "sibling lanes: shared D1 / N3 limb and the low-digit entry's wrap flags");
    cC = __builtin_amdgcn_ubfe(w1, P::FC, P::FCW);
    {
        u32 t = P::TIGHT ? scale_in<P>(cC, s0.C[L]) : s0.C[L] + cC;
        if (L < P::NN) t += s0.N3[L];
        else t -= 3 * P::EBT;
        t = mad_u24<3>(s0.S[L], t);
        cC = c_reduce<P>(s0.C[L], t);
    }
    cS = __builtin_amdgcn_ubfe(w1, P::F0, P::F0W);
    {
        const u32 d = L < P::ND ? s0.D1[L] : 0u;
        const u32 t = P::TIGHT ? scale_in<P>(cS, s0.S[L] + d) : s0.S[L] + d + cS;
        cS = s_reduce<P>(s0.S[L], t);
    }
    s0.r8 += ES;
    // limb-0 wraps of D1 / N3 (the entry's flags, one in ~B / 5 steps) step
    // their limb L here, without a branch; only limb L reaching B (one in
    // ~B^2 / 5) takes the rare path.  (Branching on the flags sent a wave
    // down the rare path on ~1 in 5 steps, mostly for this increment.)
    s0.D1[L] += (w1 >> (30 - ilog2(ES))) & ES;
    s0.N3[L] += (w1 >> (31 - ilog2(ES))) & ES;
    wrap = (s0.D1[L] >= P::ESB) | (s0.N3[L] + (L < P::SL ? 3 * P::EBT : 0u) >= P::ESB);
}

// ... and one sibling's limbs above it (returns whether a top limb carried).
template <class P>
__device__ __forceinline__ bool sib_upper_step(State<P> &st, u32 cC, u32 cS, bool &topS, bool &topC) {
    constexpr int L = P::LO;
    constexpr int CT = P::CL - 1, ST = P::SL - 1;
#pragma unroll
    for (int i = L + 1; i < CT; i++) cC = c_limb<P>(st, i, cC);
    st.C[CT] = carry_in<P>(cC, st.C[CT]);
#pragma unroll
    for (int i = L + 1; i < ST; i++) cS = s_limb<P>(st, i, cS);
    st.S[ST] = carry_in<P>(cS, st.S[ST]);
    topS = st.S[ST] >= (1u << P::SH);
    topC = st.C[CT] >= P::DC;
    return topS | topC;
}

// One sibling's looked-up table entries of a step (entries of VALU-decoded
// limbs and of limbs <= L are unused).
template <class P>
struct SibLook {
    uint2 s[P::SL], c[P::CL];
};

template <class P>
__device__ __forceinline__ void sib_issue(const State<P> &st, const unsigned char *smem, SibLook<P> &e) {
#pragma unroll
    for (int q = P::LO + 1; q < P::SL; q++)
        if (!P::vd_s(q)) e.s[q] = *(const uint2 *)(smem + (P::TB - (int)P::EBT) + st.S[q]);
#pragma unroll
    for (int q = P::LO + 1; q < P::CL; q++)
        if (!P::vd_c(q)) e.c[q] = *(const uint2 *)(smem + P::TB + st.C[q]);
}

template <class P>
__device__ __forceinline__ void sib_consume(const State<P> &st, const SibLook<P> &e, u32 (&m)[P::MW]) {
#pragma unroll
    for (int q = P::LO + 1; q < P::SL; q++) {
        if (P::vd_s(q)) {
            or_valu<P>(st.S[q] - P::EBT, m);
        } else {
            m[0] |= e.s[q].x;
            m[1] |= e.s[q].y;
        }
    }
#pragma unroll
    for (int q = P::LO + 1; q < P::CL; q++) {
        if (P::vd_c(q)) {
            or_valu<P>(st.C[q], m);
        } else {
            m[0] |= e.c[q].x;
            m[1] |= e.c[q].y;
        }
    }
}

// OR the digit bits of limb q of sibling j's S (isS) or C into m.
template <class P>
__device__ __forceinline__ void or_limb(const State<P> &st, const unsigned char *smem, bool isS, int q,
                                        u32 (&m)[P::MW]) {
    if (isS) {
        if (P::vd_s(q)) or_valu<P>(st.S[q] - P::EBT, m);
        else or_lookup<P, P::TB - (int)P::EBT, P::T2 - (int)P::EBT / 2>(smem, st.S[q], m);
    } else {
        if (P::vd_c(q)) or_valu<P>(st.C[q], m);
        else or_lookup<P, P::TB, P::T2>(smem, st.C[q], m);
    }
}

// walk_chunk for M siblings: `chunk` steps of the numbers n0 + j B^2 + i.
// Sibling 0's first number of this lane's unit (fd2_body's layout of the
// sibling parts; recomputed on the rare near-miss path instead of kept live).
struct SibUnit {
    bool active;
    u32 chunk;
    u64 lo, hi;
};
// Persistent sibling grid (Cfg::SIBPERS): the 64-unit batch each wave of the
// workgroup is on, kept in LDS for the near-miss path (not live in a VGPR).
template <class P>
__device__ __forceinline__ u32 *sib_batch_slot() {
    __shared__ u32 cur[P::WG / 64];
    return &cur[threadIdx.x >> 6];
}
// ... and the unit of lane `lane` in batch b of the launch: batches [0, nsb)
// hold the sibling units 64 b + lane, the batches after them the edge units.
template <class P>
__device__ __forceinline__ SibUnit sib_unit_at(const Fd2Args &a, u32 b, u32 lane) {
    const u32 nsb = (a.sib_units + 63) / 64;
    const bool edge = b >= nsb;
    const u32 sunit = 64 * (edge ? b - nsb : b) + lane;
    const u32 upb = edge ? 1u : a.sib_upb;
    SibUnit u;
    u.active = sunit < (edge ? a.edge_units : a.sib_units);
    u.chunk = edge ? a.edge_chunk : a.sib_chunk;
    const u32 q = sunit / upb, k = sunit - q * upb;
    u.lo = edge ? a.edge_lo : a.sib_lo;
    u.hi = edge ? a.edge_hi : a.sib_hi;
    add_u128(u.lo, u.hi, (u64)q * ((u64)P::SIB * P::B * P::B) + (u64)k * u.chunk);
    return u;
}
template <class P>
__device__ __forceinline__ SibUnit sib_unit(const Fd2Args &a) {
    if constexpr (P::SIBPERS) return sib_unit_at<P>(a, *sib_batch_slot<P>(), threadIdx.x & 63);
    const bool edge = blockIdx.x >= a.sib_blocks;
    const u32 sunit = (edge ? blockIdx.x - a.sib_blocks : blockIdx.x) * P::WG + threadIdx.x;
    const u32 upb = edge ? 1u : a.sib_upb;
    SibUnit u;
    u.active = sunit < (edge ? a.edge_units : a.sib_units);
    u.chunk = edge ? a.edge_chunk : a.sib_chunk;
    const u32 q = sunit / upb, k = sunit - q * upb;
    u.lo = edge ? a.edge_lo : a.sib_lo;
    u.hi = edge ? a.edge_hi : a.sib_hi;
    add_u128(u.lo, u.hi, (u64)q * ((u64)P::SIB * P::B * P::B) + (u64)k * u.chunk);
    return u;
}

// Histogram / near-miss record of sibling j's number at step i (mask m).
template <class P>
__device__ __forceinline__ void sib_record(u32 u, int j, u32 i, const Fd2Args &a, u32 *outl, u32 cutoff,
                                           const NumOut &out);

template <class P>
__device__ __forceinline__ void sib_count(const u32 (&m)[P::MW], int j, u32 i, const unsigned char *smem,
                                          const Fd2Args &a, u32 hbase, u32 hinc, u32 *outl, u32 cutoff,
                                          const NumOut &out) {
    u32 uw = bcnt_acc(m[0], (u32)(-P::W0));
#pragma unroll
    for (int w = 1; w < P::MW; w++) uw += __popc(m[w]);
    if (uw < (u32)P::W) {
        atomicAdd((u32 *)(smem + uw * (P::HROW * 4) + hbase), hinc);
    } else {
        sib_record<P>(uw + P::W0, j, i, a, outl, cutoff, out);
    }
}

// An out-of-window count u of sibling j's number at step i: the workgroup's
// out-of-window bin and, above the cutoff, the near-miss list.
template <class P>
__device__ __forceinline__ void sib_record(u32 u, int j, u32 i, const Fd2Args &a, u32 *outl, u32 cutoff,
                                           const NumOut &out) {
    {
        atomicAdd(&outl[u], 1u);
        if (u > cutoff) {
            const SibUnit su = sib_unit<P>(a);
            u64 lo = su.lo, hi = su.hi;
            // i opaque here: otherwise the compiler strength-reduces su.lo +
            // j B^2 + i into three 64-bit induction variables stepped on
            // every step of the walk for this once-in-1e8 branch
            u32 ii = i;
            asm volatile("" : "+v"(ii));
            add_u128(lo, hi, (u64)j * ((u64)P::B * P::B) + ii);
            u32 pos = atomicAdd(out.count, 1u);
            if (pos < out.cap) {
                out.n[2 * (u64)pos] = lo;
                out.n[2 * (u64)pos + 1] = hi;
                out.u[pos] = u;
            }
        }
    }
}

// walk_sib, pipelined (Cfg::LG >= 100): a step issues the shared lookups and
// sibling 0's, computes the shared limb's carries (they need only the
// low-digit entry) while those are in flight, issues sibling 1's, and then
// per sibling j: consumes its lookups, counts its number, steps its upper
// limbs and issues sibling j + 2's.  Two siblings' lookups are in flight
// while the VALU works, so the lookups' latency hides behind arithmetic at 4
// waves per SIMD (scheduling barriers pin the order).
template <class P>
__device__ __forceinline__ void walk_sib_pipe(State<P> (&st)[P::SIB], const unsigned char *smem, const Fd2Args &a,
                                              u32 chunk, u32 hbase, u32 hinc, u32 *outl, u32 cutoff,
                                              const NumOut &out) {
    constexpr int L = P::LO;
    constexpr int M = P::SIB;
#pragma unroll
    for (int j = 0; j < M; j++) sib_hi<P>(st[j], j, smem);
    for (u32 i = 0; i < chunk; i++) {
        SibLook<P> e[M];
        // shared lookups (limb 0 of S and C, limb L of S and C) and sibling 0's
        const uint2 vlo = *(const uint2 *)(smem + P::TL + st[0].r8);
        uint2 vs, vc;
        u32 mv[P::MW] = {};
        if (P::vd_s(L)) or_valu<P>(st[0].S[L] - P::EBT, mv);
        else vs = *(const uint2 *)(smem + (P::TB - (int)P::EBT) + st[0].S[L]);
        if (P::vd_c(L)) or_valu<P>(st[0].C[L], mv);
        else vc = *(const uint2 *)(smem + P::TB + st[0].C[L]);
        sib_issue<P>(st[0], smem, e[0]);
        __builtin_amdgcn_sched_barrier(0);
        // the shared limb's step (needs only the low-digit entry's carries)
        const u32 w1 = vlo.y;
        u32 cC, cS;
        bool any;
        sib_shared_step<P>(st[0], w1, cC, cS, any);
        if (M > 1) sib_issue<P>(st[1], smem, e[1]);
        __builtin_amdgcn_sched_barrier(0);
        u32 m0[P::MW];
        bool topS[M], topC[M];
#pragma unroll
        for (int j = 0; j < M; j++) {
            if (j == 0) {
                m0[0] = vlo.x | mv[0] | (P::vd_s(L) ? 0u : vs.x) | (P::vd_c(L) ? 0u : vc.x);
                m0[1] = (vlo.y & P::DMASK) | mv[1] | (P::vd_s(L) ? 0u : vs.y) | (P::vd_c(L) ? 0u : vc.y);
            }
            u32 m[P::MW];
#pragma unroll
            for (int w = 0; w < P::MW; w++) m[w] = m0[w] | st[j].hi[w];
            sib_consume<P>(st[j], e[j], m);
            // probe 16 (wrong by design): no window count, the mask feeds a
            // register sum instead
            if constexpr ((P::PROBE & 16) != 0) {
                any |= (m[0] ^ m[1]) == 0x5a5a5a5au;
            } else {
                sib_count<P>(m, j, i, smem, a, hbase, hinc, outl, cutoff, out);
            }
            any |= sib_upper_step<P>(st[j], cC, cS, topS[j], topC[j]);
            if (j + 2 < M) sib_issue<P>(st[j + 2], smem, e[j + 2]);
            __builtin_amdgcn_sched_barrier(0);
        }
        // probe 8 (wrong by design): the rare path never runs
        if ((P::PROBE & 8) == 0 && any) rare_sib<P>(st, smem, topS, topC);
    }
}

template <class P>
__device__ __forceinline__ void walk_sib(State<P> (&st)[P::SIB], const unsigned char *smem, const Fd2Args &a,
                                         u32 chunk, u32 hbase, u32 hinc, u32 *outl, u32 cutoff, const NumOut &out) {
    if constexpr (P::LG >= 100) {
        walk_sib_pipe<P>(st, smem, a, chunk, hbase, hinc, outl, cutoff, out);
        return;
    }
    constexpr int L = P::LO;
#pragma unroll
    for (int j = 0; j < P::SIB; j++) sib_hi<P>(st[j], j, smem);
    const u32 r80 = st[0].r8;
    for (u32 i = 0; i < chunk; i++) {
        // shared: limb 0 of S and C (low-digit entry) and limb 1 of both
        u32 m0[P::MW];
        const uint2 v = *(const uint2 *)(smem + P::TL + st[0].r8);
        const u32 w1 = v.y;
        m0[0] = v.x;
        m0[1] = v.y & P::DMASK;
        or_limb<P>(st[0], smem, true, L, m0);
        or_limb<P>(st[0], smem, false, L, m0);
#pragma unroll
        for (int j = 0; j < P::SIB; j++) {
            u32 m[P::MW];
#pragma unroll
            for (int w = 0; w < P::MW; w++) m[w] = m0[w] | st[j].hi[w];
#pragma unroll
            for (int q = L + 1; q < P::SL; q++) {
                or_limb<P>(st[j], smem, true, q, m);
                if (P::LG > 1 && (q - L) % P::LG == 0) lookup_group_end<P>(m);
            }
#pragma unroll
            for (int q = L + 1; q < P::CL; q++) {
                or_limb<P>(st[j], smem, false, q, m);
                if (P::LG > 1 && (P::SL - L - 1 + q - L) % P::LG == 0) lookup_group_end<P>(m);
            }
            // a group per sibling: its loaded words are dead before the next
            // sibling's lookups issue (bounds the VGPRs in flight)
            if (P::LG) lookup_group_end<P>(m);
            u32 uw = bcnt_acc(m[0], (u32)(-P::W0));
#pragma unroll
            for (int w = 1; w < P::MW; w++) uw += __popc(m[w]);
            if (uw < (u32)P::W) {
                atomicAdd((u32 *)(smem + uw * (P::HROW * 4) + hbase), hinc);
            } else {
                const u32 u = uw + P::W0;
                atomicAdd(&outl[u], 1u);
                if (u > cutoff) {
                    const SibUnit su = sib_unit<P>(a);
                    u64 lo = su.lo, hi = su.hi;
                    add_u128(lo, hi, (u64)j * ((u64)P::B * P::B) + (st[0].r8 - r80) / P::ES);
                    u32 pos = atomicAdd(out.count, 1u);
                    if (pos < out.cap) {
                        out.n[2 * (u64)pos] = lo;
                        out.n[2 * (u64)pos + 1] = hi;
                        out.u[pos] = u;
                    }
                }
            }
        }
        step_sib<P>(st, smem, w1);
    }
}

// fd2_batch_kernel's copies of fd2_body's first and last steps.  fd2_body keeps
// its own text: with these two called from it instead, every fd2_kernel kept
// its resource line but 6 369 instructions across the 131 instantiations came
// out in another order (scripts/isa/kernel_diff.py), and the field kernels'
// generated code is not to move for a feature they do not use.  (Tried again
// when the header was split four ways: the same 131 of 586 product kernels
// differ, same instruction counts, another order.)  Keep the two in step with
// fd2_body.
//
// A workgroup's start: the table image DMA'd into LDS and the histogram
// region zeroed (see fd2_body).
template <class P>
__device__ __forceinline__ void fd2_load_tables(unsigned char *smem, const uint4 *tabs, u32 tid) {
    constexpr u32 N16 = (u32)(P::TAB_BYTES / 16);
    const u32 lane = tid & 63, w64 = tid & ~63u;
    for (u32 i0 = w64; i0 < N16; i0 += P::WG)
        if (i0 + lane < N16)
            __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void *)(tabs + i0 + lane),
                                             (__attribute__((address_space(3))) void *)(smem + P::TC0 + 16 * i0),
                                             16, 0, 0);
    uint4 *h4 = (uint4 *)smem;
    for (u32 i = tid; i < (u32)(P::ZA / 16); i += P::WG) h4[i] = make_uint4(0, 0, 0, 0);
    if constexpr (P::SPLIT)
        for (u32 i = tid; i < (u32)(P::HIST_BYTES / 16); i += P::WG)
            h4[P::HB / 16 + i] = make_uint4(0, 0, 0, 0);
}

// A workgroup's end (after the barrier that follows its steps): the window
// rows reduced and, with the out-of-window bins, added to row `row` (kHistBins bins
// apart) of hist_rows.
template <class P>
__device__ __forceinline__ void fd2_flush(const unsigned char *smem, u64 *hist_rows, u32 row_out, u32 tid) {
    const u32 *hist = (const u32 *)(smem + P::HB);
    const u32 *outl = (const u32 *)(smem + P::OUTL);
    const u32 lane = tid & 63, wave = tid >> 6;
    u64 *hist_out = hist_rows + row_out * kHistBins;
    // Window rows: wave w sums rows w, w + WG/64, ...; all of a wave's rows
    // are read and reduced together, so their cross-lane steps overlap.
    constexpr u32 NWAVE = P::WG / 64, RPW = (P::W + NWAVE - 1) / NWAVE;
    u32 rs[RPW];
#pragma unroll
    for (u32 k = 0; k < RPW; k++) {
        const u32 row = wave + k * NWAVE;
        u32 s = 0;
        if (row < (u32)P::W) {
#pragma unroll
            for (int q = 0; q < P::HROW / 64; q++) {
                const u32 v = hist[row * P::HROW + lane + 64 * q];
                if constexpr (P::HQ == 2) s += (v & 0xffffu) + (v >> 16);
                else s += (v & 0xffu) + ((v >> 8) & 0xffu) + ((v >> 16) & 0xffu) + (v >> 24);
            }
        }
        rs[k] = s;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
        for (u32 k = 0; k < RPW; k++) rs[k] += __shfl_xor(rs[k], o);
#pragma unroll
    for (u32 k = 0; k < RPW; k++) {
        const u32 row = wave + k * NWAVE;
        if (lane == 0 && row < (u32)P::W && rs[k])
            atomicAdd((unsigned long long *)&hist_out[P::W0 + row], (unsigned long long)rs[k]);
    }
    if (tid < (u32)P::NBINS && outl[tid])
        atomicAdd((unsigned long long *)&hist_out[tid], (unsigned long long)outl[tid]);
}

// Persistent grid: batch b of the launch (64 lanes' units) -> this lane's
// unit: b < mb: main unit 64 b + lane (chunk a.chunk from a.start); else the
// tail numbers 64 (b - mb) + lane (chunk 1 from a.tail).
__device__ __forceinline__ void pers_unit(const Fd2Args &a, u32 b, u32 mb, u32 lane, bool &active, u64 &lo,
                                          u64 &hi, u32 &chunk) {
    if (b < mb) {
        const u32 unit = 64 * b + lane;
        active = unit < a.nunits;
        lo = a.start_lo;
        hi = a.start_hi;
        add_u128(lo, hi, (u64)unit * a.chunk);
        chunk = a.chunk;
    } else {
        const u32 idx = 64 * (b - mb) + lane;
        active = idx < a.tail_count;
        lo = a.tail_lo;
        hi = a.tail_hi;
        add_u128(lo, hi, (u64)idx);
        chunk = 1;
    }
}

template <class P>
__device__ __forceinline__ void fd2_body(const Fd2Args &a) {
    // Static LDS: its address is a compile-time constant, so a lookup is one
    // ds_read with the table offset in the instruction's immediate field.
    __shared__ __attribute__((aligned(16))) unsigned char smem[P::LDS_BYTES];
    u32 *hist = (u32 *)(smem + P::HB);
    u32 *outl = (u32 *)(smem + P::OUTL);
    const u32 tid = threadIdx.x;
    const NumOut out = a.out;
    const u32 cutoff = a.cutoff;
    // sibling parts (Cfg::SIB), then the main part and the tail part of the
    // launch (workgroup-uniform)
    const u32 sib_end = P::SIB > 1 ? a.sib_blocks + a.edge_blocks : 0u;
    const bool sib_part = P::SIB > 1 && blockIdx.x < sib_end;
    const u32 bid = blockIdx.x - sib_end;
    const bool main_part = bid < a.main_blocks;
    const u64 start_lo = main_part ? a.start_lo : a.tail_lo;
    const u64 start_hi = main_part ? a.start_hi : a.tail_hi;
    const u32 nunits = main_part ? a.nunits : a.tail_count;
    const u32 chunk = main_part ? a.chunk : 1u;
    const u32 blk = main_part ? bid : bid - a.main_blocks;
    FD2_STAMP(a, 0);  // start

    // The tables (built once per device and base in global memory,
    // fd2_tables, fd2_launch.hpp) are DMA'd into LDS, and the histogram region zeroed:
    // building them here cost ~5 % of a launch of short chunks.  One
    // global_load_lds_dwordx4 wave-instruction moves 1 KiB (lane l's 16 bytes
    // land at the wave-uniform base + 16 l): every load of the copy is in
    // flight at once, with no VGPR round trip and no ds_write (the register
    // copy it replaces waited one L2 round trip per 16 bytes a lane moved:
    // b40 1e6 spent 2.1 us of a 12.5 us kernel in it, fd2_stamps_before.log).
    {
        constexpr u32 N16 = (u32)(P::TAB_BYTES / 16);
        const u32 lane = tid & 63, w64 = tid & ~63u;
        for (u32 i0 = w64; i0 < N16; i0 += P::WG)
            if (i0 + lane < N16)
                __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void *)(a.tabs + i0 + lane),
                                                 (__attribute__((address_space(3))) void *)(smem + P::TC0 + 16 * i0),
                                                 16, 0, 0);
        uint4 *h4 = (uint4 *)smem;
        for (u32 i = tid; i < (u32)(P::ZA / 16); i += P::WG) h4[i] = make_uint4(0, 0, 0, 0);
        if constexpr (P::SPLIT)
            for (u32 i = tid; i < (u32)(P::HIST_BYTES / 16); i += P::WG)
                h4[P::HB / 16 + i] = make_uint4(0, 0, 0, 0);
    }
    // A lane's first chunk (without PERS its only one: plan_regular sizes the
    // grid to cover every unit) is set up while the table DMA is in flight;
    // only the cached high limbs' mask needs the tables.
    const u32 lane_id = tid & 63;
    u32 unit = blk * P::WG + tid;
    bool active = unit < nunits;
    u64 n0_lo = start_lo, n0_hi = start_hi;
    u32 chunk_l = chunk;
    // persistent grid: this workgroup's batches are b = blockIdx + G k, k <
    // pnk, of the launch's nb = mb main + tail batches (strided, so every
    // workgroup samples the whole field: contiguous slabs were up to 40 %
    // slower on some n-ranges, profiles/r03/fd2_stamps_pers.log), and the
    // next k to hand out
    __shared__ u32 pers_next;
    u32 pmb = 0, pnk = 0, pk = 0;
    u64 n0_off = 0;          // n0 - the part's first n (init_at)
    const bool n0_tail = !main_part;
    if constexpr (P::PERS) {
        pmb = (a.nunits + 63) / 64;
        const u32 nb = pmb + (a.tail_count + 63) / 64, G = gridDim.x;
        pnk = nb > blockIdx.x ? (nb - blockIdx.x + G - 1) / G : 0;
        pk = tid >> 6;
        if (tid == 0) pers_next = P::WG / 64;
        if (pk < pnk) pers_unit(a, blockIdx.x + G * pk, pmb, lane_id, active, n0_lo, n0_hi, chunk_l);
        else active = false;
    } else {
        n0_off = (u64)unit * chunk;
        add_u128(n0_lo, n0_hi, n0_off);
    }
    // Window counters: row u - W0, column tid mod HROW (u16 halves / u8 quarters).
    const u32 hbase = P::HB + tid % P::HROW * 4;
    // (HROW is a multiple of 64: the increment is wave-uniform, an SGPR)
    static_assert(P::HROW % 64 == 0, "window row of whole waves");
    const u32 hinc = __builtin_amdgcn_readfirstlane(1u << (32 / P::HQ * (tid / P::HROW)));
    u32 probe_acc = 0;
    // Sibling lanes (workgroup-uniform): the sibling state is built, waited
    // for and walked on its own path, so its registers never overlap the
    // regular path's (one State live at the barrier, not M + 1).
    bool sib_done = false;
    if constexpr (P::SIB > 1) {
        if constexpr (P::SIBPERS) {
            // Persistent sibling grid: the a.sib_blocks workgroups of the
            // sibling part are one round of resident ones.  Workgroup g owns
            // the batches g + G k, k < nk, of the launch's sibling and edge
            // batches (strided, as the regular persistent grid's); after the
            // one barrier its waves take k = wave, then pull the next k from
            // an LDS counter, until the batches run out or a wave has taken
            // wave_cap of them (its lanes' u16 window counters hold
            // wave_cap M L numbers; the host sizes launches so the waves'
            // caps cover every workgroup's batches).  Every loop bound is the
            // host's: no workgroup waits for another.
            if (sib_part) {
                __shared__ u32 sib_next;
                const u32 G = a.sib_blocks;
                const u32 nb = (a.sib_units + 63) / 64 + (a.edge_units + 63) / 64;
                const u32 nk = nb > blockIdx.x ? (nb - blockIdx.x + G - 1) / G : 0;
                if (tid == 0) sib_next = P::WG / 64;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                FD2_STAMP(a, 14);
                u32 k = __builtin_amdgcn_readfirstlane(tid >> 6), taken = 0;
                while (k < nk) {
                    const u32 b = blockIdx.x + G * k;
                    if (lane_id == 0) *sib_batch_slot<P>() = b;
                    const SibUnit su = sib_unit_at<P>(a, b, lane_id);
                    if (su.active) {
                        State<P> sst[P::SIB];
                        u32 X[P::NX];
                        init_digits<P>(X, su.lo, su.hi);
                        init_plain<P>(sst[0], X);
#pragma unroll
                        for (int j = 1; j < P::SIB; j++) sib_derive<P>(sst[j], sst[0], X, (u32)j);
#pragma unroll
                        for (int j = 0; j < P::SIB; j++) {
                            init_scale<P>(sst[j]);
                            sib_park<P>(sst[j], j, smem);
                        }
                        walk_sib<P>(sst, smem, a, su.chunk, hbase, hinc, outl, cutoff, out);
                    }
                    if (++taken >= a.wave_cap) break;
                    u32 next = 0;
                    if (lane_id == 0) next = atomicAdd(&sib_next, 1u);
                    k = __builtin_amdgcn_readfirstlane(__shfl(next, 0));
                }
                FD2_STAMP(a, 15);
                FD2_WAVE_STAMP(a);
                sib_done = true;
            }
        } else if (sib_part) {
            State<P> sst[P::SIB];
            const SibUnit su = sib_unit<P>(a);
            if (su.active) {
                u32 X[P::NX];
                init_digits<P>(X, su.lo, su.hi);
                init_plain<P>(sst[0], X);
#pragma unroll
                for (int j = 1; j < P::SIB; j++) sib_derive<P>(sst[j], sst[0], X, (u32)j);
#pragma unroll
                for (int j = 0; j < P::SIB; j++) {
                    init_scale<P>(sst[j]);
                    sib_park<P>(sst[j], j, smem);
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            FD2_STAMP(a, 14);  // sibling part: state built, tables in LDS
            if (su.active) walk_sib<P>(sst, smem, a, su.chunk, hbase, hinc, outl, cutoff, out);
            FD2_STAMP(a, 15);  // sibling part: thread 0's steps done
            FD2_WAVE_STAMP(a);
            sib_done = true;
        }
    }
    State<P> st;
    // (the persistent grid runs only on the 1024-thread kernels, which keep
    // init(): C64)
    if constexpr (P::PERS || P::N64 || P::C64) {
        if (!sib_done && active) init<P>(st, n0_lo, n0_hi);
    } else {
        if (!sib_done && active) init_at<P>(st, n0_tail ? a.xt : a.xs, n0_off, n0_lo, n0_hi);
    }
    // The table DMA must have landed before any wave reads LDS: wait for it
    // explicitly (a workgroup barrier alone need not imply vmcnt(0)), then
    // the barrier.
    if (!sib_done) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    FD2_STAMP(a, 1);  // state built, tables in LDS
    FD2_STAMP(a, 2);  // (the cached mask is built inside walk_chunk)
    if constexpr (P::SIB > 1) {
        if (!sib_done && active)
            walk_chunk<P>(st, smem, chunk, n0_lo, n0_hi, hbase, hinc, outl, cutoff, out, probe_acc);
    } else if constexpr (!P::PERS) {
        if (active) {
            walk_chunk<P>(st, smem, chunk, n0_lo, n0_hi, hbase, hinc, outl, cutoff, out, probe_acc);
        }
    } else {
        // Persistent grid: wave w starts on this workgroup's batch k = w (its
        // state is already built), then pulls the next k from the LDS counter
        // until the workgroup's batches are exhausted or the wave has taken
        // wave_cap of them (its lanes' u16 counters hold them; the host sizes
        // launches so the waves' caps cover the workgroup's batches).
        u32 k = pk, taken = 0;
        bool act = active;
        u64 m_lo = n0_lo, m_hi = n0_hi;
        u32 ch = chunk_l;
        while (k < pnk) {
            if (taken) {
                pers_unit(a, blockIdx.x + gridDim.x * k, pmb, lane_id, act, m_lo, m_hi, ch);
                if (act) init<P>(st, m_lo, m_hi);
            }
            if (act) walk_chunk<P>(st, smem, ch, m_lo, m_hi, hbase, hinc, outl, cutoff, out, probe_acc);
            if (++taken >= a.wave_cap) break;
            u32 nk = 0;
            if (lane_id == 0) nk = atomicAdd(&pers_next, 1u);
            k = __builtin_amdgcn_readfirstlane(__shfl(nk, 0));
        }
    }
    if constexpr ((P::PROBE & 2) != 0) atomicAdd(&outl[P::W0], probe_acc);  // mass only
    FD2_STAMP(a, 3);  // thread 0's steps done
    __syncthreads();
    FD2_STAMP(a, 4);  // every wave's steps done
    const u32 lane = tid & 63, wave = tid >> 6;
    u64 *hist_out = a.hist + (blockIdx.x % a.ncopies) * kHistBins;
    // Window rows: wave w sums rows w, w + WG/64, ...; all of a wave's rows
    // are read and reduced together, so their cross-lane steps overlap.
    constexpr u32 NWAVE = P::WG / 64, RPW = (P::W + NWAVE - 1) / NWAVE;
    u32 rs[RPW];
#pragma unroll
    for (u32 k = 0; k < RPW; k++) {
        const u32 row = wave + k * NWAVE;
        u32 s = 0;
        if (row < (u32)P::W) {
#pragma unroll
            for (int q = 0; q < P::HROW / 64; q++) {
                const u32 v = hist[row * P::HROW + lane + 64 * q];
                if constexpr (P::HQ == 2) s += (v & 0xffffu) + (v >> 16);
                else s += (v & 0xffu) + ((v >> 8) & 0xffu) + ((v >> 16) & 0xffu) + (v >> 24);
            }
        }
        rs[k] = s;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
        for (u32 k = 0; k < RPW; k++) rs[k] += __shfl_xor(rs[k], o);
#pragma unroll
    for (u32 k = 0; k < RPW; k++) {
        const u32 row = wave + k * NWAVE;
        if (lane == 0 && row < (u32)P::W && rs[k])
            atomicAdd((unsigned long long *)&hist_out[P::W0 + row], (unsigned long long)rs[k]);
    }
    if (tid < (u32)P::NBINS && outl[tid])
        atomicAdd((unsigned long long *)&hist_out[tid], (unsigned long long)outl[tid]);
    FD2_STAMP(a, 5);  // histogram flushed (thread 0's part)
    if (a.fin.out_mapped) {
        __syncthreads();  // smem is reused by the finish
        field_finish<P::WG>(a.fin, a.hist, a.ncopies, P::NBINS, out.count, smem, a.stamps);
    }
    FD2_STAMP(a, 6);  // end (the finishing workgroup: after the finish)
}

template <class P>
__global__ void __launch_bounds__(P::WG) __attribute__((amdgpu_waves_per_eu(P::WPE, P::WPE)))
fd2_kernel(Fd2Args a) {
    fd2_body<P>(a);
}

// ---------------------------------------------------------------------------
// Batched ranges: one grid whose workgroups belong to different ranges.
// Workgroup blockIdx.x reads ONE descriptor (wave-uniform: scalar loads, every
// walk parameter stays in SGPRs as in fd2_body) and runs the same device code
// -- table DMA, init / init_at, walk_chunk, the window-row reduction and the
// out-of-window bins -- over lanes x chunk numbers from its first n, then
// flushes into its range's own histogram row (or, sum mode, into copy
// blockIdx.x % ncopies as single fields do).  Near-misses go to the launch's
// shared NumOut.  No in-kernel finish (a batch has no single result row to
// publish; the host reads the rows back), no sibling lanes, no persistent grid:
// rounds of workgroups, the configuration small fields run.
// ---------------------------------------------------------------------------
constexpr int kXDigits = 12;  // Fd2Args::xs / Fd2Unit::xs (>= NX of every FD base)
struct Fd2Unit {
    u64 lo, hi;   // first n
    u32 lanes;    // active lanes (<= WG)
    u32 chunk;    // numbers per lane (<= B); 1 for a tail workgroup
    u32 row;      // result row (per-range mode)
    u32 pad;
    u32 xs[kXDigits];  // radix-B digits of the first n (init_at; bases whose n passes 64 bits)
};
static_assert(sizeof(Fd2Unit) == 80, "descriptor layout");

struct Fd2BatchArgs {
    const Fd2Unit *units;  // one per workgroup
    u64 *hist;             // rows of kHistBins bins
    u32 ncopies;           // 0: row = the descriptor's; else blockIdx.x % ncopies (sum mode)
    u32 cutoff;
    NumOut out;
    const uint4 *tabs;
};

template <class P>
__global__ void __launch_bounds__(P::WG) __attribute__((amdgpu_waves_per_eu(P::WPE, P::WPE)))
fd2_batch_kernel(Fd2BatchArgs a) {
    static_assert(!P::PERS && P::SIB == 1 && P::PROBE == 0, "batch kernel: rounds, regular lanes");
    static_assert(!(P::MW == 3 && P::WG >= 1024) && P::LGW == 0, "BatchCfg spells out the default lookup groups");
    __shared__ __attribute__((aligned(16))) unsigned char smem[P::LDS_BYTES];
    u32 *outl = (u32 *)(smem + P::OUTL);
    const u32 tid = threadIdx.x;
    // The descriptor, indexed by blockIdx.x only: read before anything is
    // written, so the loads are scalar.
    const Fd2Unit *__restrict__ d = a.units + blockIdx.x;
    const u64 start_lo = d->lo, start_hi = d->hi;
    const u32 lanes = d->lanes, chunk = d->chunk;
    const u32 row = a.ncopies ? blockIdx.x % a.ncopies : d->row;
    u32 xs[P::NX];
    if constexpr (!P::N64 && !P::C64) {
#pragma unroll
        for (int i = 0; i < P::NX; i++) xs[i] = d->xs[i];
    }
    const NumOut out = a.out;
    const u32 cutoff = a.cutoff;
    fd2_load_tables<P>(smem, a.tabs, tid);
    const bool active = tid < lanes;
    const u64 n0_off = (u64)tid * chunk;
    u64 n0_lo = start_lo, n0_hi = start_hi;
    add_u128(n0_lo, n0_hi, n0_off);
    const u32 hbase = P::HB + tid % P::HROW * 4;
    const u32 hinc = __builtin_amdgcn_readfirstlane(1u << (32 / P::HQ * (tid / P::HROW)));
    u32 probe_acc = 0;
    State<P> st;
    if constexpr (P::N64 || P::C64) {
        if (active) init<P>(st, n0_lo, n0_hi);
    } else {
        if (active) init_at<P>(st, xs, n0_off, n0_lo, n0_hi);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (active) walk_chunk<P>(st, smem, chunk, n0_lo, n0_hi, hbase, hinc, outl, cutoff, out, probe_acc);
    __syncthreads();
    fd2_flush<P>(smem, a.hist, row, tid);  // row < 2^14 rows of a pass: row * kHistBins fits 32 bits
}

}  // namespace fd2
}  // namespace nice
