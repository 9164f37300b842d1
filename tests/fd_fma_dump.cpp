// fd_fma_dump.cpp -- the FD step's f32-pipe limb arithmetic (Cfg::FMA,
// fma_bits in nice_amd/csrc/fd2_kernel.hpp) evaluated on the host for
// tests/test_fd_fma_exact.py.  Host-only, built with a plain C++17 compiler
// and no fast-math from fd2_cfg.hpp; instantiating every configuration with
// the flag on is itself the check of Cfg's static_asserts on the operand
// bounds.
//
// fb(a, K, c) is what v_fma_f32 returns for the bit patterns a and c and the
// float K: fmaf on the patterns (the host keeps subnormals unless told
// otherwise).  Every form below is the kernel's, in the kernel's order, next
// to the integer expression it replaces.
//
// stdout, one line per (base, ND, NE, NE2) of fd2_combos.h:
//   F base nd ne ne2 es  bad_t1 bad_red bad_s bad_top bad_chain
//     max_t1 max_t max_ts   lim_t1 lim_t lim_ts  bad_wrong
// bad_*: mismatches of a form against its integer expression; max_*: the
// largest operand or result seen per form; lim_*: Cfg's compile-time bounds;
// bad_wrong: the control -- the same limbs with the offset N3 term added to C
// BEFORE the carry's FMA, where the wrapped sum is a NaN pattern: it must be
// non-zero, or the comparison would prove nothing.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "fd2_cfg.hpp"
#include "fd2_combos.h"

using namespace nice;
using namespace nice::fd2;

typedef unsigned long long ull;

static inline float as_f(u32 x) {
    float f;
    memcpy(&f, &x, 4);
    return f;
}
static inline u32 fb(u32 a, float k, u32 c) {
    const float r = fmaf(as_f(a), k, as_f(c));
    u32 x;
    memcpy(&x, &r, 4);
    return x;
}
static inline u32 mulhi(u32 a, u32 b) { return (u32)(((ull)a * b) >> 32); }

template <class P>
static u32 carry_of(u32 t) {
    return P::C1 ? mulhi(t, P::MAGIC) : mulhi(t / P::ES, P::MAGICB);
}

// One C limb, f32 order: returns the new limb, the unscaled carry in cout.
// n3 is the stored N3 limb (offset by -3 ES BT, so possibly wrapped) or, for a
// limb past N3, the wrapped constant -3 ES BT.
template <class P>
static u32 c_limb_fma(u32 C, u32 S, u32 n3, u32 c, u32 &cout, ull &m1, ull &mt) {
    const u32 t1 = fb(c, (float)P::ES, C);
    const u32 t = S * 3 + (t1 + n3);  // integers (v_mad_u32_u24's addend is 32 bits): may wrap on the way
    if (t1 > m1) m1 = t1;
    if (t > mt) mt = t;
    cout = carry_of<P>(t);
    return fb(cout, -(float)P::DC, t);
}
// ... and the integer order (scaled carry in, N3 first).
template <class P>
static u32 c_limb_int(u32 C, u32 S, u32 n3, u32 c, u32 &cout) {
    u32 t = C + c * P::ES;
    t += n3;
    t = S * 3 + t;
    cout = carry_of<P>(t);
    return t - cout * P::DC;
}

template <class P>
static void run() {
    static_assert(P::FMA, "the flag under test");
    constexpr u32 ES = P::ES, B = P::B, DC = P::DC;
    const float fES = (float)ES, fDC = -(float)DC;
    ull bad_t1 = 0, bad_red = 0, bad_s = 0, bad_top = 0, bad_chain = 0;
    ull m1 = 0, mt = 0, ms = 0, bad_wrong = 0;
    // t1 = ES c + C over every scaled limb value up to the unreduced top limb's
    // (also the top limb's own carry add)
    for (u32 c = 0; c <= 4; c++)
        for (u32 C = 0; C <= DC + 4 * ES; C += ES) {
            const u32 r = fb(c, fES, C);
            bad_t1 += r != ES * c + C;
            if (r > m1) m1 = r;
        }
    // the reduction C = t - c DC, exhaustively over t = ES u, u <= 5B + 4, with
    // every c that leaves it non-negative (the step's c = t / DC among them)
    for (u32 u = 0; u <= 5 * B + 4; u++) {
        const u32 t = ES * u;
        if (t > mt) mt = t;
        bad_red += carry_of<P>(t) != t / DC;
        for (u32 c = 0; c <= 4 && c * DC <= t; c++) bad_red += fb(c, fDC, t) != t - c * DC;
    }
    // S limb: t = ES c + x (x = S + D1, both scaled), carry = bit SH alone,
    // S = t - carry DC, against the integer form's shift, mask and multiply
    for (u32 c = 0; c <= 1; c++)
        for (u32 x = 0; x + ES * c < (2u << P::SH); x += ES) {
            const u32 t = fb(c, fES, x);
            bad_s += t != x + ES * c;
            const u32 cy = t >> P::SH, cs = (t >> P::T) & ES;
            bad_s += cy * ES != cs || cy > 1;
            bad_s += fb(cy, fDC, t) != t - cs * B || (cy && t < DC);
            if (t > ms) ms = t;
        }
    // the top stepped limbs only take the carry: S up to its compare value
    for (u32 c = 0; c <= 1; c++)
        for (u32 S = 0; S <= (1u << P::SH); S += ES) bad_top += fb(c, fES, S) != S + ES * c;
    // whole C limbs in the step's order, with N3's stored limbs (offset by
    // -3 ES BT: wrapped below zero for small limbs) and the bare -3 ES BT
    // term: every S limb, the extreme C limbs, N3 limbs and carries
    for (u32 s = 0; s < B; s++)
        for (u32 C : {0u, DC - ES})
            for (u32 n : {0u, B - 1, ~0u})
                for (u32 c = 0; c <= 4; c++) {
                    const u32 S = (s + P::BT) * ES;
                    const u32 n3 = (n == ~0u ? 0u : n * ES) - 3 * P::EBT;
                    // in-range only: a C-limb sum is < 5B + 4 (cfg: TMAX)
                    if ((ull)C + c * ES + 3ull * s * ES + (n == ~0u ? 0u : n * ES) > P::TMAX) continue;
                    u32 c0, c1;
                    const u32 a = c_limb_fma<P>(C, S, n3, c, c1, m1, mt);
                    const u32 b = c_limb_int<P>(C, S, n3, c, c0);
                    bad_chain += a != b || c0 != c1 || a >= DC;
                    bad_wrong += fb(c, fES, C + n3) != C + n3 + c * ES;
                }
    printf("F %d %d %d %d %u  %llu %llu %llu %llu %llu  %llu %llu %llu  %llu %llu %llu  %llu\n", P::BASE, P::ND, P::NE,
           P::NE2, ES, bad_t1, bad_red, bad_s, bad_top, bad_chain, m1, mt, ms, (ull)P::FMA_T1, (ull)P::TMAX,
           (ull)P::FMA_TS, bad_wrong);
}

int main() {
    // the low-digit-table mode of the base (vd::SIDE) kept, as fd2_part.hip's
    // configurations keep it; the flag on
#define X(B_, ND_, NE_, NE2_) run<Cfg<B_, ND_, NE_, NE2_, 0, 512, (valu_limbs(B_) & vd::SIDE) | vd::FMA>>();
    FD2_COMBOS(X)
#undef X
    return 0;
}
