// niceonly_bases.h -- the ONE list of niceonly fast bases: every base with an
// FD kernel (fd2_combos.h FD2_BASES) whose k = 2 stride table has at least one
// residue.  (43, 47, 55, 59, 63 and 67 have an empty residue filter: their
// niceonly fields return an empty list before any kernel runs.)
//
// Everything with a per-base compile-time niceonly path dispatches from it:
//   * the device kernels (niceonly_cand.hpp, niceonly_msd.hpp and
//     niceonly_wave.hpp, instantiated per part in
//     niceonly_part.hip: ConstBase divisors, radix_fast.hpp's in-range limb
//     paths, the square-survivor queue, the LDS pair table, the lane walk);
//   * the ABI hooks (abi_hooks.cpp) and nice_niceonly_fast_base
//     (abi_context.cpp);
//   * the host paths' compile-time divisors (cpu_path.cpp with_base,
//     host_math.hpp make_msd).
// tests/test_niceonly_bases.py checks the list against its definition.
//
// The list is written as NICEONLY_NPARTS part lists: part k's bases are
// instantiated by the object built from niceonly_part.hip with
// -DNICEONLY_PART=k, so the ~90 kernel instantiations compile in parallel
// (the heavy ones -- the three-word bases and b62 / b64 -- one per part).
// Taking a base out of the fast path is deleting its X(b) here.
#pragma once

#include <stdint.h>

#define NICEONLY_NPARTS 6
#define NICE_NICEONLY_PART0(X) X(40) X(57) X(65)
#define NICE_NICEONLY_PART1(X) X(42) X(58) X(68)
#define NICE_NICEONLY_PART2(X) X(44) X(60) X(80)
#define NICE_NICEONLY_PART3(X) X(45) X(50) X(62)
#define NICE_NICEONLY_PART4(X) X(48) X(52) X(64)
#define NICE_NICEONLY_PART5(X) X(49) X(53) X(54)

#define NICE_NICEONLY_BASES(X)                                                                   \
    NICE_NICEONLY_PART0(X) NICE_NICEONLY_PART1(X) NICE_NICEONLY_PART2(X) NICE_NICEONLY_PART3(X) \
    NICE_NICEONLY_PART4(X) NICE_NICEONLY_PART5(X)

namespace nice {

inline bool niceonly_fast_base(uint32_t base) {
    switch (base) {
#define X(b) case b:
        NICE_NICEONLY_BASES(X)
#undef X
        return true;
    default: return false;
    }
}

}  // namespace nice
