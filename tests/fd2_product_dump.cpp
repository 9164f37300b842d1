// fd2_product_dump.cpp -- the FD kernels production can launch, for
// tests/test_fd2_product.py.  Host-only.  For every (base, combo) of
// fd2_combos.h: the selector's kernels (nice_amd/csrc/fd2_cfg.hpp: SmallCfg,
// BigCfg, BatchCfg) and everything the launchers reach from them (fd2_launch.hpp:
// NoSib from a sibling kernel, its persistent twin SibPers, NoPers from a
// persistent grid).  Instantiating them also evaluates every static_assert of
// Cfg on the CPU.
//
// stdout, one line per kernel (repeats included):
//   K base nd ne ne2 probe wg vd lg pers sib      an fd2_kernel<Cfg<...>>
//   B base nd ne ne2 probe wg vd lg pers sib      an fd2_batch_kernel<Cfg<...>>
#include <stdio.h>

#include "fd2_cfg.hpp"
#include "fd2_combos.h"

using namespace nice::fd2;

template <class P>
struct Args;
template <int B_, int ND_, int NE_, int NE2_, int PROBE_, int WG_, int VD_, int LG_, int PERS_, int SIB_>
struct Args<Cfg<B_, ND_, NE_, NE2_, PROBE_, WG_, VD_, LG_, PERS_, SIB_>> {
    static void print(char tag) {
        printf("%c %d %d %d %d %d %d %d %d %d %d\n", tag, B_, ND_, NE_, NE2_, PROBE_, WG_, VD_, LG_, PERS_, SIB_);
    }
};

// launch_cfg / launch_sib: P and what they fall back to.
template <class P>
static void reach() {
    static_assert(P::WPE >= 1, "a complete Cfg");
    Args<P>::print('K');
    if constexpr (P::SIB > 1) {
        reach<typename P::NoSib>();
        if constexpr (P::HAS_SIBPERS) {
            static_assert(P::SibPers::SIBPERS && P::SibPers::WPE >= 1, "a complete Cfg");
            Args<typename P::SibPers>::print('K');
        }
    } else if constexpr (P::PERS) {
        reach<typename P::NoPers>();
    }
}

int main() {
#define X(B_, ND_, NE_, NE2_)                                              \
    reach<SmallCfg<B_, ND_, NE_, NE2_>>();                                 \
    reach<BigCfg<B_, ND_, NE_, NE2_>>();                                   \
    static_assert(BatchCfg<B_, ND_, NE_, NE2_>::LDS_BYTES > 0, "complete"); \
    Args<BatchCfg<B_, ND_, NE_, NE2_>>::print('B');
    FD2_COMBOS(X)
#undef X
    return 0;
}
