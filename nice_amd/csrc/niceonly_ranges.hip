// niceonly_ranges.hip -- batched niceonly ranges on gfx950: the entry point of
// kernels.h (launch_niceonly_ranges).  The kernel template is in
// niceonly_ranges.hpp; this object holds its run-time-base instantiation (any
// base 2..128, any n < 2^128) and the dispatch to the fast bases' compile-time
// instantiations, built a few bases per object from niceonly_ranges_part.hip.
#include "niceonly_bases.h"
#include "niceonly_ranges.hpp"

namespace nice {

hipError_t launch_niceonly_ranges(const NiceRangesLaunch &rl, int num_cus, hipStream_t s,
                                  const RangesPrefixLaunch *pre) {
    if (rl.n_leaves == 0) return hipSuccess;
    if (pre && !rl.c.in_range) return hipErrorInvalidValue;  // the run-time-base kernel has no variant
    if (rl.c.in_range) {
        switch (rl.c.base) {
#define X(b) case b: return pre ? RangesBaseLaunch<b>::nice_prefix(rl, *pre, num_cus, s) \
                                : RangesBaseLaunch<b>::nice(rl, num_cus, s);
            NICE_NICEONLY_BASES(X)
#undef X
        default: return hipErrorInvalidValue;  // no compile-time kernel: a missing kernel is an error
        }
    }
    return launch_nice_ranges(rl, make_generic(rl.c.base), num_cus, s);
}

hipError_t launch_range_masks(uint32_t base, const RangeSpan *spans, uint32_t n, LeafMask *masks, hipStream_t s) {
    if (n == 0) return hipSuccess;
    switch (base) {
#define X(b) case b: return RangesBaseLaunch<b>::masks(spans, n, masks, s);
        NICE_NICEONLY_BASES(X)
#undef X
    default: return hipErrorInvalidValue;
    }
}

}  // namespace nice
