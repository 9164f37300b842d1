// niceonly_ranges_part.hip -- niceonly_ranges_kernel of the fast bases, one
// object per part (built with -DNICEONLY_PART=k, k < NICEONLY_NPARTS) over the
// same part lists as niceonly_part.hip (niceonly_bases.h), so they compile in
// parallel and the field kernels' objects stay as they are.  Beside each base's
// kernel: its prefix-testing variant and its range_mask_kernel.
#include "niceonly_bases.h"
#include "niceonly_ranges.hpp"

#ifndef NICEONLY_PART
#error "build with -DNICEONLY_PART=k"
#endif

#define NICEONLY_CAT2(a, b) a##b
#define NICEONLY_CAT(a, b) NICEONLY_CAT2(a, b)
#define NICEONLY_PART_BASES NICEONLY_CAT(NICE_NICEONLY_PART, NICEONLY_PART)

namespace nice {

template <int B>
hipError_t RangesBaseLaunch<B>::nice(const NiceRangesLaunch &rl, int num_cus, hipStream_t s) {
    return launch_nice_ranges(rl, ConstBase<B>{}, num_cus, s);
}
template <int B>
hipError_t RangesBaseLaunch<B>::nice_prefix(const NiceRangesLaunch &rl, const RangesPrefixLaunch &pre, int num_cus,
                                            hipStream_t s) {
    return launch_nice_ranges(rl, ConstBase<B>{}, num_cus, s, pre);
}
template <int B>
hipError_t RangesBaseLaunch<B>::masks(const RangeSpan *spans, u32 n, LeafMask *out, hipStream_t s) {
    hipLaunchKernelGGL((range_mask_kernel<B>), dim3((n + 255) / 256), dim3(256), 0, s, spans, n, out);
    return hipGetLastError();
}

#define X(b) template struct RangesBaseLaunch<b>;
NICEONLY_PART_BASES(X)
#undef X

}  // namespace nice
