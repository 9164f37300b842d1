// msd_ranges_part.hip -- msd_ranges_fused_kernel and msd_ranges_level_kernel of
// the fast bases under both filters, one object per part (built with
// -DNICEONLY_PART=k, k < NICEONLY_NPARTS) over the same part lists as
// niceonly_part.hip (niceonly_bases.h), so they compile in parallel and the
// field kernels' objects stay as they are.
#include "msd_ranges.hpp"
#include "niceonly_bases.h"

#ifndef NICEONLY_PART
#error "build with -DNICEONLY_PART=k"
#endif

#define NICEONLY_CAT2(a, b) a##b
#define NICEONLY_CAT(a, b) NICEONLY_CAT2(a, b)
#define NICEONLY_PART_BASES NICEONLY_CAT(NICE_NICEONLY_PART, NICEONLY_PART)

namespace nice {

template <int B>
hipError_t MsdRangesBaseLaunch<B>::group(const MsdRangesLaunch &p, bool sound, u64 max_size, int num_cus,
                                         hipStream_t s, ChunkNode *scratch, u32 cap, u32 grid, u32 *launches) {
    using G = ConstBase<B>;
    if (sound) return launch_msd_ranges_group<G, true>(p, G{}, max_size, num_cus, s, scratch, cap, grid, launches);
    return launch_msd_ranges_group<G, false>(p, G{}, max_size, num_cus, s, scratch, cap, grid, launches);
}

#define X(b) template struct MsdRangesBaseLaunch<b>;
NICEONLY_PART_BASES(X)
#undef X

}  // namespace nice
