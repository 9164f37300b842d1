// msd_ranges.hip -- the recursion's range list on gfx950: the entry points of
// kernels.h (launch_msd_ranges, msd_ranges_sort).  The kernel templates are in
// msd_ranges.hpp; this object holds their run-time-base instantiations (any
// base 2..128, any n < 2^128), the level-0 kernel, the dispatch to the fast
// bases' compile-time instantiations (built a few bases per object from
// msd_ranges_part.hip) and the device sort of the records (rocPRIM's radix
// sort over the key's 60 bits).
#include <string.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "msd_ranges.hpp"
#include "niceonly_bases.h"

namespace nice {

__global__ void msd_ranges_init_kernel(MsdRangesLaunch p) {
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < p.n; i += gridDim.x * blockDim.x) {
        const u32 root = p.list[i];
        p.q[0][i] = MsdNode{(u64)root << kRangeOffBits, p.roots[root].size};
    }
    if (blockIdx.x == 0 && threadIdx.x < kMsdLevels) p.ctl[threadIdx.x] = threadIdx.x == 0 ? p.n : 0u;
}

void launch_msd_ranges_init(const MsdRangesLaunch &p, hipStream_t s) {
    const u32 grid = std::min<u32>((p.n + 255) / 256, 256);
    hipLaunchKernelGGL(msd_ranges_init_kernel, dim3(grid), dim3(256), 0, s, p);
}

hipError_t launch_msd_ranges(const MsdRangesLaunch &p, uint32_t base, bool fast, bool sound, uint64_t max_size,
                             int num_cus, hipStream_t s, ChunkNode *scratch, uint32_t cap, uint32_t grid,
                             uint32_t *launches) {
    if (p.n == 0) return hipSuccess;
    if (p.n > p.q_cap && !scratch) return hipErrorInvalidValue;
    if (fast) {
        switch (base) {
#define X(b) case b: return MsdRangesBaseLaunch<b>::group(p, sound, max_size, num_cus, s, scratch, cap, grid, launches);
            NICE_NICEONLY_BASES(X)
#undef X
        default: return hipErrorInvalidValue;  // no compile-time kernel: a missing kernel is an error
        }
    }
    const GenericBase g = make_generic(base);
    if (sound) return launch_msd_ranges_group<GenericBase, true>(p, g, max_size, num_cus, s, scratch, cap, grid, launches);
    return launch_msd_ranges_group<GenericBase, false>(p, g, max_size, num_cus, s, scratch, cap, grid, launches);
}

hipError_t msd_ranges_sort_bytes(size_t n, size_t *bytes) {
    u64 *k = nullptr;
    return rocprim::radix_sort_pairs(nullptr, *bytes, k, k, k, k, n, 0, kRangeOffBits + 20);
}

hipError_t msd_ranges_sort(void *temp, size_t temp_bytes, uint64_t *keys, uint64_t *keys_out, uint64_t *sizes,
                           uint64_t *sizes_out, size_t n, hipStream_t s) {
    return rocprim::radix_sort_pairs(temp, temp_bytes, keys, keys_out, sizes, sizes_out, n, 0, kRangeOffBits + 20, s);
}

}  // namespace nice
