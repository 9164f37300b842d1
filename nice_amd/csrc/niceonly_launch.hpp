// niceonly_launch.hpp -- the host launchers of the niceonly kernel templates,
// and BaseLaunch, through which niceonly.hip reaches the fast bases'
// instantiations in the part objects.  The grids are msd_plan.hpp's.
#pragma once

#include "msd_plan.hpp"
#include "niceonly_wave.hpp"

namespace nice {

// (S: nothing, or one SoundLaunch for the sound variants)
template <class G, class... S>
static hipError_t launch_nice(const NiceonlyLaunch &p, const G &g, int num_cus, hipStream_t s, S... snd) {
    // (probe NICE_NICE_GRID: caps of 128..2048 workgroups tie on the bench
    // step, 1.25e8 and 1e9; profiles/r06/niceonly/nice_grid.log)
    const u64 cap = probe_knob("NICE_NICE_GRID", (u64)num_cus * 8);
    const u32 grid = nice_grid(p.n_leaves_dev != nullptr, p.n_leaves, num_cus, cap);
    hipLaunchKernelGGL((niceonly_kernel<G, S...>), dim3(grid), dim3(256), 0, s, p, g, snd...);
    return hipGetLastError();
}

// Level 0 of a batch (msd_init_kernel, niceonly.hip): the field's dealt chunks
// into p.q[0], the batch's counters zeroed.
void launch_msd_init(const MsdLaunch &p, hipStream_t s);

// ... and its levels [from, to), one launch each.
template <class G, u32 MC, class... S>
static void launch_levels(const MsdLaunch &p, u32 from, u32 to, const G &g, int num_cus, hipStream_t s, S... snd) {
    for (u32 level = from; level < to; level++)
        hipLaunchKernelGGL((msd_level_kernel<G, MC, S...>), dim3(msd_level_grid(p.nchunks, level, num_cus)), dim3(256),
                           0, s, p, level, g, snd...);
}

// A batch's recursion into its leaf list.  scratch: one fused launch of
// `grid` workgroups (scratch holds grid x 2 x cap ChunkNodes), else init + the
// levels that can hold a split.
// (Measured and not kept, round 6: one wave per chunk instead of four.  On
// the bench field's first 1.25e8 numbers, which have no survivors, the
// pipelined step was 1.3 % faster; on the whole 1e9 field 0.7 % slower (the
// niceonly chain 0.061 against 0.040 ms) and on the 8-way dealt shares, the
// N = 8 load, 0.7-0.9 % slower; profiles/r06/niceonly/msd_wg.log, sp_wg.log.)
template <class G, u32 MC = 0, class... S>
static hipError_t launch_msd(const MsdLaunch &p, const G &g, int num_cus, hipStream_t s, ChunkNode *scratch, u32 cap,
                             u32 grid, S... snd) {
    if (scratch) {
        hipLaunchKernelGGL((msd_fused_kernel<G, MC, S...>), dim3(grid), dim3(256), 0, s, p, scratch, cap, g, snd...);
    } else {
        launch_msd_init(p, s);
        launch_levels<G, MC>(p, 0, msd_last_level(p.chunk, p.floor_size) + 1, g, num_cus, s, snd...);
    }
    return hipGetLastError();
}

template <class G, u32 MC = 0, class... S>
static hipError_t launch_wave(const MsdLaunch &p, const NiceonlyLaunch &c, u32 level0, StackNode *scratch,
                              u32 grid, const G &g, int num_cus, hipStream_t s, S... snd) {
    launch_msd_init(p, s);
    launch_levels<G, MC>(p, 0, level0, g, num_cus, s, snd...);
    hipLaunchKernelGGL((msd_wave_kernel<G, MC, S...>), dim3(grid), dim3(kWaveWG), 0, s, p, c, level0, scratch, g, snd...);
    return hipGetLastError();
}

// Diagnostics: the in-range fast path's unique-digit count (the popcount that
// niceonly_kernel's in-range test compares with the base), per n.
template <int B>
__global__ void unique_fast_kernel(const u64 *n_pairs, u32 count, u32 *out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = unique_fast<B>(n_pairs[2 * i], n_pairs[2 * i + 1]);
}
// ... and the cube pass's count (cube_count, niceonly_cand.hpp), per n: the
// pair table filled as niceonly_kernel fills it.
template <int B>
__global__ void __launch_bounds__(256) cube_count_kernel(const u64 *n_pairs, u32 count, u32 *out) {
    using G = ConstBase<B>;
    __shared__ uint2 tab[PairTab<G>::N];
    pair_tab_fill<G>(tab);  // (ends with a barrier)
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = cube_count<B>(n_pairs[2 * i], n_pairs[2 * i + 1], tab);
}

// The launchers of one fast base (niceonly_bases.h), defined and instantiated
// in that base's part object (niceonly_part.hip); niceonly.hip dispatches.
// snd: null for the reference filter's kernels, else the base's sound
// variants -- only for the fields they run the prefix test on (sound_fast: in
// range on the k = 2 table); niceonly.hip sends every other sound field to the
// run-time-base variants.
template <int B>
struct BaseLaunch {
    static bool sound_fast(const MsdLaunch &p);
    static hipError_t nice(const NiceonlyLaunch &p, int num_cus, hipStream_t s, const SoundLaunch *snd);
    // (scratch, cap, grid: launch_msd's)
    static hipError_t msd(const MsdLaunch &p, int num_cus, hipStream_t s, ChunkNode *scratch, u32 cap, u32 grid,
                          const SoundLaunch *snd);
    static hipError_t wave(const MsdLaunch &p, const NiceonlyLaunch &c, u32 level0, StackNode *scratch, u32 grid,
                           int num_cus, hipStream_t s, const SoundLaunch *snd);
    static hipError_t unique(const u64 *n_pairs, u32 count, u32 *out, hipStream_t s);
    static hipError_t cube(const u64 *n_pairs, u32 count, u32 *out, hipStream_t s);
};

}  // namespace nice
