// niceonly_part.hip -- the niceonly kernels of the fast bases, one object per
// part (built with -DNICEONLY_PART=k, k < NICEONLY_NPARTS): part k
// instantiates niceonly_kernel, msd_level_kernel, msd_fused_kernel,
// msd_wave_kernel, unique_fast_kernel and cube_count_kernel for the bases of
// NICE_NICEONLY_PARTk (niceonly_bases.h), so they compile in parallel.
#include "niceonly_bases.h"
#include "niceonly_launch.hpp"

#ifndef NICEONLY_PART
#error "build with -DNICEONLY_PART=k"
#endif

#define NICEONLY_CAT2(a, b) a##b
#define NICEONLY_CAT(a, b) NICEONLY_CAT2(a, b)
#define NICEONLY_PART_BASES NICEONLY_CAT(NICE_NICEONLY_PART, NICEONLY_PART)

namespace nice {

// The const-modulus instantiations (leaf_desc's constant divisions, the lane
// walk) take in-range fields on the k = 2 stride table; a wide base's also
// need the field's end inside the walk's packed high part.
template <int B>
static bool const_mod_field(const MsdLaunch &p) {
    if (const_modulus<B>() == 0 || !p.in_range || p.M != const_modulus<B>()) return false;
    return wide_n<B>() ? (p.end_hi >> kWideHiBits) == 0 : true;
}

// Sound variants (snd; niceonly.hip sends only sound_fast fields here): one
// instantiation set per base -- the const-modulus one of a two-word base, the
// plain one of a three-word base.
// Each launcher below names the reference filter's instantiations before the
// sound one.  The order matters to the build, not to the result: the compiler
// emits a part's kernels in the order its host code first names them, and the
// sound level and fused kernels of the two-word bases came out with other
// instructions when they were named first.
template <int B>
bool BaseLaunch<B>::sound_fast(const MsdLaunch &p) {
    if (!p.in_range || p.M != (u32)(B - 1) * B * B) return false;
    return const_modulus<B>() == 0 || const_mod_field<B>(p);
}

template <int B>
hipError_t BaseLaunch<B>::nice(const NiceonlyLaunch &p, int num_cus, hipStream_t s, const SoundLaunch *snd) {
    if (!snd) return launch_nice(p, ConstBase<B>{}, num_cus, s);
    return launch_nice(p, ConstBase<B>{}, num_cus, s, *snd);
}

template <int B>
hipError_t BaseLaunch<B>::msd(const MsdLaunch &p, int num_cus, hipStream_t s, ChunkNode *scratch, u32 cap, u32 grid,
                              const SoundLaunch *snd) {
    using G = ConstBase<B>;
    constexpr u32 MC = const_modulus<B>();
    if (!snd) {
        if (const_mod_field<B>(p)) return launch_msd<G, MC>(p, G{}, num_cus, s, scratch, cap, grid);
        return launch_msd<G, 0>(p, G{}, num_cus, s, scratch, cap, grid);
    }
    return launch_msd<G, MC>(p, G{}, num_cus, s, scratch, cap, grid, *snd);
}

template <int B>
hipError_t BaseLaunch<B>::wave(const MsdLaunch &p, const NiceonlyLaunch &c, u32 level0, StackNode *scratch,
                               u32 grid, int num_cus, hipStream_t s, const SoundLaunch *snd) {
    using G = ConstBase<B>;
    constexpr u32 MC = const_modulus<B>();
    if (!snd) {
        if (const_mod_field<B>(p)) return launch_wave<G, MC>(p, c, level0, scratch, grid, G{}, num_cus, s);
        return launch_wave<G, 0>(p, c, level0, scratch, grid, G{}, num_cus, s);
    }
    return launch_wave<G, MC>(p, c, level0, scratch, grid, G{}, num_cus, s, *snd);
}

template <int B>
hipError_t BaseLaunch<B>::unique(const u64 *n_pairs, u32 count, u32 *out, hipStream_t s) {
    hipLaunchKernelGGL(unique_fast_kernel<B>, dim3((count + 255) / 256), dim3(256), 0, s, n_pairs, count, out);
    return hipGetLastError();
}

template <int B>
hipError_t BaseLaunch<B>::cube(const u64 *n_pairs, u32 count, u32 *out, hipStream_t s) {
    hipLaunchKernelGGL(cube_count_kernel<B>, dim3((count + 255) / 256), dim3(256), 0, s, n_pairs, count, out);
    return hipGetLastError();
}

#define X(b) template struct BaseLaunch<b>;
NICEONLY_PART_BASES(X)
#undef X

}  // namespace nice
