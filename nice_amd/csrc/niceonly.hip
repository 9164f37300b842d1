// niceonly.hip -- niceonly field processing on gfx950: the entry points of
// kernels.h.  The kernel templates are in niceonly_cand.hpp, niceonly_msd.hpp
// and niceonly_wave.hpp, their launchers in niceonly_launch.hpp; this object
// holds their run-time-base instantiations (any base 2..128, any n < 2^128),
// the kernels without a base parameter, and the dispatch to the fast bases'
// compile-time instantiations (niceonly_bases.h), which are built a few bases
// per object from niceonly_part.hip.
#include "niceonly_bases.h"
#include "niceonly_launch.hpp"

namespace nice {

__global__ void is_nice_kernel(const u64 *n_pairs, u32 count, GenericBase g, u32 *out) {
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = is_nice_dev(n_pairs[2 * i], n_pairs[2 * i + 1], g) ? 1u : 0u;
}

// Level 0: this batch's chunks of the field (dealt: every deal_stride-th
// chunk from deal_offset), each clipped to the field's end.
__global__ void msd_init_kernel(MsdLaunch p) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < p.nchunks;
         i += (u64)gridDim.x * blockDim.x) {
        const u64 c = p.deal_offset + (p.first + i) * p.deal_stride;
        u64 lo = p.start_lo, hi = p.start_hi;
        // c * chunk < field size < 2^64 (checked by the host)
        add_u128(lo, hi, c * p.chunk);
        // numbers left in the field from this chunk's start: end - lo (u128)
        const u64 rem_lo = p.end_lo - lo;
        const u64 rem_hi = p.end_hi - hi - (p.end_lo < lo ? 1 : 0);
        const u64 size = rem_hi || rem_lo > p.chunk ? p.chunk : rem_lo;
        p.q[0][i] = MsdNode{c * p.chunk, size};
    }
    // counters (layout.h): [0] level-0 size, up to kMsdLeafCount per batch,
    // the rest sticky over the field (zeroed with the first batch, as is the
    // field's nice count)
    if (blockIdx.x == 0 && threadIdx.x < kMsdSquareParts) {
        const u32 w = threadIdx.x;
        if (w == 0) p.counters[0] = (u32)p.nchunks;
        else if (w <= kMsdLeafCount || p.first_batch) p.counters[w] = 0;
        if (w == 0 && p.first_batch) *p.nice_count = 0;
    }
}

void launch_msd_init(const MsdLaunch &p, hipStream_t s) {
    hipLaunchKernelGGL(msd_init_kernel, dim3(256), dim3(256), 0, s, p);
}

// A sound field's kernels: the base's compile-time variants where the prefix
// test can run (SoundLaunch::fast, which the caller sets only for device-MSD
// fields that sound_prefix_field accepts), else the run-time-base variants,
// which only leave Filter C out.
bool sound_prefix_field(const MsdLaunch &p) {
    switch (p.base) {
#define X(b) case b: return BaseLaunch<b>::sound_fast(p);
        NICE_NICEONLY_BASES(X)
#undef X
    default: return false;
    }
}

// One launch for any base: fast(BaseLaunch<b>{}, snd) runs a fast base's
// compile-time kernels, generic(snd...) the run-time-base ones.  A sound field
// that is not fast_ok, or whose base has no compile-time kernels, runs the
// latter with the prefix test cleared.
template <class Fast, class Generic>
static hipError_t dispatch_base(u32 base, const SoundLaunch *snd, bool fast_ok, Fast fast, Generic generic) {
    if (!snd || fast_ok) {
        switch (base) {
#define X(b) case b: return fast(BaseLaunch<b>{}, snd);
            NICE_NICEONLY_BASES(X)
#undef X
        default: break;
        }
    }
    if (!snd) return generic();
    SoundLaunch off = *snd;
    off.prefix_test = 0;
    return generic(off);
}

hipError_t launch_niceonly(const NiceonlyLaunch &p, int num_cus, hipStream_t s, const SoundLaunch *snd) {
    if (!p.n_leaves_dev && p.n_leaves == 0 && !p.fin.done) return hipSuccess;
    return dispatch_base(
        p.base, snd, snd && snd->fast && p.n_leaves_dev,
        [&](auto b, const SoundLaunch *sn) { return decltype(b)::nice(p, num_cus, s, sn); },
        [&](auto... off) { return launch_nice(p, make_generic(p.base), num_cus, s, off...); });
}

hipError_t launch_msd_wave(const MsdLaunch &p, const NiceonlyLaunch &c, uint32_t level0, void *scratch,
                           uint32_t grid, int num_cus, hipStream_t s, const SoundLaunch *snd) {
    if (level0 > 22 || (p.nchunks << level0) >> level0 != p.nchunks) return hipErrorInvalidValue;
    StackNode *st = (StackNode *)scratch;
    return dispatch_base(
        p.base, snd, snd && snd->fast,
        [&](auto b, const SoundLaunch *sn) { return decltype(b)::wave(p, c, level0, st, grid, num_cus, s, sn); },
        [&](auto... off) { return launch_wave(p, c, level0, st, grid, make_generic(p.base), num_cus, s, off...); });
}

hipError_t launch_msd_device(const MsdLaunch &p, int num_cus, hipStream_t s, ChunkNode *scratch,
                             u32 cap, u32 grid, const SoundLaunch *snd) {
    if (scratch && p.nchunks > 0xffffffffull) return hipErrorInvalidValue;
    return dispatch_base(
        p.base, snd, snd && snd->fast,
        [&](auto b, const SoundLaunch *sn) { return decltype(b)::msd(p, num_cus, s, scratch, cap, grid, sn); },
        [&](auto... off) { return launch_msd(p, make_generic(p.base), num_cus, s, scratch, cap, grid, off...); });
}

hipError_t launch_unique_fast(const uint64_t *n_pairs, uint32_t count, uint32_t base, uint32_t *out,
                              hipStream_t s) {
    switch (base) {
#define X(b) case b: return BaseLaunch<b>::unique(n_pairs, count, out, s);
        NICE_NICEONLY_BASES(X)
#undef X
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_cube_count(const uint64_t *n_pairs, uint32_t count, uint32_t base, uint32_t *out,
                             hipStream_t s) {
    switch (base) {
#define X(b) case b: return BaseLaunch<b>::cube(n_pairs, count, out, s);
        NICE_NICEONLY_BASES(X)
#undef X
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_is_nice(const uint64_t *n_pairs, uint32_t count, uint32_t base, uint32_t *out,
                          hipStream_t s) {
    hipLaunchKernelGGL(is_nice_kernel, dim3((count + 255) / 256), dim3(256), 0, s, n_pairs, count,
                       make_generic(base), out);
    return hipGetLastError();
}

}  // namespace nice
