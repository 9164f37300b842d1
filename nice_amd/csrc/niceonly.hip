// niceonly.hip -- niceonly field processing on gfx950: the entry points of
// kernels.h.  The kernel templates are in niceonly_kernels.hpp; this object
// holds their run-time-base instantiations (any base 2..128, any n < 2^128),
// the kernels without a base parameter, and the dispatch to the fast bases'
// compile-time instantiations (niceonly_bases.h), which are built a few bases
// per object from niceonly_part.hip.
#include "niceonly_bases.h"
#include "niceonly_kernels.hpp"

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

hipError_t launch_niceonly(const NiceonlyLaunch &p, int num_cus, hipStream_t s, const SoundLaunch *snd) {
    if (!p.n_leaves_dev && p.n_leaves == 0 && !p.fin.done) return hipSuccess;
    if (snd) {
        if (snd->fast && p.n_leaves_dev) {
            switch (p.base) {
#define X(b) case b: return BaseLaunch<b>::nice_sound(p, num_cus, s, *snd);
                NICE_NICEONLY_BASES(X)
#undef X
            default: break;
            }
        }
        SoundLaunch off = *snd;
        off.prefix_test = 0;
        return launch_nice<GenericBase>(p, make_generic(p.base), num_cus, s, off);
    }
    switch (p.base) {
#define X(b) case b: return BaseLaunch<b>::nice(p, num_cus, s);
        NICE_NICEONLY_BASES(X)
#undef X
    default: return launch_nice(p, make_generic(p.base), num_cus, s);
    }
}

hipError_t launch_msd_wave(const MsdLaunch &p, const NiceonlyLaunch &c, uint32_t level0, void *scratch,
                           uint32_t grid, int num_cus, hipStream_t s, const SoundLaunch *snd) {
    if (level0 > 22 || (p.nchunks << level0) >> level0 != p.nchunks) return hipErrorInvalidValue;
    StackNode *st = (StackNode *)scratch;
    if (snd) {
        if (snd->fast) {
            switch (p.base) {
#define X(b) case b: return BaseLaunch<b>::wave_sound(p, c, level0, st, grid, num_cus, s, *snd);
                NICE_NICEONLY_BASES(X)
#undef X
            default: break;
            }
        }
        SoundLaunch off = *snd;
        off.prefix_test = 0;
        return launch_wave<GenericBase, 0>(p, c, level0, st, grid, make_generic(p.base), num_cus, s,
                                                 off);
    }
    switch (p.base) {
#define X(b) case b: return BaseLaunch<b>::wave(p, c, level0, st, grid, num_cus, s);
        NICE_NICEONLY_BASES(X)
#undef X
    default: return launch_wave(p, c, level0, st, grid, make_generic(p.base), num_cus, s);
    }
}

size_t msd_wave_scratch_bytes(uint32_t grid) { return (size_t)grid * (kWaveWG / 64) * kStackCap * sizeof(StackNode); }
uint32_t msd_wave_waves_per_group() { return kWaveWG / 64; }

u32 msd_fused_cap(u64 chunk, u64 floor_size) {
    if (chunk > 0xffffffffull || floor_size == 0) return 0;
    const u64 need = chunk / floor_size + 2;
    if (need > kFusedMaxCap) return 0;
    u32 cap = 64;
    while (cap < need) cap <<= 1;
    return cap;
}

hipError_t launch_msd_device(const MsdLaunch &p, int num_cus, hipStream_t s, ChunkNode *scratch,
                             u32 cap, u32 grid, const SoundLaunch *snd) {
    if (scratch && p.nchunks > 0xffffffffull) return hipErrorInvalidValue;
    if (snd) {
        if (snd->fast) {
            switch (p.base) {
#define X(b) case b: return BaseLaunch<b>::msd_sound(p, num_cus, s, scratch, cap, grid, *snd);
                NICE_NICEONLY_BASES(X)
#undef X
            default: break;
            }
        }
        SoundLaunch off = *snd;
        off.prefix_test = 0;
        if (scratch) return launch_fused<GenericBase, 0>(p, make_generic(p.base), scratch, cap, grid, s, off);
        return launch_msd<GenericBase, 0>(p, make_generic(p.base), num_cus, s, off);
    }
    switch (p.base) {
#define X(b) case b: return BaseLaunch<b>::msd(p, num_cus, s, scratch, cap, grid);
        NICE_NICEONLY_BASES(X)
#undef X
    default:
        if (scratch) return launch_fused(p, make_generic(p.base), scratch, cap, grid, s);
        return launch_msd(p, make_generic(p.base), num_cus, s);
    }
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

hipError_t launch_is_nice(const uint64_t *n_pairs, uint32_t count, uint32_t base, uint32_t *out,
                          hipStream_t s) {
    hipLaunchKernelGGL(is_nice_kernel, dim3((count + 255) / 256), dim3(256), 0, s, n_pairs, count,
                       make_generic(base), out);
    return hipGetLastError();
}

}  // namespace nice
