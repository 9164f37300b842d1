// msd_ranges.hpp -- the device MSD recursion with a range sink: the kernels of
// nice_msd_ranges.  They are msd_fused_kernel and msd_level_kernel
// (niceonly_msd.hpp) with two changes: the level-0 nodes are a call's roots,
// which differ in size and may lie anywhere, instead of a field's chunk grid,
// and a leaf becomes a record -- (root, offset inside the root) packed into a
// 60-bit key, and its size -- instead of append_leaf's stride descriptors, so
// nothing here needs a stride table.
//
// The node rule is not restated: both kernels call classify_node with the
// template arguments the field kernels give it (ConstBase<B> or the run-time
// base, TAB off, SOUND on or off; MsdLaunch::in_range per root, as a field's
// is per field), and append with block_reserve's one atomic per workgroup.
// Sound variants only leave Filter C out: the prefix test is a per-candidate
// test and a range list has no candidates, so their SoundCtx has it off.
//
// The field kernels stay as they are; these are instantiated in objects of
// their own (msd_ranges.hip for the run-time base and the device sort,
// msd_ranges_part.hip for the fast bases).
#pragma once

#include "msd_plan.hpp"
#include "niceonly_msd.hpp"

namespace nice {

static_assert(sizeof(MsdRangeRoot) == 32, "the host stages MsdRangeRoot records as they are");

constexpr u32 kRangeOffBits = 40;  // msd_ranges_plan.hpp kMsdRangesOffBits

template <bool SOUND>
__device__ __forceinline__ SoundCtx<SOUND> ranges_sound_ctx() {
    if constexpr (SOUND) return SoundCtx<true>{nullptr, false, 0u, LeafMask{{0, 0, 0}, 0}};
    else return SoundCtx<false>{};
}

// What classify_node reads of a launch: the floor and the root's in_range (the
// probe bits stay clear: a range list has no probe form).
__device__ __forceinline__ MsdLaunch node_rule_launch(u64 floor_size) {
    MsdLaunch mp{};
    mp.floor_size = floor_size;
    return mp;
}

// A leaf's record, appended with one atomic per workgroup.  Every thread of
// the workgroup calls it (act == 1: this lane has a leaf).
__device__ __forceinline__ void append_range(const MsdRangesLaunch &p, u32 act, u64 key, u64 size, u32 *slots) {
    const u32 pos = block_reserve(&p.ctl[kMsdLeafCount], act == 1 ? 1u : 0u, slots);
    if (act != 1) return;
    if (pos >= p.leaf_cap) {
        atomicOr(&p.ctl[kMsdOverflow], 1u);
    } else {
        p.keys[pos] = key;
        p.sizes[pos] = size;
    }
}

// Form 0:msd_level_kernel over the roots of a launch together.  A node is
// (root << 40 | offset inside the root, size).
template <class G, bool SOUND>
__global__ void __launch_bounds__(256)
msd_ranges_level_kernel(MsdRangesLaunch p, u32 level, G g) {
    __shared__ u32 slots[4];
    const MsdNode *qin = p.q[level & 1];
    MsdNode *qout = p.q[(level + 1) & 1];
    const u32 n_in = min(p.ctl[level], p.q_cap);
    const u32 stride = gridDim.x * blockDim.x;
    SoundCtx<SOUND> sc = ranges_sound_ctx<SOUND>();
    MsdLaunch mp = node_rule_launch(p.floor_size);
    for (u32 b0 = blockIdx.x * blockDim.x; b0 < n_in; b0 += stride) {
        const u32 i = b0 + threadIdx.x;
        u32 act = 0;  // 0 drop / idle, 1 leaf, 2 split
        MsdNode nd{0, 0};
        if (i < n_in) {
            nd = qin[i];
            const MsdRangeRoot rt = p.roots[nd.off >> kRangeOffBits];
            u64 lo = rt.start_lo, hi = rt.start_hi;
            add_u128(lo, hi, nd.off & ((1ull << kRangeOffBits) - 1));
            mp.in_range = rt.in_range;
            act = classify_node<G, false, SOUND>(mp, level, lo, hi, nd.size, g, nullptr, &sc);
        }
        append_range(p, act, nd.off, nd.size, slots);
        const u32 cpos = block_reserve(&p.ctl[level + 1], act == 2 ? 2u : 0u, slots);
        if (act == 2) {
            if (cpos + 1 >= p.q_cap) {
                atomicOr(&p.ctl[kMsdOverflow], 1u);
            } else {
                const u64 half = nd.size / 2;
                qout[cpos] = MsdNode{nd.off, half};
                qout[cpos + 1] = MsdNode{nd.off + half, nd.size - half};
            }
        }
    }
}

// Form 1: msd_fused_kernel with a root per workgroup (grid-strided) -- the
// whole recursion of a root level by level in the workgroup's own ping-pong
// queue (`scratch`: gridDim.x x 2 x cap ChunkNodes; cap follows the launch's
// largest root, msd_plan.hpp msd_fused_cap).
template <class G, bool SOUND>
__global__ void __launch_bounds__(256)
msd_ranges_fused_kernel(MsdRangesLaunch p, ChunkNode *scratch, u32 cap, G g) {
    __shared__ u32 slots[4];
    __shared__ u32 cnt[2];
    ChunkNode *qa = scratch + (u64)blockIdx.x * 2 * cap, *qb = qa + cap;
    SoundCtx<SOUND> sc = ranges_sound_ctx<SOUND>();
    MsdLaunch mp = node_rule_launch(p.floor_size);
    for (u32 ri = blockIdx.x; ri < p.n; ri += gridDim.x) {
        const u32 root = p.list[ri];
        const MsdRangeRoot rt = p.roots[root];
        mp.in_range = rt.in_range;
        if (threadIdx.x == 0) {
            qa[0] = ChunkNode{0u, (u32)rt.size};
            cnt[0] = 1;
            cnt[1] = 0;
        }
        __syncthreads();
        ChunkNode *qin = qa, *qout = qb;
        for (u32 level = 0; level <= 22; level++) {
            const u32 n_in = cnt[0];
            if (n_in == 0) break;
            for (u32 b0 = 0; b0 < n_in; b0 += 256) {
                const u32 i = b0 + threadIdx.x;
                u32 act = 0;
                ChunkNode nd{0u, 0u};
                if (i < n_in) {
                    nd = qin[i];
                    u64 lo = rt.start_lo, hi = rt.start_hi;
                    add_u128(lo, hi, nd.off);
                    act = classify_node<G, false, SOUND>(mp, level, lo, hi, nd.size, g, nullptr, &sc);
                }
                append_range(p, act, (u64)root << kRangeOffBits | nd.off, nd.size, slots);
                if (act == 2) {
                    const u32 cp = atomicAdd(&cnt[1], 2u);
                    if (cp + 2 > cap) {
                        atomicOr(&p.ctl[kMsdOverflow], 1u);
                    } else {
                        const u32 half = nd.size / 2;
                        qout[cp] = ChunkNode{nd.off, half};
                        qout[cp + 1] = ChunkNode{nd.off + half, nd.size - half};
                    }
                }
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                cnt[0] = cnt[1] > cap ? cap : cnt[1];
                cnt[1] = 0;
            }
            __syncthreads();
            ChunkNode *t = qin;
            qin = qout;
            qout = t;
        }
        __syncthreads();  // the queues are reused by the next root
    }
}

// Form 0, level 0 (msd_ranges_init_kernel, msd_ranges.hip): the group's roots
// into q[0], the level sizes set.
void launch_msd_ranges_init(const MsdRangesLaunch &p, hipStream_t s);

// One group of a batch: form 1 with `scratch` (one launch), else init + the
// levels that can hold a split of the group's largest root (max_size).
template <class G, bool SOUND>
static hipError_t launch_msd_ranges_group(const MsdRangesLaunch &p, const G &g, u64 max_size, int num_cus,
                                          hipStream_t s, ChunkNode *scratch, u32 cap, u32 grid, u32 *launches) {
    if (scratch) {
        hipLaunchKernelGGL((msd_ranges_fused_kernel<G, SOUND>), dim3(grid), dim3(256), 0, s, p, scratch, cap, g);
        ++*launches;
    } else {
        launch_msd_ranges_init(p, s);
        ++*launches;
        const u32 last = msd_last_level(max_size, p.floor_size);
        for (u32 level = 0; level <= last; level++) {
            hipLaunchKernelGGL((msd_ranges_level_kernel<G, SOUND>), dim3(msd_level_grid(p.n, level, num_cus)),
                               dim3(256), 0, s, p, level, g);
            ++*launches;
        }
    }
    return hipGetLastError();
}

// The launcher of one fast base, defined and instantiated in that base's part
// object (msd_ranges_part.hip); msd_ranges.hip dispatches.
template <int B>
struct MsdRangesBaseLaunch {
    static hipError_t group(const MsdRangesLaunch &p, bool sound, u64 max_size, int num_cus, hipStream_t s,
                            ChunkNode *scratch, u32 cap, u32 grid, u32 *launches);
};

}  // namespace nice
