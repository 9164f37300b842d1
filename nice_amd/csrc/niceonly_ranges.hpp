// niceonly_ranges.hpp -- niceonly_ranges_kernel: the candidate test of
// nice_process_ranges_niceonly, many caller-given ranges in one launch.
//
// The walk is niceonly_kernel's (niceonly_cand.hpp): a wave takes 8 leaves,
// scans their candidate counts and walks the packed candidate space 64 at a
// time, each candidate rebuilt as n = b0 + (gi / R) * M + residues[gi % R]
// with cand_wave's exact magic division, the square tested through the LDS
// pair table (VALU on the three-word bases), the survivors queued per wave
// for a full-wave cube pass that compares with nice_min.  New here: a leaf
// carries the index of the caller's range it was cut from (RangeLeaf), a listed
// number takes that index with it (NumOut::u), and a square survivor counts
// in its range's square_ok counter in global memory.
//
// The device functions are niceonly_cand.hpp's and radix_fast.hpp's, by
// inclusion; check_leaf_group and niceonly_kernel stay as they are and this
// kernel is instantiated in objects of its own (niceonly_ranges.hip for the
// run-time base, niceonly_ranges_part.hip for the fast bases), so the field
// kernels' objects build from unchanged sources.  No MSD filter and no sound
// variant: the ranges are tested as given.
#pragma once

#include "msd_plan.hpp"
#include "niceonly_cand.hpp"
#include "niceonly_ranges_plan.hpp"

namespace nice {

static_assert(sizeof(RangeLeaf) == 32, "the host stages RangeLeaf records as they are");

__device__ __forceinline__ void emit_range_nice(const NiceonlyLaunch &p, u64 n_lo, u64 n_hi, u32 range) {
    const u32 pos = atomicAdd(p.out.count, 1u);
    if (pos < p.out.cap) {
        p.out.n[2 * (u64)pos] = n_lo;
        p.out.n[2 * (u64)pos + 1] = n_hi;
        p.out.u[pos] = range;
    }
}

// cube_pass for ring entries whose high word carries the range index above
// bit kRangeIdShift (in range n_hi stays below it: niceonly_ranges_plan.hpp).
template <int B>
__device__ __forceinline__ void range_cube_pass(const NiceonlyLaunch &p, const ulonglong2 *q, u32 head, u32 cnt,
                                                u32 lane, const uint2 *tab) {
    wave_sync_lds();  // the queue was written by other lanes of this wave
    if (lane < cnt) {
        const ulonglong2 e = q[(head + lane) & (kCubeQ - 1)];
        const u64 n_hi = e.y & ((1ull << kRangeIdShift) - 1);
        if (cube_count<B>(e.x, n_hi, tab) >= p.nice_min) emit_range_nice(p, e.x, n_hi, (u32)(e.y >> kRangeIdShift));
    }
    wave_sync_lds();
}

// check_leaf_group with a range index per leaf.  Lane l < LPW holds leaf l and
// keeps that leaf's square survivors in a register: each round that has
// survivors counts them leaf by leaf (one ballot per leaf), and the leaf's
// total goes to its range's counter with one vector atomic at the end -- about
// one atomic per hundred candidates at the MSD floor's leaf sizes, and none
// for a leaf without survivors.
template <class G, u32 LPW>
__device__ __forceinline__ void check_range_leaf_group(const NiceRangesLaunch &rl, const G &g, const RangeLeaf &lf,
                                                       u32 lane, CandWave &cw) {
    const NiceonlyLaunch &p = rl.c;
    u32 incl = lf.count;
#pragma unroll
    for (int o = 1; o < (int)LPW; o <<= 1) {
        u32 v = __shfl_up(incl, o);
        if (lane >= (u32)o) incl += v;
    }
    const u32 excl = incl - lf.count;
    const u32 total = __shfl(incl, LPW - 1);
    [[maybe_unused]] u32 sq_mine = 0;  // lane l < LPW: square survivors of leaf l
    for (u32 r0 = 0; r0 < total; r0 += 64) {
        const u32 k = r0 + lane;
        // largest l < LPW with excl_l <= k (uniform search, all lanes active)
        u32 lo = 0;
#pragma unroll
        for (u32 step = LPW / 2; step >= 1; step >>= 1) {
            const u32 e = __shfl(excl, lo + step);
            if (lo + step < LPW && e <= k) lo += step;
        }
        const u32 j = k - __shfl(excl, lo);
        const u32 g0 = __shfl(lf.g0, lo);
        const u32 ri = __shfl(lf.range, lo);
        const u64 b0lo = __shfl(lf.b0_lo, lo), b0hi = __shfl(lf.b0_hi, lo);
        u64 n_lo = 0, n_hi = 0;
        if (k < total) {
            const u32 gi = g0 + j;
            const u32 cyc = (u32)(((u64)gi * cw.r_magic) >> cw.r_shift);
            const u32 idx = gi - cyc * p.R;
            n_lo = b0lo;
            n_hi = b0hi;
            add_u128(n_lo, n_hi, (u64)cyc * p.M + p.residues[idx]);
        }
        if constexpr (IsConst<G>::value) {
            // (every leaf of a compile-time launch lies in range)
            bool sq = false;
            if (k < total) {
                if constexpr (PairTab<G>::on) sq = square_ok_tab<IsConst<G>::base>(n_lo, n_hi, cw.tab);
                else sq = square_ok<IsConst<G>::base>(n_lo, n_hi);
            }
            const u64 bal = __ballot(sq);
            if (bal) {
#pragma unroll
                for (u32 l = 0; l < LPW; l++) {
                    const u64 m = __ballot(sq && lo == l);
                    if (lane == l) sq_mine += (u32)__popcll(m);
                }
                if (sq)
                    cw.cq[(cw.q_tail + lane_rank(bal)) & (kCubeQ - 1)] =
                        make_ulonglong2(n_lo, n_hi | (u64)ri << kRangeIdShift);
                cw.q_tail += (u32)__popcll(bal);
                if (cw.q_tail - cw.q_head >= 64) {
                    range_cube_pass<IsConst<G>::base>(p, cw.cq, cw.q_head, 64, lane, cw.tab);
                    cw.q_head += 64;
                }
            }
        } else {
            if (k < total && is_nice_dev(n_lo, n_hi, g)) emit_range_nice(p, n_lo, n_hi, ri);
        }
    }
    if constexpr (IsConst<G>::value) {
        if (lane < LPW && sq_mine) atomicAdd(&rl.square_ok[lf.range], sq_mine);
    }
}

// End of a launch, as the other batch kernels end: the last workgroup to
// retire publishes the list count to mapped host memory and re-zeroes the
// arrival counters for the stream's next launch (own atomics drained,
// barrier, one agent add per workgroup: nice_launch_finish's order).  Every
// thread of the workgroup calls it.
__device__ __forceinline__ void ranges_launch_finish(const NiceRangesLaunch &rl) {
    __shared__ u32 last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) last = last_block_arrive(rl.done);
    __syncthreads();
    if (!last) return;
    if (threadIdx.x == 0)
        *rl.count_mapped = __hip_atomic_load(rl.c.out.count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    done_reset(rl.done);
}

// The three-word bases (b65, b68, b80) need ~150-170 VGPRs: asked for 3 waves
// per SIMD (<= 168) -- b68 came out at 169, one wave less than its
// niceonly_kernel twin, without it; b65 and b80 fit anyway, and no base spills
// (profiles/ranges_niceonly/build_and_resources.txt).  The others are bounded by
// their launch bounds alone.
template <class G>
constexpr int ranges_min_waves() {
    return IsConst<G>::value && IsConst<G>::base > 64 ? 3 : 1;
}

template <class G>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ranges_min_waves<G>())))
niceonly_ranges_kernel(NiceRangesLaunch rl, G g) {
    const u32 lane = threadIdx.x & 63;
    const u32 gwave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const u32 nwaves = (gridDim.x * blockDim.x) >> 6;
    __shared__ ulonglong2 cq[4][IsConst<G>::value ? kCubeQ : 1];
    __shared__ uint2 tab[PairTab<G>::N];
    pair_tab_fill<G>(tab);  // (ends with a barrier)
    CandWave cw = cand_wave(rl.c, cq[threadIdx.x >> 6], tab);
    constexpr u32 LPW = 8;  // as niceonly_kernel
    for (u32 base = gwave * LPW; base < rl.n_leaves; base += nwaves * LPW) {
        const u32 li = base + lane;
        RangeLeaf lf{0, 0, 0, 0, 0, 0};
        if (lane < LPW && li < rl.n_leaves) lf = rl.leaves[li];
        check_range_leaf_group<G, LPW>(rl, g, lf, lane, cw);
    }
    if constexpr (IsConst<G>::value) {
        if (cw.q_tail != cw.q_head)
            range_cube_pass<IsConst<G>::base>(rl.c, cw.cq, cw.q_head, cw.q_tail - cw.q_head, lane, cw.tab);
    }
    ranges_launch_finish(rl);
}

// (the grid is niceonly_kernel's for a host leaf list: msd_plan.hpp nice_grid)
template <class G>
static hipError_t launch_nice_ranges(const NiceRangesLaunch &rl, const G &g, int num_cus, hipStream_t s) {
    const u32 grid = nice_grid(false, rl.n_leaves, num_cus, (u64)num_cus * 8);
    hipLaunchKernelGGL((niceonly_ranges_kernel<G>), dim3(grid), dim3(256), 0, s, rl, g);
    return hipGetLastError();
}

// The launcher of one fast base, defined and instantiated in that base's part
// object (niceonly_ranges_part.hip); niceonly_ranges.hip dispatches.
template <int B>
struct RangesBaseLaunch {
    static hipError_t nice(const NiceRangesLaunch &rl, int num_cus, hipStream_t s);
};

}  // namespace nice
