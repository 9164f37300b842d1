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
// kernels' objects build from unchanged sources.  No MSD filter: the ranges are
// tested as given.
//
// The prefix test (RangesPrefixLaunch, kernels.h): the kernel takes a trailing
// parameter pack, as niceonly_cand.hpp's kernels do for their sound variants
// -- empty for the plain call, whose instantiations compile to what they were,
// and one RangesPrefixLaunch for the variant of the fast bases -- and
// check_range_leaf_group the flag PRE.  There a leaf carries its range's LeafMask, made
// by range_mask_kernel below in a launch of its own (one lane per range, every
// lane busy; at leaf load only 8 lanes of a wave hold leaves, and a mask costs
// as much as several candidate tests), and cand_rejected runs ahead of the
// square test: a rejected candidate skips it and counts in its range's
// rejected counter, a kept one queues in a ring of the wave's for a full-wave
// square pass (range_square_pass).  The run-time-base kernel has no variant.
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

// What the prefix-testing variant keeps per lane (SoundCtx's role in
// niceonly_cand.hpp): the launch's tables and the mask of the lane's leaf.  The
// plain kernel's holds nothing, and the steps below read the fields only under
// `if constexpr (PRE)`.
template <bool PRE>
struct RangePrefixCtx {};
template <>
struct RangePrefixCtx<true> {
    const RangesPrefixLaunch *pl;
    LeafMask lm;
    // The wave's ring of kept candidates (kCubeQ entries, as the survivor ring:
    // n, the range index above kRangeIdShift; head / tail wave-uniform).  The
    // test rejects lane by lane, so testing the kept squares in place would run
    // the square test for nearly every round with a fifth of the lanes; queued,
    // it runs once per 64 kept candidates.
    ulonglong2 *kq;
    u32 k_head, k_tail;
};
__device__ __forceinline__ RangePrefixCtx<false> range_prefix_ctx() { return {}; }
__device__ __forceinline__ RangePrefixCtx<true> range_prefix_ctx(const RangesPrefixLaunch &pl) {
    return RangePrefixCtx<true>{&pl, LeafMask{{0, 0, 0}, 0}, nullptr, 0, 0};
}

// The square test on the first `cnt` <= 64 entries of the kept ring, one per
// lane.  A survivor counts in its range's square_ok with an atomic of its own
// (about one kept candidate in twenty; the leaf that held it may belong to an
// earlier group of the wave, so no lane keeps its count) and queues for the
// cube pass as in the plain kernel.
template <class G>
__device__ __forceinline__ void range_square_pass(const NiceRangesLaunch &rl, RangePrefixCtx<true> &pc, CandWave &cw,
                                                  u32 cnt, u32 lane) {
    constexpr int B = IsConst<G>::base;
    wave_sync_lds();  // the ring was written by other lanes of this wave
    bool sq = false;
    ulonglong2 e = make_ulonglong2(0, 0);
    if (lane < cnt) {
        e = pc.kq[(pc.k_head + lane) & (kCubeQ - 1)];
        const u64 n_hi = e.y & ((1ull << kRangeIdShift) - 1);
        if constexpr (PairTab<G>::on) sq = square_ok_tab<B>(e.x, n_hi, cw.tab);
        else sq = square_ok<B>(e.x, n_hi);
    }
    wave_sync_lds();
    pc.k_head += cnt;
    const u64 bal = __ballot(sq);
    if (bal) {
        if (sq) {
            atomicAdd(&rl.square_ok[(u32)(e.y >> kRangeIdShift)], 1u);
            cw.cq[(cw.q_tail + lane_rank(bal)) & (kCubeQ - 1)] = e;
        }
        cw.q_tail += (u32)__popcll(bal);
        if (cw.q_tail - cw.q_head >= 64) {
            range_cube_pass<B>(rl.c, cw.cq, cw.q_head, 64, lane, cw.tab);
            cw.q_head += 64;
        }
    }
}

// check_leaf_group with a range index per leaf.  Lane l < LPW holds leaf l and
// keeps that leaf's square survivors in a register: each round that has
// survivors counts them leaf by leaf (one ballot per leaf), and the leaf's
// total goes to its range's counter with one vector atomic at the end -- about
// one atomic per hundred candidates at the MSD floor's leaf sizes, and none
// for a leaf without survivors.
// PRE: pc.lm is the mask of the lane's leaf, shuffled to the lanes that walk
// the leaf as check_leaf_group does; rejected candidates are counted per leaf
// like the square survivors, and the kept ones queue for range_square_pass.
template <class G, u32 LPW, bool PRE>
__device__ __forceinline__ void check_range_leaf_group(const NiceRangesLaunch &rl, const G &g, const RangeLeaf &lf,
                                                       u32 lane, CandWave &cw, RangePrefixCtx<PRE> &pc) {
    static_assert(!PRE || IsConst<G>::value, "the prefix test runs on the compile-time kernels");
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
    [[maybe_unused]] u32 rej_mine = 0;  // PRE: ... and the candidates of leaf l the prefix test rejected
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
        [[maybe_unused]] bool gone = false;  // PRE: rejected by the prefix test
        [[maybe_unused]] LeafMask mk;
        if constexpr (PRE) {  // lane lo holds the leaf's mask (read with every lane active)
#pragma unroll
            for (int w = 0; w < Radix<IsConst<G>::base>::MW; w++) mk.w[w] = __shfl(pc.lm.w[w], lo);
            mk.multi = __shfl(pc.lm.multi, lo);
        }
        if (k < total) {
            const u32 gi = g0 + j;
            const u32 cyc = (u32)(((u64)gi * cw.r_magic) >> cw.r_shift);
            const u32 idx = gi - cyc * p.R;
            n_lo = b0lo;
            n_hi = b0hi;
            add_u128(n_lo, n_hi, (u64)cyc * p.M + p.residues[idx]);
            if constexpr (PRE) {
                constexpr int MW = Radix<IsConst<G>::base>::MW;
                u32 pm[MW];
#pragma unroll
                for (int w = 0; w < MW; w++) pm[w] = mk.w[w];
                gone = cand_rejected<IsConst<G>::base>(pc.pl->snd, pm, mk.multi, idx);
            }
        }
        if constexpr (PRE) {
            if (__ballot(gone)) {
#pragma unroll
                for (u32 l = 0; l < LPW; l++) {
                    const u64 m = __ballot(gone && lo == l);
                    if (lane == l) rej_mine += (u32)__popcll(m);
                }
            }
            const bool kept = k < total && !gone;
            const u64 kb = __ballot(kept);
            if (kb) {
                if (kept)
                    pc.kq[(pc.k_tail + lane_rank(kb)) & (kCubeQ - 1)] =
                        make_ulonglong2(n_lo, n_hi | (u64)ri << kRangeIdShift);
                pc.k_tail += (u32)__popcll(kb);
                if (pc.k_tail - pc.k_head >= 64) range_square_pass<G>(rl, pc, cw, 64, lane);
            }
        } else if constexpr (IsConst<G>::value) {
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
    if constexpr (IsConst<G>::value && !PRE) {
        if (lane < LPW && sq_mine) atomicAdd(&rl.square_ok[lf.range], sq_mine);
    }
    if constexpr (PRE) {
        if (lane < LPW && rej_mine) atomicAdd(&pc.pl->rejected[lf.range], (unsigned long long)rej_mine);
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

template <class G, class... S>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ranges_min_waves<G>())))
niceonly_ranges_kernel(NiceRangesLaunch rl, G g, S... pre) {
    constexpr bool PRE = sizeof...(S) != 0;
    const u32 lane = threadIdx.x & 63;
    const u32 gwave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const u32 nwaves = (gridDim.x * blockDim.x) >> 6;
    __shared__ ulonglong2 cq[4][IsConst<G>::value ? kCubeQ : 1];
    __shared__ uint2 tab[PairTab<G>::N];
    pair_tab_fill<G>(tab);  // (ends with a barrier)
    CandWave cw = cand_wave(rl.c, cq[threadIdx.x >> 6], tab);
    [[maybe_unused]] RangePrefixCtx<PRE> pc = range_prefix_ctx(pre...);
    if constexpr (PRE) {
        __shared__ ulonglong2 kq[4][kCubeQ];
        pc.kq = kq[threadIdx.x >> 6];
    }
    constexpr u32 LPW = 8;  // as niceonly_kernel
    for (u32 base = gwave * LPW; base < rl.n_leaves; base += nwaves * LPW) {
        const u32 li = base + lane;
        RangeLeaf lf{0, 0, 0, 0, 0, 0};
        if (lane < LPW && li < rl.n_leaves) lf = rl.leaves[li];
        if constexpr (PRE) {
            pc.lm = LeafMask{{0, 0, 0}, 0};
            if (lane < LPW && li < rl.n_leaves) pc.lm = pc.pl->masks[lf.mask];
        }
        check_range_leaf_group<G, LPW, PRE>(rl, g, lf, lane, cw, pc);
    }
    if constexpr (PRE) {
        if (pc.k_tail != pc.k_head) range_square_pass<G>(rl, pc, cw, pc.k_tail - pc.k_head, lane);
    }
    if constexpr (IsConst<G>::value) {
        if (cw.q_tail != cw.q_head)
            range_cube_pass<IsConst<G>::base>(rl.c, cw.cq, cw.q_head, cw.q_tail - cw.q_head, lane, cw.tab);
    }
    ranges_launch_finish(rl);
}

// (the grid is niceonly_kernel's for a host leaf list: msd_plan.hpp nice_grid)
template <class G, class... S>
static hipError_t launch_nice_ranges(const NiceRangesLaunch &rl, const G &g, int num_cus, hipStream_t s,
                                     const S &...pre) {
    const u32 grid = nice_grid(false, rl.n_leaves, num_cus, (u64)num_cus * 8);
    hipLaunchKernelGGL((niceonly_ranges_kernel<G, S...>), dim3(grid), dim3(256), 0, s, rl, g, pre...);
    return hipGetLastError();
}

// The LeafMask of each caller range, one lane per range: msd_prefix_masks on
// [first, last] as classify_node computes a leaf's -- all ones when P2 + P3
// itself repeats (every candidate of the range goes), multi = 1 -- and the
// all-zero mask with multi = 0, which rejects nothing, for a range of one
// number.
template <int B>
__global__ void __launch_bounds__(256) range_mask_kernel(const RangeSpan *spans, u32 n, LeafMask *masks) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const RangeSpan sp = spans[i];
    LeafMask m{{0, 0, 0}, 0};
    if (sp.first_lo != sp.last_lo || sp.first_hi != sp.last_hi) {
        constexpr int MW = Radix<B>::MW;
        u32 pm[MW];
        const u32 dup = msd_prefix_masks<B>(sp.first_lo, sp.first_hi, sp.last_lo, sp.last_hi, pm);
#pragma unroll
        for (int w = 0; w < MW; w++) m.w[w] = dup ? ~0u : pm[w];
        m.multi = 1;
    }
    masks[i] = m;
}

// The launcher of one fast base, defined and instantiated in that base's part
// object (niceonly_ranges_part.hip); niceonly_ranges.hip dispatches.
template <int B>
struct RangesBaseLaunch {
    static hipError_t nice(const NiceRangesLaunch &rl, int num_cus, hipStream_t s);
    static hipError_t nice_prefix(const NiceRangesLaunch &rl, const RangesPrefixLaunch &pre, int num_cus,
                                  hipStream_t s);
    static hipError_t masks(const RangeSpan *spans, u32 n, LeafMask *out, hipStream_t s);
};

}  // namespace nice
