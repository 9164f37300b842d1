// niceonly_cand.hpp -- the candidate test of niceonly field processing on
// gfx950, and the compile-time rules and sound-filter state every niceonly
// kernel template shares.  The templates are in four headers, each including
// the one before it:
//   niceonly_cand.hpp    the rules; the candidate test; niceonly_kernel
//   niceonly_msd.hpp     the device MSD filter; msd_level_kernel, msd_fused_kernel
//   niceonly_wave.hpp    the lane walk; msd_wave_kernel
//   niceonly_launch.hpp  the host launchers and BaseLaunch
// Instantiated for the run-time base in niceonly.hip and for the fast bases of
// niceonly_bases.h, a few per object, in niceonly_part.hip.
//
// Replaces niceonly_ranges_kernel (common/src/cuda/nice_kernels.cu:420-470),
// the CPU stride walk it mirrors (common/src/stride_filter.rs:139-155) and,
// optionally, the host MSD recursion in front of it
// (common/src/msd_prefix_filter.rs:382-674).
//
// niceonly_kernel: wave-level load balancing.  A wave takes 8 leaves (lanes
// 0..7), scans their candidate counts across the wave, and then walks the
// packed candidate space 64 at a time: lane k finds its leaf by a binary
// search over the wave's exclusive prefix (cross-lane reads), rebuilds n = b0
// + ((g0 + j) / R) * M + residues[(g0 + j) % R] and tests it: in range, the
// digit union of n^2 (pair-mask table in LDS) and, for the few repeat-free
// squares queued per wave, of n^3 has b members (client_process.rs:222-253).
// A leaf holds ~20 candidates at the CPU path's MSD floor of 250 (b40), so
// one-wave-per-range would leave two thirds of a 64-lane wave idle.
//
// msd_fused_kernel: a chunk's whole MSD recursion in one workgroup (chunks up
// to 16384 floors, e.g. the client's 1e6 chunks).
// msd_level_kernel: the MSD recursion as a level-synchronous BFS.  Every node
// of level d is one lane: leaf -> stride-index descriptor appended to the leaf
// list; skippable -> dropped; else two children appended to level d+1.
// msd_wave_kernel: larger chunks -- the level BFS stops at a root level and
// each wave recurses below it with its own work stack, testing the leaves it
// finds in the same launch (see there).
#pragma once

#include "kernels.h"
#include "nice_device.hpp"
#include "probe.hpp"
#include "radix_fast.hpp"

namespace nice {

template <class G>
struct IsConst {
    static constexpr bool value = false;
    static constexpr int base = 0;
};
template <int B>
struct IsConst<ConstBase<B>> {
    static constexpr bool value = true;
    static constexpr int base = B;
};

// The k = 2 stride modulus M = (b - 1) b^2 as a compile-time constant for the
// in-range fields of the two-word bases (leaf_desc's constant divisions, the
// wave kernel's lane walk), else 0.
template <int B>
constexpr u32 const_modulus() {
    return B > 32 && B <= 64 ? (u32)((B - 1) * B * B) : 0u;
}
// Two-word bases whose in-range n pass 64 bits (b57..64, b^DN >= 2^64): the
// wide leaf descriptor and lane walk.  The others' n fit a u64.
template <int B>
constexpr bool wide_n() {
    if (const_modulus<B>() == 0) return false;
    unsigned __int128 v = 1;
    for (int i = 0; i < Radix<B>::DN; i++) v *= (unsigned)B;
    return (v >> 64) != 0;
}
template <class G>
struct WideN {
    static constexpr bool value = false;
};
template <int B>
struct WideN<ConstBase<B>> {
    static constexpr bool value = wide_n<B>();
};
// A wide in-range n's high word fits kWideHiBits bits (n^3 has D3 digits: b64
// n < 64^(38/3) = 2^76, the largest; the launchers check the field's end), and
// every stride index g0 <= R < M < 2^kWideG0Bits: the lane walk packs both
// into one queue word (LeafW).
constexpr u32 kWideHiBits = 12, kWideG0Bits = 20;

// Sound filter (NICE_FILTER_SOUND; kernels.h SoundLaunch, radix_fast.hpp): the
// kernels below take a trailing parameter pack, empty for the reference filter
// -- whose instantiations keep their signature and compile to what they were --
// and one SoundLaunch for the sound variants.  Those leave Filter C out of the
// recursion; with the prefix test on (compile-time base, in-range field, k = 2
// table) a leaf carries its prefix mask and every stride candidate is tested
// against its residue's low-digit mask before the square test.  What a sound
// variant keeps per lane is in SoundCtx<true>.  Every kernel makes one
// SoundCtx<SOUND> and hands its address to the shared steps, which take SOUND
// as a template argument, or what mask_list() and mask() give: each step has
// one call site for both filters.  SoundCtx<false> holds nothing -- its mask
// list and mask are null, as a sound launch's list is with the prefix test off
// -- and the steps read the fields of SoundCtx<true> only under `if constexpr
// (SOUND)`, which encloses code that one filter alone has (loading a leaf's
// mask, the rejected count).
template <bool SOUND>
struct SoundCtx {
    __device__ __forceinline__ LeafMask *mask_list() const { return nullptr; }
    __device__ __forceinline__ const LeafMask *mask() const { return nullptr; }
};
template <>
struct SoundCtx<true> {
    const SoundLaunch *snd;
    bool pt;      // the prefix test is on (uniform over the launch)
    u32 rej;      // candidates this lane rejected
    LeafMask lm;  // the mask of the lane's node or leaf
    // where append_leaf puts a leaf's mask beside its records, and that mask
    __device__ __forceinline__ LeafMask *mask_list() const { return pt ? snd->leaf_masks : nullptr; }
    __device__ __forceinline__ const LeafMask *mask() const { return &lm; }
};
template <class G>
__device__ __forceinline__ SoundCtx<false> sound_ctx(u32) { return {}; }
template <class G>
__device__ __forceinline__ SoundCtx<true> sound_ctx(u32 in_range, const SoundLaunch &snd) {
    return SoundCtx<true>{&snd, IsConst<G>::value && in_range && snd.prefix_test, 0u, LeafMask{{0, 0, 0}, 0}};
}

// A leaf's prefix mask from its queue word(s) against candidate idx's residue
// words: the candidate is rejected.
template <int B>
__device__ __forceinline__ bool cand_rejected(const SoundLaunch &snd, const u32 (&pm)[Radix<B>::MW], u32 multi,
                                              u32 idx) {
    constexpr int MW = Radix<B>::MW;
    u32 low[MW];
#pragma unroll
    for (int w = 0; w < MW; w++) low[w] = snd.lowmask[idx * MW + w];
    return prefix_rejects<MW>(pm, multi, low, snd.residues[idx] >> 31);
}

// This workgroup's rejected candidates (per-lane counts) into the field's
// counter: one LDS add per wave, one global add per workgroup.  Every thread
// calls it (a barrier inside).
__device__ __forceinline__ void rejected_flush(unsigned long long *ctr, u32 mine) {
    __shared__ unsigned long long wg_sum;
    if (threadIdx.x == 0) wg_sum = 0;
    __syncthreads();
    u64 v = mine;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&wg_sum, (unsigned long long)v);
    __syncthreads();
    if (threadIdx.x == 0 && wg_sum) atomicAdd(ctr, wg_sum);
}

// ---------------------------------------------------------------------------
// Candidate check kernel
// ---------------------------------------------------------------------------
__device__ __forceinline__ u32 lane_rank(u64 mask) {
    return __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0u));
}

// LDS (and, with the workgroup-scope fence, global) accesses of one wave
// ordered across its lanes: a wave runs in lockstep, so no barrier is needed.
__device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ void wave_sync_global() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ void emit_nice(const NiceonlyLaunch &p, u64 n_lo, u64 n_hi) {
    const u32 pos = atomicAdd(p.out.count, 1u);
    if (pos < p.out.cap) {
        p.out.n[2 * (u64)pos] = n_lo;
        p.out.n[2 * (u64)pos + 1] = n_hi;
    }
}

// Square-survivor ring per wave (entries; a power of two >= 128: a round adds
// at most 64 to fewer than 64 queued).
constexpr u32 kCubeQ = 128;

// LDS pair-mask table of the in-range test (two-word fast bases): entries
// per base, 1 (unused) otherwise.
template <class G>
struct PairTab {
    static constexpr bool on = IsConst<G>::value && IsConst<G>::base > 32 && IsConst<G>::base <= 64;
    static constexpr u32 N = on ? (u32)IsConst<G>::base * IsConst<G>::base : 1u;
};
// Every thread of the workgroup calls it (ends with a barrier).
template <class G>
__device__ __forceinline__ void pair_tab_fill(uint2 *tab) {
    if constexpr (PairTab<G>::on) {
        constexpr u32 b = IsConst<G>::base;
        for (u32 e = threadIdx.x; e < PairTab<G>::N; e += blockDim.x) {
            const u64 bits = (1ull << (e % b)) | (1ull << (e / b));
            tab[e] = make_uint2((u32)bits, (u32)(bits >> 32));
        }
    }
    __syncthreads();
}

// The full niceness test on `cnt` <= 64 queued candidates, one per lane.  At
// the MSD floor about one stride candidate in ~20 has a repeat-free square
// (the MSD filter already vetted the leading digits), yet nearly every round of
// 64 holds one: testing the cube in place ran the 220-instruction cube for
// almost every wave and round.  Queued, it runs once per 64 survivors.
// A queued n is listed when the digit union of n^2 and n^3 (cube_count: 0 when
// n^2 repeats a digit) has at least p.nice_min members: b in production, which
// in range is "exactly b"; nice_debug_set_nice_min lowers it for the tests.
template <int B>
__device__ __forceinline__ u32 cube_count(u64 n_lo, u64 n_hi, const uint2 *tab) {
    if constexpr (B > 32 && B <= 64) return nice_count_tab<B>(n_lo, n_hi, tab);
    else return nice_count_fast<B>(n_lo, n_hi);
}
template <int B>
__device__ __forceinline__ void cube_pass(const NiceonlyLaunch &p, const ulonglong2 *q, u32 head, u32 cnt,
                                          u32 lane, const uint2 *tab) {
    wave_sync_lds();  // the queue was written by other lanes of this wave
    if (lane < cnt) {
        const ulonglong2 e = q[(head + lane) & (kCubeQ - 1)];
        if (cube_count<B>(e.x, e.y, tab) >= p.nice_min) emit_nice(p, e.x, e.y);
    }
    wave_sync_lds();
}

// Per-wave candidate state: the exact gi / R of the stride walk and the
// square-survivor ring (head / tail wave-uniform).
struct CandWave {
    u64 r_magic;
    u32 r_shift;
    ulonglong2 *cq;
    const uint2 *tab;  // LDS pair-mask table (PairTab), or unused
    u32 q_head, q_tail;
};
__device__ __forceinline__ CandWave cand_wave(const NiceonlyLaunch &p, ulonglong2 *cq, const uint2 *tab) {
    // gi / R by one 32x32->64 multiply and a shift: gi = g0 + j < R + 2^28 <
    // 2^29 and m = floor(2^s / R) + 1 with s = 30 + ceil(log2 R) keep the error
    // below 2^-(L+1) <= 1/(2R), so the quotient is exact (m < 2^31 + 1).
    const u32 r_log = 32 - __clz(p.R - 1);
    return CandWave{(1ull << (30 + r_log)) / p.R + 1, 30 + r_log, cq, tab, 0, 0};
}

// The stride candidates of LPW leaves (lane l < LPW holds leaf l, the others
// count 0), 64 per round: lane k finds its leaf by a uniform binary search over
// the wave's exclusive prefix (cross-lane reads), rebuilds n = b0 + ((g0 + j) /
// R) * M + residues[(g0 + j) % R] and tests it (client_process.rs:222-253).
// SOUND with the prefix test on: sc->lm is the lane's leaf mask; a rejected
// candidate skips the square test and counts in sc->rej.
template <class G, u32 LPW, bool SOUND>
__device__ __forceinline__ void check_leaf_group(const NiceonlyLaunch &p, const G &g, const Leaf &lf, u32 lane,
                                                 CandWave &cw, SoundCtx<SOUND> *sc) {
    u32 incl = lf.count;
#pragma unroll
    for (int o = 1; o < (int)LPW; o <<= 1) {
        u32 v = __shfl_up(incl, o);
        if (lane >= (u32)o) incl += v;
    }
    const u32 excl = incl - lf.count;
    const u32 total = __shfl(incl, LPW - 1);
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
        const u64 b0lo = __shfl(lf.b0_lo, lo), b0hi = __shfl(lf.b0_hi, lo);
        u64 n_lo = 0, n_hi = 0;
        bool gone = false;  // SOUND: rejected by the prefix test
        [[maybe_unused]] LeafMask mk;
        if constexpr (SOUND && IsConst<G>::value) {
            if (sc->pt) {  // lane lo holds the leaf's mask (read with every lane active)
#pragma unroll
                for (int w = 0; w < 3; w++) mk.w[w] = __shfl(sc->lm.w[w], lo);
                mk.multi = __shfl(sc->lm.multi, lo);
            }
        }
        if (k < total) {
            const u32 gi = g0 + j;
            const u32 cyc = (u32)(((u64)gi * cw.r_magic) >> cw.r_shift);
            const u32 idx = gi - cyc * p.R;
            n_lo = b0lo;
            n_hi = b0hi;
            add_u128(n_lo, n_hi, (u64)cyc * p.M + p.residues[idx]);
            if constexpr (SOUND && IsConst<G>::value) {
                if (sc->pt) {
                    constexpr int MW = Radix<IsConst<G>::base>::MW;
                    u32 pm[MW];
#pragma unroll
                    for (int w = 0; w < MW; w++) pm[w] = mk.w[w];
                    gone = cand_rejected<IsConst<G>::base>(*sc->snd, pm, mk.multi, idx);
                    sc->rej += gone ? 1u : 0u;
                }
            }
        }
        if constexpr (IsConst<G>::value) {
            if (p.in_range) {  // wave-uniform
                // n^2 first; the few survivors queue for a full-wave cube pass
                bool sq = false;
                if (k < total && !gone) {
                    if constexpr (PairTab<G>::on) sq = square_ok_tab<IsConst<G>::base>(n_lo, n_hi, cw.tab);
                    else sq = square_ok<IsConst<G>::base>(n_lo, n_hi);
                }
                const u64 bal = __ballot(sq);
                if (bal) {
                    if (sq) cw.cq[(cw.q_tail + lane_rank(bal)) & (kCubeQ - 1)] = make_ulonglong2(n_lo, n_hi);
                    cw.q_tail += (u32)__popcll(bal);
                    if (cw.q_tail - cw.q_head >= 64) {
                        cube_pass<IsConst<G>::base>(p, cw.cq, cw.q_head, 64, lane, cw.tab);
                        cw.q_head += 64;
                    }
                }
                continue;
            }
        }
        if (k < total && is_nice_dev(n_lo, n_hi, g)) emit_nice(p, n_lo, n_hi);
    }
}

template <class G>
__device__ __forceinline__ void cand_flush(const NiceonlyLaunch &p, CandWave &cw, u32 lane) {
    if constexpr (IsConst<G>::value) {
        if (cw.q_tail != cw.q_head)
            cube_pass<IsConst<G>::base>(p, cw.cq, cw.q_head, cw.q_tail - cw.q_head, lane, cw.tab);
        cw.q_head = cw.q_tail;
    }
}

// This workgroup's square survivors (every wave's cube-queue total) into the
// field's partial counts (kMsdSquareParts, layout.h): one LDS add per wave, one
// global add per workgroup.  Every thread calls it (a barrier inside).
__device__ __forceinline__ void square_ok_flush(u32 *ctr, u32 *wg_sum, u32 waves_total, u32 lane) {
    if (lane == 0 && waves_total) atomicAdd(wg_sum, waves_total);
    __syncthreads();
    if (threadIdx.x == 0 && ctr && *wg_sum) atomicAdd(&ctr[kMsdSquareParts + blockIdx.x % kMsdSquarePartCount], *wg_sum);
}

// End of a niceonly launch (every thread of the workgroup calls it): the last
// workgroup to retire copies the field's results to mapped host memory (the
// count is agent-atomic, so: own atomics drained, barrier, one agent add per
// workgroup -- no L2 write-back fence, see fd2's field_finish).  Field end
// (count_mapped set): the MSD counters and the nice count out, then re-zeroed
// for the slot's next field.  Batch end: only the per-batch leaf-record count
// is re-zeroed, for the next batch.
// SOUND: the prefix test's rejected count (kMsdRejected) goes out to mapped
// words kMsdMappedRejected, +1 and is re-zeroed with the rest.
template <bool SOUND = false>
__device__ __forceinline__ void nice_launch_finish(const NiceFinish &fin, u32 *count) {
    __shared__ u32 last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) last = last_block_arrive(fin.done);
    __syncthreads();
    if (!last) return;
    u32 *ctr = fin.msd_counters;
    const u32 w = threadIdx.x;
    if (fin.count_mapped) {
        if (ctr && w < kMsdSquarePartCount) {  // wave 0
            // the square-survivor partials summed into kMsdSquareOk, then re-zeroed
            u32 part = __hip_atomic_load(&ctr[kMsdSquareParts + w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&ctr[kMsdSquareParts + w], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) part += __shfl_xor(part, o);
            if (w < kMsdSquareParts) {
                const u32 v = __hip_atomic_load(&ctr[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                fin.msd_mapped[w] = w == kMsdSquareOk ? part : v;
                if (w >= kMsdLeafCount) __hip_atomic_store(&ctr[w], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if constexpr (SOUND) {
                if (w >= kMsdMappedRejected && w < kMsdMappedWords) {
                    u32 *rej = &ctr[kMsdRejected - kMsdMappedRejected + w];
                    fin.msd_mapped[w] = __hip_atomic_load(rej, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(rej, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        if (w == 0) {
            *fin.count_mapped = __hip_atomic_load(count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else if (ctr && w == kMsdLeafCount) {
        __hip_atomic_store(&ctr[kMsdLeafCount], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    done_reset(fin.done);
}

template <class G, class... S>
__global__ void __launch_bounds__(256)
niceonly_kernel(NiceonlyLaunch p, G g, S... snd) {
    constexpr bool SOUND = sizeof...(S) != 0;
    const u32 lane = threadIdx.x & 63;
    const u32 gwave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const u32 nwaves = (gridDim.x * blockDim.x) >> 6;
    const u32 n_leaves = p.n_leaves_dev ? min(*p.n_leaves_dev, p.n_leaves) : p.n_leaves;
    __shared__ ulonglong2 cq[4][IsConst<G>::value ? kCubeQ : 1];
    __shared__ uint2 tab[PairTab<G>::N];
    __shared__ u32 sq_sum;
    if (threadIdx.x == 0) sq_sum = 0;
    SoundCtx<SOUND> sc = sound_ctx<G>(p.in_range, snd...);
    pair_tab_fill<G>(tab);  // (ends with a barrier)
    CandWave cw = cand_wave(p, cq[threadIdx.x >> 6], tab);
    // LPW leaves per wave (lanes >= LPW carry count 0): at the CPU path's
    // floor a leaf holds ~40 candidates, so 8 leaves keep a wave ~5 rounds
    // deep and spread a 35k-leaf field over ~4400 waves instead of ~550.
    constexpr u32 LPW = 8;
    for (u32 base = gwave * LPW; base < n_leaves; base += nwaves * LPW) {
        const u32 li = base + lane;
        Leaf lf{0, 0, 0, 0};
        if (lane < LPW && li < n_leaves) lf = p.leaves[li];
        if constexpr (SOUND) {
            sc.lm = LeafMask{{0, 0, 0}, 0};
            if (sc.pt && lane < LPW && li < n_leaves) sc.lm = sc.snd->leaf_masks[li];
        }
        check_leaf_group<G, LPW, SOUND>(p, g, lf, lane, cw, &sc);
    }
    cand_flush<G>(p, cw, lane);
    square_ok_flush(p.fin.msd_counters, &sq_sum, cw.q_tail, lane);
    if constexpr (SOUND) {
        if (sc.pt) rejected_flush(sc.snd->rejected, sc.rej);
    }
    if (p.fin.done) nice_launch_finish<SOUND>(p.fin, p.out.count);
}

}  // namespace nice
