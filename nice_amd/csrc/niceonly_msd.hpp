// niceonly_msd.hpp -- the device MSD filter of niceonly field processing: the
// node rule of the recursion (msd_prefix_filter.rs:382-674), a leaf's stride
// descriptor, and the two kernels that write leaves to a batch's leaf list
// for niceonly_kernel (niceonly_cand.hpp has the overview of all four).
#pragma once

#include "niceonly_cand.hpp"

namespace nice {

// ---------------------------------------------------------------------------
// Device MSD filter
// ---------------------------------------------------------------------------

// u128 {lo, hi} divided by a u32 (q written back), returns the remainder.
__device__ __forceinline__ u32 divmod_u128(u64 &lo, u64 &hi, u32 d) {
    u32 w[4] = {(u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32)};
    u64 rem = 0;
#pragma unroll
    for (int i = 3; i >= 0; i--) {
        u64 cur = (rem << 32) | w[i];
        w[i] = (u32)(cur / d);
        rem = cur - (u64)w[i] * d;
    }
    lo = ((u64)w[1] << 32) | w[0];
    hi = ((u64)w[3] << 32) | w[2];
    return (u32)rem;
}

__device__ __forceinline__ bool overlaps(const Mask<4> &a, const Mask<4> &b) {
    return ((a.w[0] & b.w[0]) | (a.w[1] & b.w[1]) | (a.w[2] & b.w[2]) | (a.w[3] & b.w[3])) != 0;
}

// Common most-significant-digit prefix of x and y (both consumed), in one
// least-significant-first pass over both, without storing digits: the running
// mask holds the digits seen since the last position where x and y differed,
// and is snapshotted at every non-zero digit of x, so after the pass the
// snapshot is the mask of the common prefix of the two numbers.  Returns false
// if the digit counts differ; lsd0/lsd1 are x's two lowest digits.
struct PrefixScan {
    Mask<4> mask;
    u32 dup;
    u32 lsd0, lsd1;
    int len;
};
template <int NW, class G>
__device__ __forceinline__ bool common_prefix(u32 (&x)[NW], u32 (&y)[NW], const G &g,
                                              PrefixScan &r) {
    int tx = top_word(x), ty = top_word(y);
    Mask<4> cur;
    cur.clear();
    r.mask.clear();
    u32 dup = 0;
    r.dup = 0;
    r.lsd0 = r.lsd1 = 0;
    int pos = 0, lx = 0, ly = 0;
    while (tx >= 0 || ty >= 0) {
        u32 cx = tx >= 0 ? div_chunk<NW>(x, tx, g.D) : 0u;
        u32 cy = ty >= 0 ? div_chunk<NW>(y, ty, g.D) : 0u;
        for (u32 q = 0; q < g.E; q++, pos++) {
            const u32 dx = cx % g.base, dy = cy % g.base;
            cx /= g.base;
            cy /= g.base;
            if (pos == 0) r.lsd0 = dx;
            if (pos == 1) r.lsd1 = dx;
            if (dx != dy) {
                cur.clear();
                dup = 0;
            } else {
                dup |= cur.test_set(dx);
            }
            if (dx) {
                lx = pos + 1;
                r.mask = cur;
                r.dup = dup;
            }
            if (dy) ly = pos + 1;
        }
    }
    r.len = lx;
    return lx == ly;
}

// has_duplicate_msd_prefix (msd_prefix_filter.rs:382-563) on [first, last].
// SOUND: without Filter C.
template <class G, bool SOUND = false>
__device__ bool msd_skippable(u64 f_lo, u64 f_hi, u64 l_lo, u64 l_hi, const G &g) {
    u32 fn[4] = {(u32)f_lo, (u32)(f_lo >> 32), (u32)f_hi, (u32)(f_hi >> 32)};
    u32 ln[4] = {(u32)l_lo, (u32)(l_lo >> 32), (u32)l_hi, (u32)(l_hi >> 32)};
    u32 fsq[8], lsq[8];
    mul_words<4, 4>(fn, fn, fsq);
    mul_words<4, 4>(ln, ln, lsq);
    u32 fcu[12], lcu[12];
    mul_words<8, 4>(fsq, fn, fcu);
    mul_words<8, 4>(lsq, ln, lcu);
    PrefixScan sq, cu;
    if (!common_prefix<8>(fsq, lsq, g, sq)) return false;  // digit counts differ
    if (sq.dup) return true;
    if (!common_prefix<12>(fcu, lcu, g, cu)) return false;
    if (cu.dup) return true;
    if (overlaps(sq.mask, cu.mask)) return true;
    if constexpr (SOUND) return false;
    // Filter C (MSD_LSD_OVERLAP_K_VALUE = 2): first / b^2 == last / b^2, with
    // *first*'s two lowest digits of n^2 and n^3 (msd_prefix_filter.rs:461-559).
    u64 a_lo = f_lo, a_hi = f_hi, b_lo = l_lo, b_hi = l_hi;
    divmod_u128(a_lo, a_hi, g.base * g.base);
    divmod_u128(b_lo, b_hi, g.base * g.base);
    if (a_lo == b_lo && a_hi == b_hi) {
        Mask<4> ms, mc;
        ms.clear();
        mc.clear();
        u32 ds = 0, dc = 0;
        if (sq.len > 0) ds |= ms.test_set(sq.lsd0);
        if (sq.len > 1) ds |= ms.test_set(sq.lsd1);
        if (cu.len > 0) dc |= mc.test_set(cu.lsd0);
        if (cu.len > 1) dc |= mc.test_set(cu.lsd1);
        if (overlaps(sq.mask, ms) || overlaps(cu.mask, mc) || overlaps(sq.mask, mc) ||
            overlaps(cu.mask, ms) || ds || dc || overlaps(ms, mc))
            return true;
    }
    return false;
}

// Stride-index descriptor of [a, a + size): cycle base b0 = a - a mod M,
// first residue index g0 and candidate count (stride_filter.rs:99-155).
struct LeafDesc {
    u64 b0_lo, b0_hi, count;
    u32 g0;
};
// x = hi 2^64 + lo (hi < 2^32) divided by the constant MC < 2^20: two u64
// divisions by a constant (the quotient fits a u64), returns x mod MC.
template <u32 MC>
__device__ __forceinline__ u32 divmod_wide(u64 lo, u64 hi, u64 &q) {
    static_assert(MC != 0 && MC < (1u << kWideG0Bits), "stride modulus");
    const u64 c1 = (hi << 32) | (lo >> 32);
    const u64 q1 = c1 / MC;
    const u64 c0 = ((c1 - q1 * MC) << 32) | (u32)lo;
    const u64 q0 = c0 / MC;
    q = (q1 << 32) + q0;
    return (u32)(c0 - q0 * MC);
}

template <u32 MC, bool WIDE = false>
__device__ __forceinline__ LeafDesc leaf_desc(u64 a_lo, u64 a_hi, u64 size, const MsdLaunch &p) {
    if constexpr (MC != 0 && WIDE) {
        // In-range b57..64 (n < 2^76): the same with a u128 start.
        u64 e_lo = a_lo, e_hi = a_hi;
        add_u128(e_lo, e_hi, size);
        u64 qa, qe;
        const u32 ra = divmod_wide<MC>(a_lo, a_hi, qa), re = divmod_wide<MC>(e_lo, e_hi, qe);
        const u32 g0 = p.ranks[ra], g1 = p.ranks[re];
        return LeafDesc{a_lo - ra, a_hi - (a_lo < ra ? 1 : 0), (qe - qa) * p.R + g1 - g0, g0};
    } else if constexpr (MC != 0) {
        // In-range two-word bases whose n fit 64 bits (b40..54) with the k = 2
        // stride modulus as a compile-time constant: u64 divisions by a
        // constant.
        const u64 a = a_lo, e = a_lo + size;
        const u64 qa = a / MC, qe = e / MC;
        const u32 ra = (u32)(a - qa * MC), re = (u32)(e - qe * MC);
        const u32 g0 = p.ranks[ra], g1 = p.ranks[re];
        return LeafDesc{a - ra, 0, (qe - qa) * p.R + g1 - g0, g0};
    }
    u64 q_lo = a_lo, q_hi = a_hi;
    const u32 ra = divmod_u128(q_lo, q_hi, p.M);
    u64 e_lo = a_lo, e_hi = a_hi;
    add_u128(e_lo, e_hi, size);
    u64 qe_lo = e_lo, qe_hi = e_hi;
    const u32 re = divmod_u128(qe_lo, qe_hi, p.M);
    const u32 g0 = p.ranks[ra], g1 = p.ranks[re];
    // cycles between the two ends (< 2^64 / M for any batch)
    const u64 count = (qe_lo - q_lo) * p.R + g1 - g0;
    u64 b0_lo = a_lo, b0_hi = a_hi;
    b0_hi -= (b0_lo < ra) ? 1 : 0;  // b0 = a - ra (u128 minus u32)
    b0_lo -= ra;
    return LeafDesc{b0_lo, b0_hi, count, g0};
}

// Sum over the wave (every lane calls it).
__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Reserve `mine` slots per thread of a 256-thread workgroup with ONE atomic
// per workgroup (same-address atomics from every wave of the chip serialise in
// L2: ~1000 per level cost ~40 us).  All threads must call it; `slots` is 4
// words of LDS.  Returns this thread's first slot.
__device__ __forceinline__ u32 block_reserve(u32 *ctr, u32 mine, u32 *slots) {
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u32 v = __shfl_up(incl, o);
        if (lane >= (u32)o) incl += v;
    }
    if (lane == 63) slots[wave] = incl;
    __syncthreads();
    u32 before = 0, total = 0;
#pragma unroll
    for (u32 w = 0; w < 4; w++) {
        const u32 t = slots[w];
        before += w < wave ? t : 0u;
        total += t;
    }
    __syncthreads();
    if (threadIdx.x == 0) slots[0] = total ? atomicAdd(ctr, total) : 0u;
    __syncthreads();
    const u32 base = slots[0];
    __syncthreads();
    return base + before + incl - mine;
}

// The recursion's rule for one node (msd_prefix_filter.rs:583-658):
// 0 = dropped (has_duplicate_msd_prefix), 1 = leaf, 2 = split in two.
// SOUND: no Filter C; with the prefix test on a leaf's mask goes to sc->lm --
// also for the leaves made without a skip test (size <= floor on entry, depth
// 22), which still count as ranges while every candidate of theirs goes when
// their prefix repeats.
template <class G, bool TAB, bool SOUND>
__device__ __forceinline__ u32 classify_node(const MsdLaunch &p, u32 level, u64 lo, u64 hi, u64 size,
                                             const G &g, const uint2 *tab, SoundCtx<SOUND> *sc) {
    bool leaf = level >= 22 || size <= p.floor_size;
    if constexpr (SOUND && IsConst<G>::value) {
        if (sc->pt) {
            LeafMask *lm = &sc->lm;
            *lm = LeafMask{{0, 0, 0}, size > 1 ? 1u : 0u};
            if (size <= 1) return 1;
            u64 l_lo = lo, l_hi = hi;
            add_u128(l_lo, l_hi, size - 1);
            constexpr int MW = Radix<IsConst<G>::base>::MW;
            u32 pm[MW];
            const u32 dup = msd_prefix_masks<IsConst<G>::base, TAB>(lo, hi, l_lo, l_hi, pm, tab);
#pragma unroll
            for (int w = 0; w < MW; w++) lm->w[w] = dup ? ~0u : pm[w];
            if (leaf) return 1;
            if (dup && !(kProbes && (p.probe & 1))) return 0;
            return size < 2 * p.floor_size ? 1u : 2u;
        }
    }
    if (leaf) return 1;
    u64 l_lo = lo, l_hi = hi;
    add_u128(l_lo, l_hi, size - 1);
    const bool no_skip_test = kProbes && (p.probe & 1);
    bool skip = false;
    if (size != 1 && !no_skip_test) {
        if constexpr (IsConst<G>::value) {
            if constexpr (SOUND) {
                u32 pm[Radix<IsConst<G>::base>::MW];
                skip = p.in_range ? msd_prefix_masks<IsConst<G>::base, TAB>(lo, hi, l_lo, l_hi, pm, tab) != 0
                                  : msd_skippable<G, true>(lo, hi, l_lo, l_hi, g);
            } else {
                skip = p.in_range ? msd_skippable_fast<IsConst<G>::base, TAB>(lo, hi, l_lo, l_hi, tab)
                                  : msd_skippable<G>(lo, hi, l_lo, l_hi, g);
            }
        } else {
            skip = msd_skippable<G, SOUND>(lo, hi, l_lo, l_hi, g);
        }
    }
    if (skip) return 0;
    return size < 2 * p.floor_size ? 1u : 2u;
}

// A leaf's stride-index records (one per kLeafPiece candidates; a range
// without candidates still counts as an MSD-surviving range, none stored),
// appended with one atomic per workgroup; statistics accumulated per lane.
// Every thread of the workgroup calls it (act == 1: this lane has a leaf).
// masks (SoundCtx::mask_list: sound variants with the prefix test on, else
// null): the leaf's mask *lm beside each of its records.
template <u32 MC, bool WIDE>
__device__ __forceinline__ void append_leaf(const MsdLaunch &p, u32 act, u64 lo, u64 hi, u64 size,
                                            u32 *slots, u64 &n_st, u64 &c_st, u64 &s_st,
                                            LeafMask *masks, const LeafMask *lm) {
    LeafDesc ld{0, 0, 0, 0};
    if (kProbes && act == 1 && (p.probe & 2)) {
        ld = LeafDesc{lo, hi, size, 0};
    } else
    if (act == 1) {
        ld = leaf_desc<MC, WIDE>(lo, hi, size, p);
    }
    const u64 pieces64 = act == 1 ? (ld.count + kLeafPiece - 1) / kLeafPiece : 0;
    const u32 pieces = pieces64 > 0xffffu ? 0xffffu : (u32)pieces64;
    const u32 pos = block_reserve(&p.counters[kMsdLeafCount], pieces, slots);
    if (act != 1) return;
    if (pieces64 > 0xffffu || (u64)pos + pieces > p.leaf_cap) {
        atomicOr(&p.counters[kMsdOverflow], 1u);
    } else {
        u64 b0_lo = ld.b0_lo, b0_hi = ld.b0_hi;
        u64 gi = ld.g0;  // residue-sequence index relative to b0
        for (u32 q = 0; q < pieces; q++) {
            if (gi >= p.R) {  // re-base: g0 < R keeps the kernel's index 32-bit
                const u64 cyc = gi / p.R;
                add_u128(b0_lo, b0_hi, cyc * p.M);
                gi -= cyc * p.R;
            }
            const u64 left = ld.count - (u64)q * kLeafPiece;
            const u32 cnt = left < kLeafPiece ? (u32)left : kLeafPiece;
            p.leaves[pos + q] = Leaf{b0_lo, b0_hi, (u32)gi, cnt};
            if (masks) masks[pos + q] = *lm;
            gi += cnt;
        }
    }
    n_st++;
    c_st += ld.count;
    s_st += size;
}

// Workgroup statistics -> the sticky counters, one atomic each.
__device__ __forceinline__ void flush_stats(const MsdLaunch &p, u64 n_st, u64 c_st, u64 s_st,
                                            unsigned long long *stat) {
    const u32 lane = threadIdx.x & 63;
    n_st = wave_sum(n_st);
    c_st = wave_sum(c_st);
    s_st = wave_sum(s_st);
    __syncthreads();
    if (lane == 0 && n_st) {
        atomicAdd(&stat[0], (unsigned long long)n_st);
        atomicAdd(&stat[1], (unsigned long long)c_st);
        atomicAdd(&stat[2], (unsigned long long)s_st);
    }
    __syncthreads();
    if (threadIdx.x == 0 && stat[0]) {
        atomicAdd(&p.counters[kMsdRanges], (u32)stat[0]);
        atomicAdd((unsigned long long *)(p.counters + kMsdCandidates), stat[1]);
        atomicAdd((unsigned long long *)(p.counters + kMsdNumbers), stat[2]);
    }
}

template <class G, u32 MC, class... S>
__global__ void __launch_bounds__(256)
msd_level_kernel(MsdLaunch p, u32 level, G g, S... snd) {
    constexpr bool SOUND = sizeof...(S) != 0;
    __shared__ u32 slots[4];
    __shared__ unsigned long long stat[3];
    if (threadIdx.x < 3) stat[threadIdx.x] = 0;
    const MsdNode *qin = p.q[level & 1];
    MsdNode *qout = p.q[(level + 1) & 1];
    // (an overflowed level leaves its count above the queue: flagged, and
    // never read past)
    const u32 n_in = min(p.counters[level], p.q_cap);
    // Workgroup-uniform loop: leaves and children are appended with one atomic
    // per workgroup, statistics summed in LDS and added once at the end.
    const u32 stride = gridDim.x * blockDim.x;
    SoundCtx<SOUND> sc = sound_ctx<G>(p.in_range, snd...);
    u64 n_st = 0, c_st = 0, s_st = 0;
    for (u32 b0 = blockIdx.x * blockDim.x; b0 < n_in; b0 += stride) {
        const u32 i = b0 + threadIdx.x;
        u32 act = 0;  // 0 drop / idle, 1 leaf, 2 split
        MsdNode nd{0, 0};
        u64 lo = p.start_lo, hi = p.start_hi;
        if (i < n_in) {
            nd = qin[i];
            add_u128(lo, hi, nd.off);
            act = classify_node<G, false, SOUND>(p, level, lo, hi, nd.size, g, nullptr, &sc);
        }
        append_leaf<MC, WideN<G>::value>(p, act, lo, hi, nd.size, slots, n_st, c_st, s_st, sc.mask_list(), sc.mask());
        // children
        const u32 cpos = block_reserve(&p.counters[level + 1], act == 2 ? 2u : 0u, slots);
        if (act == 2) {
            if (cpos + 1 >= p.q_cap) {
                atomicOr(&p.counters[kMsdOverflow], 1u);
            } else {
                const u64 half = nd.size / 2;
                qout[cpos] = MsdNode{nd.off, half};
                qout[cpos + 1] = MsdNode{nd.off + half, nd.size - half};
            }
        }
    }
    flush_stats(p, n_st, c_st, s_st, stat);
}

// The whole recursion of a chunk in ONE workgroup, level by level with
// workgroup barriers, for chunks whose levels fit `cap` nodes (at most
// chunk / floor: a node splits only if it holds >= 2 floor numbers).  A
// batch is then ONE launch instead of init + up to 23 level launches --
// each of those waited for free CUs behind the detailed kernel that runs
// beside it, and their grids were sized for the unpruned tree.  Nodes are
// (offset in the chunk, size) pairs in a per-workgroup ping-pong queue in
// global memory (`scratch`: gridDim.x x 2 x cap).
template <class G, u32 MC, class... S>
__global__ void __launch_bounds__(256)
msd_fused_kernel(MsdLaunch p, ChunkNode *scratch, u32 cap, G g, S... snd) {
    constexpr bool SOUND = sizeof...(S) != 0;
    __shared__ u32 slots[4];
    __shared__ u32 cnt[2];
    __shared__ unsigned long long stat[3];
    if (threadIdx.x < 3) stat[threadIdx.x] = 0;
    ChunkNode *qa = scratch + (u64)blockIdx.x * 2 * cap, *qb = qa + cap;
    SoundCtx<SOUND> sc = sound_ctx<G>(p.in_range, snd...);
    u64 n_st = 0, c_st = 0, s_st = 0;
    for (u64 ci = blockIdx.x; ci < p.nchunks; ci += gridDim.x) {
        const u64 c = p.deal_offset + (p.first + ci) * p.deal_stride;
        u64 clo = p.start_lo, chi = p.start_hi;
        add_u128(clo, chi, c * p.chunk);
        const u64 rem_lo = p.end_lo - clo;
        const u64 rem_hi = p.end_hi - chi - (p.end_lo < clo ? 1 : 0);
        const u32 csize = (u32)(rem_hi || rem_lo > p.chunk ? p.chunk : rem_lo);
        if (threadIdx.x == 0) {
            qa[0] = ChunkNode{0u, csize};
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
                u64 lo = clo, hi = chi;
                if (i < n_in) {
                    nd = qin[i];
                    add_u128(lo, hi, nd.off);
                    act = classify_node<G, false, SOUND>(p, level, lo, hi, nd.size, g, nullptr, &sc);
                }
                append_leaf<MC, WideN<G>::value>(p, act, lo, hi, nd.size, slots, n_st, c_st, s_st, sc.mask_list(),
                                                 sc.mask());
                if (act == 2) {
                    const u32 cp = atomicAdd(&cnt[1], 2u);
                    if (cp + 2 > cap) {
                        atomicOr(&p.counters[kMsdOverflow], 1u);
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
        __syncthreads();  // the queues are reused by the next chunk
    }
    flush_stats(p, n_st, c_st, s_st, stat);
}

}  // namespace nice
