// niceonly_wave.hpp -- msd_wave_kernel: the device MSD recursion below a root
// level and the candidate test of its leaves in one launch, for chunks too
// large for msd_fused_kernel (niceonly_cand.hpp has the overview of all four
// headers).
#pragma once

#include "niceonly_msd.hpp"

namespace nice {

// MSD recursion and candidate test fused, one wave per subtree stream, for
// chunks too large for msd_fused_kernel (the massive field's 1e8 chunks).
// The level BFS above it runs only the first few levels (until a batch has
// tens of thousands of nodes of <= 2^26 numbers); each wave then takes those
// roots grid-strided and recurses with a wave-private work stack in global
// memory: pop up to 64 nodes (one per lane), classify (the reference's node
// rule), push the split nodes' halves.  The stack is topped up with fresh
// roots whenever it holds fewer than 64 nodes, so lanes stay busy across
// small subtrees.  Leaves never leave the wave: their stride descriptors queue
// in LDS and are tested 64 at a time by the candidate code above (square
// first, cube on a full wave of survivors).  No leaf list, no level launches
// below the roots, and no same-address atomic per level iteration: the level
// BFS spent most of its 85 ms on the massive field in launches and in the
// L2-serialised queue and statistics atomics of ~10^4 small launches.
struct StackNode {
    u64 off;    // from the field start
    u32 size;   // <= 2^26 (the host picks the root level for it)
    u32 depth;  // recursion level (the reference's depth, <= 22)
};
// (kWaveWG threads per workgroup, a work stack of kStackCap nodes per wave:
// layout.h, where the host sizes the stacks.)
static_assert(sizeof(StackNode) == kStackNodeBytes, "msd_wave_scratch_bytes (msd_plan.hpp) sizes the work stacks");
// Leaf-descriptor queue per wave: tested 64 at a time, in groups of 16.
constexpr u32 kLeafQ = 128, kLeafGroup = 16;

// Lane walk (two-word in-range bases: the wave kernel's const-modulus
// instantiations).  Each lane takes one leaf from the wave's
// queue and tests one of its candidates per round, stepping the residue index
// (no division, no search) and taking the next queued leaf when its own runs
// out.  The packed walk of check_leaf_group spends ~10 cross-lane reads per
// round locating each lane's leaf (a binary search over the group's prefix,
// then the leaf's fields).  Queue entries are 16 bytes; the queue is walked
// once it holds kWalkAt leaves (>= 3 per lane, so lanes rarely idle at the
// end).  Massive field: 0.0688 -> 0.0652 s.  (Loading the next round's
// residue ahead of the current test gained nothing, and stepping the limbs by
// the residue gaps instead of converting n lost 7 %: 0.0696 s.)
// WIDE (b57..64, n past 64 bits): the entry stays 16 bytes -- the cycle base's
// high part (< 2^kWideHiBits) rides above g0 (<= R < 2^kWideG0Bits) -- and
// each lane steps its cycle base by M with a carry into the high part.
struct LeafW {
    u64 b0;
    u32 g0, count;  // WIDE: g0 | b0's high part << kWideG0Bits
};
constexpr u32 kWalkQ = 256;
// b64's pair table is 32 KB: with a 256-entry walk queue per wave the
// workgroup passes 80 KB and only one fits a CU, so its queue is half as long.
template <class G>
constexpr u32 walk_q() { return PairTab<G>::N * 8 + 8 * (kCubeQ + kWalkQ) * 16 + 512 <= 80 * 1024 ? kWalkQ : kWalkQ / 2; }
// Sound variants: a queued leaf also holds its 8-byte prefix mask (24 bytes),
// which leaves 256 entries only to b40..45; the others walk 128, as b64 does
// anyway, and two workgroups still fit a CU.
template <class G>
constexpr u32 walk_q_sound() {
    return PairTab<G>::N * 8 + 8 * (kCubeQ * 16 + kWalkQ * 24) + 512 <= 80 * 1024 ? kWalkQ : kWalkQ / 2;
}
// LDS of a sound variant only (a block-scope array would also grow the
// reference filter's instantiations).
template <class T, u32 N>
__device__ __forceinline__ T *lds_array() {
    __shared__ T a[N];
    return a;
}

// SOUND: bit 31 of a leaf's count says it holds >= 2 numbers; with the prefix
// test on, qm holds the queued leaves' prefix masks and a lane steps its
// residue index past the candidates the test rejects (counted in sc->rej)
// before it joins the round, so the square test runs on survivors only.
template <int B, bool WIDE, u32 Q, bool SOUND>
__device__ __forceinline__ void walk_leaves(const NiceonlyLaunch &c, const LeafW *q, u32 head, u32 n, u32 lane,
                                            CandWave &cw, SoundCtx<SOUND> *sc, const uint2 *qm) {
    wave_sync_lds();  // queue entries written by other lanes
    u32 taken = 0;    // wave-uniform
    bool have = false;
    u64 cb = 0;  // the candidate's cycle base b0 + k M
    u32 cbh = 0;  // WIDE: its high part
    u32 idx = 0, left = 0;
    for (;;) {
        const u64 need = __ballot(!have);
        if (need && taken < n) {  // lanes without a leaf take the next ones
            const u32 r = lane_rank(need);
            if (!have && taken + r < n) {
                const LeafW e = q[(head + taken + r) & (Q - 1)];
                cb = e.b0;
                idx = e.g0;
                if constexpr (WIDE) {
                    cbh = idx >> kWideG0Bits;
                    idx &= (1u << kWideG0Bits) - 1;
                }
                left = e.count;
                if constexpr (SOUND) {
                    sc->lm.multi = left >> 31;
                    left &= 0x7fffffffu;
                    if (sc->pt) {
                        const uint2 m = qm[(head + taken + r) & (Q - 1)];
                        sc->lm.w[0] = m.x;
                        sc->lm.w[1] = m.y;
                    }
                }
                if (idx >= c.R) {  // g0 == R: the first candidate is in the next cycle
                    idx -= c.R;
                    cb += c.M;
                    if constexpr (WIDE) cbh += cb < c.M ? 1u : 0u;
                }
                have = left != 0;
            }
            const u32 np = (u32)__popcll(need);
            taken = n - taken > np ? taken + np : n;
        }
        if constexpr (SOUND) {
            if (sc->pt) {
                const u32 pm[2] = {sc->lm.w[0], sc->lm.w[1]};
                while (have && cand_rejected<B>(*sc->snd, pm, sc->lm.multi, idx)) {
                    sc->rej++;
                    if (++idx == c.R) {
                        idx = 0;
                        cb += c.M;
                        if constexpr (WIDE) cbh += cb < c.M ? 1u : 0u;
                    }
                    have = --left != 0;
                }
            }
        }
        if (!__ballot(have)) {
            if (taken >= n) break;
            continue;
        }
        u64 nv = 0, nvh = 0;
        bool sq = false;
        if (have) {
            nv = cb + c.residues[idx];
            if constexpr (WIDE) nvh = (u64)cbh + (nv < cb ? 1u : 0u);
            sq = square_ok_tab<B>(nv, nvh, cw.tab);
            if (++idx == c.R) {
                idx = 0;
                cb += c.M;
                if constexpr (WIDE) cbh += cb < c.M ? 1u : 0u;
            }
            have = --left != 0;
        }
        const u64 nv_sq = nv;
        const u64 bal = __ballot(sq);
        if (bal) {
            if (sq) cw.cq[(cw.q_tail + lane_rank(bal)) & (kCubeQ - 1)] = make_ulonglong2(nv_sq, nvh);
            cw.q_tail += (u32)__popcll(bal);
            if (cw.q_tail - cw.q_head >= 64) {
                cube_pass<B>(c, cw.cq, cw.q_head, 64, lane, cw.tab);
                cw.q_head += 64;
            }
        }
    }
    wave_sync_lds();
}

// 4 waves per SIMD (<= 128 VGPRs) where the base's limb arrays allow it
// without spilling; the three-word paths (b65, b68, b80) need ~190-220.
// b57..64 at 4 waves carry 64-128 B of scratch per lane (b54: 16-32 B), at
// NICE_WIDE_WAVES = 3 (<= 168 VGPRs) none: the A/B of
// scripts/niceonly_bases_ab.py builds both (DESIGN 3.4 has the table).
#ifndef NICE_WIDE_WAVES
#define NICE_WIDE_WAVES 4
#endif
template <class G>
constexpr int wave_occupancy() {
    return IsConst<G>::value && IsConst<G>::base > 64 ? 2 : (WideN<G>::value ? NICE_WIDE_WAVES : 4);
}

template <class G, u32 MC, class... S>
__global__ void __launch_bounds__(kWaveWG) __attribute__((amdgpu_waves_per_eu(wave_occupancy<G>())))
msd_wave_kernel(MsdLaunch p, NiceonlyLaunch c, u32 level0, StackNode *scratch, G g, S... snd) {
    constexpr bool SOUND = sizeof...(S) != 0;
    constexpr u32 W = kWaveWG / 64;
    constexpr bool WALK = PairTab<G>::on && MC != 0;  // lane walk (see walk_leaves)
    constexpr bool WIDE = WALK && WideN<G>::value;
    // (a round queues <= 64 leaves on top of fewer than kWalkAt: 192 of 256, b64 64 of 128)
    constexpr u32 kWalkQ = SOUND ? walk_q_sound<G>() : walk_q<G>(), kWalkAt = kWalkQ - 64;
    __shared__ ulonglong2 cq[W][IsConst<G>::value ? kCubeQ : 1];
    __shared__ Leaf lq[W][WALK ? 1 : kLeafQ];
    __shared__ LeafW lw[W][WALK ? kWalkQ : 1];
    __shared__ uint2 tab[PairTab<G>::N];
    __shared__ unsigned long long stat[3];
    __shared__ u32 sq_sum;
    if (threadIdx.x < 3) stat[threadIdx.x] = 0;
    if (threadIdx.x == 0) sq_sum = 0;
    pair_tab_fill<G>(tab);  // (ends with a barrier)
    const u32 lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const u64 gwave = (u64)blockIdx.x * W + wv, nwaves = (u64)gridDim.x * W;
    StackNode *st = scratch + gwave * kStackCap;
    Leaf *q = lq[wv];
    LeafW *qw = lw[wv];
    CandWave cw = cand_wave(c, cq[wv], tab);
    u64 n_st = 0, c_st = 0, s_st = 0;
    // SOUND: the queued leaves' prefix masks beside lw / lq
    SoundCtx<SOUND> sc = sound_ctx<G>(p.in_range, snd...);
    [[maybe_unused]] uint2 *qwm = nullptr;
    [[maybe_unused]] LeafMask *qm = nullptr;
    if constexpr (SOUND && WALK) qwm = lds_array<uint2, W * kWalkQ>() + wv * kWalkQ;
    else if constexpr (SOUND) qm = lds_array<LeafMask, W * kLeafQ>() + wv * kLeafQ;

    // Leaves the BFS levels above produced (clipped or depth-limited nodes):
    // already stride descriptors in the batch's leaf list.
    const u32 n_list = min(p.counters[kMsdLeafCount], p.leaf_cap);
    for (u64 b = gwave * kLeafGroup; b < n_list; b += nwaves * kLeafGroup) {
        Leaf lf{0, 0, 0, 0};
        if (lane < kLeafGroup && b + lane < n_list) lf = p.leaves[b + lane];
        if constexpr (SOUND) {
            sc.lm = LeafMask{{0, 0, 0}, 0};
            if (sc.pt && lane < kLeafGroup && b + lane < n_list) sc.lm = sc.snd->leaf_masks[b + lane];
        }
        check_leaf_group<G, kLeafGroup, SOUND>(c, g, lf, lane, cw, &sc);
    }

    const MsdNode *roots = p.q[level0 & 1];
    const u64 n_roots = min(p.counters[level0], p.q_cap);
    u64 next = gwave;    // next root of this wave (grid-strided)
    u32 sp = 0;          // stack depth (wave-uniform)
    u32 lq_head = 0, lq_tail = 0;
    for (;;) {
        if (sp < 64 && next < n_roots) {  // top up with roots
            const u64 ri = next + (u64)lane * nwaves;
            const bool ok = lane < 64 - sp && ri < n_roots;
            if (ok) {
                const MsdNode r = roots[ri];
                st[sp + lane] = StackNode{r.off, (u32)r.size, level0};
            }
            const u32 got = (u32)__popcll(__ballot(ok));
            next += (u64)got * nwaves;
            sp += got;
            wave_sync_global();
        }
        if (sp == 0) break;
        const u32 cnt = sp < 64 ? sp : 64;
        sp -= cnt;
        StackNode nd{0, 0, 0};
        if (lane < cnt) nd = st[sp + lane];
        wave_sync_global();  // popped before the pushes below reuse the slots
        u64 lo = p.start_lo, hi = p.start_hi;
        add_u128(lo, hi, nd.off);
        const u32 act = lane < cnt ? classify_node<G, PairTab<G>::on, SOUND>(p, nd.depth, lo, hi, nd.size, g, tab, &sc) : 0u;
        // a leaf: its stride descriptor to the queue (statistics as the
        // reference counts them: every MSD-surviving range)
        LeafDesc ld{0, 0, 0, 0};
        if (act == 1) {
            ld = leaf_desc<MC, WIDE>(lo, hi, nd.size, p);
            n_st++;
            c_st += ld.count;
            s_st += nd.size;
        }
        const bool put = act == 1 && ld.count != 0 && !(kProbes && (p.probe & 4));  // probe 4: MSD only
        const u64 bl = __ballot(put);
        if (put) {
            if constexpr (SOUND) {
                // bit 31 of a walk entry's count: the leaf holds >= 2 numbers
                if constexpr (WALK) {
                    ld.count |= sc.pt ? sc.lm.multi << 31 : 0u;
                    qwm[(lq_tail + lane_rank(bl)) & (kWalkQ - 1)] = make_uint2(sc.lm.w[0], sc.lm.w[1]);
                } else {
                    qm[(lq_tail + lane_rank(bl)) & (kLeafQ - 1)] = sc.lm;
                }
            }
            if constexpr (WIDE)
                qw[(lq_tail + lane_rank(bl)) & (kWalkQ - 1)] =
                    LeafW{ld.b0_lo, ld.g0 | (u32)ld.b0_hi << kWideG0Bits, (u32)ld.count};
            else if constexpr (WALK) qw[(lq_tail + lane_rank(bl)) & (kWalkQ - 1)] = LeafW{ld.b0_lo, ld.g0, (u32)ld.count};
            else q[(lq_tail + lane_rank(bl)) & (kLeafQ - 1)] = Leaf{ld.b0_lo, ld.b0_hi, ld.g0, (u32)ld.count};
        }
        lq_tail += (u32)__popcll(bl);
        // a split: both halves on the stack, one level deeper
        const u64 bs = __ballot(act == 2);
        const u32 nsplit = (u32)__popcll(bs);
        if (sp + 2 * nsplit > kStackCap) {
            if (lane == 0) atomicOr(&p.counters[kMsdOverflow], 1u);  // reported as an error by the host
        } else {
            if (act == 2) {
                const u32 r = sp + 2 * lane_rank(bs), half = nd.size / 2;
                st[r] = StackNode{nd.off, half, nd.depth + 1};
                st[r + 1] = StackNode{nd.off + half, nd.size - half, nd.depth + 1};
            }
            sp += 2 * nsplit;
        }
        wave_sync_global();
        // test queued leaves: the lane walk once kWalkAt are queued, else 64
        // at a time in packed groups
        if constexpr (WALK) {
            if (lq_tail - lq_head >= kWalkAt) {
                walk_leaves<IsConst<G>::base, WIDE, kWalkQ, SOUND>(c, qw, lq_head, lq_tail - lq_head, lane, cw, &sc, qwm);
                lq_head = lq_tail;
            }
        } else if (lq_tail - lq_head >= 64) {
            wave_sync_lds();
            for (u32 gq = 0; gq < 64; gq += kLeafGroup) {
                Leaf lf{0, 0, 0, 0};
                if (lane < kLeafGroup) lf = q[(lq_head + gq + lane) & (kLeafQ - 1)];
                if constexpr (SOUND) {
                    if (lane < kLeafGroup) sc.lm = qm[(lq_head + gq + lane) & (kLeafQ - 1)];
                }
                check_leaf_group<G, kLeafGroup, SOUND>(c, g, lf, lane, cw, &sc);
            }
            lq_head += 64;
        }
    }
    wave_sync_lds();
    if constexpr (WALK) {
        if (lq_head != lq_tail)
            walk_leaves<IsConst<G>::base, WIDE, kWalkQ, SOUND>(c, qw, lq_head, lq_tail - lq_head, lane, cw, &sc, qwm);
        lq_head = lq_tail;
    }
    while (lq_head != lq_tail) {
        const u32 n = lq_tail - lq_head < kLeafGroup ? lq_tail - lq_head : kLeafGroup;
        Leaf lf{0, 0, 0, 0};
        if (lane < n) lf = q[(lq_head + lane) & (kLeafQ - 1)];
        if constexpr (SOUND) {
            if (lane < n) sc.lm = qm[(lq_head + lane) & (kLeafQ - 1)];
        }
        check_leaf_group<G, kLeafGroup, SOUND>(c, g, lf, lane, cw, &sc);
        lq_head += n;
    }
    cand_flush<G>(c, cw, lane);
    square_ok_flush(c.fin.msd_counters, &sq_sum, cw.q_tail, lane);
    flush_stats(p, n_st, c_st, s_st, stat);
    if constexpr (SOUND) {
        if (sc.pt) rejected_flush(sc.snd->rejected, sc.rej);
    }
    if (c.fin.done) nice_launch_finish<SOUND>(c.fin, c.out.count);
}

}  // namespace nice
