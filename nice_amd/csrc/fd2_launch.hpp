// fd2_launch.hpp -- the FD detailed kernel's per-instantiation launchers: the
// occupancy query, the probe build's knobs and the forced stride, the table
// image, the dispatch between the persistent-grid, rounds and sibling-lane
// kernels, and a loop that asks fd2_plan.hpp for the next launch's shape,
// fills the kernel arguments from it and launches.  Included by fd2_part.hip
// (one object per part) and fd2_detailed.hip.
#pragma once
#include <stdlib.h>

#include <atomic>
#include <map>
#include <mutex>

#include "fd2_kernel.hpp"
#include "fd2_plan.hpp"
#include "host_math.hpp"

namespace nice {
namespace fd2 {

NICE_PROBE_ONLY(extern u64 *g_stamps; extern u64 g_last_launch[6];)  // last launch: grid, WG, chunk, nunits, tail, per_cu
// Forced sibling lane stride (nice_debug_force_sib_stride; 0: the model's pick).
extern std::atomic<uint32_t> g_force_sib_stride;
// Forced persistent sibling grid (nice_debug_force_sib_persistent): [0] the
// mode (0: production, 1: on, 2: never), [1] mode 1's workgroup cap (0: none).
extern std::atomic<uint32_t> g_force_sib_pers[2];

// The table image for this device and base, built on first use (the layout
// depends on the base only) and kept for the process.
template <class P>
static hipError_t fd2_tables(hipStream_t s, const uint4 **out) {
    if constexpr (P::TAB_BYTES == 0) {  // table-free kernel (Cfg::NOTAB)
        (void)s;
        *out = nullptr;
        return hipSuccess;
    }
    static std::mutex mu;
    static std::map<int, unsigned char *> have;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> g(mu);
    auto it = have.find(dev);
    if (it == have.end()) {
        unsigned char *t = nullptr;
        if ((e = hipMalloc(&t, P::TAB_BYTES)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(t, 0, P::TAB_BYTES, s)) != hipSuccess) return e;  // padding
        hipLaunchKernelGGL(fd2_tables_kernel<P>, dim3((P::B + 255) / 256), dim3(256), 0, s, t);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        // other streams (contexts) of this device may read it next
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
        it = have.emplace(dev, t).first;
    }
    *out = (const uint4 *)it->second;
    return hipSuccess;
}

// Workgroups of fd2_kernel<P> a CU holds, or -1.  Occupancy is a property of
// the code object: queried once per instantiation (a runtime call per launch
// is host latency on small fields).
template <class P>
static int fd2_occupancy() {
    static const int per_cu_q = [] {
        int v = 0;
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, (const void *)fd2_kernel<P>, P::WG, 0) == hipSuccess
                   ? v : -1;
    }();
    return per_cu_q;
}

// The plans' knobs: the environment's in the probe build, the defaults in
// the product (probe_knob is then a constant).
template <class P>
static PlanKnobs<P> fd2_knobs() {
    PlanKnobs<P> k;
    k.tchunk = probe_knob("NICE_FD2_TCHUNK", k.tchunk);
    k.min_chunk = probe_knob("NICE_FD2_MINCHUNK", k.min_chunk);
    k.sib_chunk = probe_knob("NICE_FD2_SIBCHUNK", k.sib_chunk);
    k.sib_rounds = probe_knob("NICE_FD2_SIBROUNDS", k.sib_rounds);
    k.sib_pers_min = probe_knob("NICE_FD2_SIBPERS_MIN", k.sib_pers_min);
    k.sib_pers_k = probe_knob("NICE_FD2_SIBPERS_K", k.sib_pers_k);
    return k;
}

// The regular parts of a launch: nunits chunks from (lo, hi), then the tail.
static inline void fd2_regular_parts(Fd2Args &a, u64 lo, u64 hi, u64 nunits, u64 chunk, u64 tail, u64 main_blocks) {
    a.start_lo = a.tail_lo = lo;
    a.start_hi = a.tail_hi = hi;
    add_u128(a.tail_lo, a.tail_hi, nunits * chunk);
    a.nunits = (u32)nunits;
    a.chunk = (u32)chunk;
    a.tail_count = (u32)tail;
    a.main_blocks = (u32)main_blocks;
}

// What every launch of a field shares, then the launch.  last: the field's
// finish rides on its last launch.
template <class P>
static hipError_t fd2_enqueue(Fd2Args &a, const DetailedLaunch &q, const uint4 *tabs, bool last, u64 grid,
                              hipStream_t s) {
    NICE_PROBE_ONLY(a.stamps = g_stamps;)
    a.cutoff = q.cutoff;
    a.ncopies = q.hist_copies;
    a.hist = q.hist;
    a.out = q.out;
    a.tabs = tabs;
    a.fin = last ? q.fin : FieldFinish{nullptr, nullptr, 0, 0};
    hipLaunchKernelGGL(fd2_kernel<P>, dim3((u32)grid), dim3(P::WG), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess && q.launches) ++*q.launches;
    return e;
}

template <class P>
static hipError_t launch_sib(const DetailedLaunch &p, int num_cus, hipStream_t s);
template <class K, class P>
static hipError_t launch_sib_shape(const DetailedLaunch &p, const SibShape &sh, const uint4 *tabs,
                                   const PlanKnobs<P> &knobs, int num_cus, int per_cu, hipStream_t s);

template <class P>
static hipError_t launch_cfg(const DetailedLaunch &p, int num_cus, hipStream_t s) {
    if constexpr (P::SIB > 1) return launch_sib<P>(p, num_cus, s);
    const int per_cu_q = fd2_occupancy<P>();
    if (per_cu_q < 0) return hipErrorInvalidDeviceFunction;
    const int per_cu = per_cu_q < 1 ? 1 : per_cu_q;
    // Every near-miss count must lie above the window (it is recorded on the
    // out-of-window branch).
    if (p.cutoff + 1 < (u32)(P::W0 + P::W)) return hipErrorInvalidValue;
    const PlanKnobs<P> knobs = fd2_knobs<P>();
    if constexpr (P::PERS) {
        if (!pers_suits<P>(p.count, num_cus, per_cu_q, knobs)) return launch_cfg<typename P::NoPers>(p, num_cus, s);
    }
    const uint4 *tabs = nullptr;
    hipError_t e = fd2_tables<P>(s, &tabs);
    if (e != hipSuccess) return e;
    DetailedLaunch q = p;
    u64 left = p.count;
    while (left) {
        const RegularPlan pl = plan_regular<P>(left, num_cus, per_cu, knobs);
        if (!pl.ok) return hipErrorInvalidValue;
        Fd2Args a{};
        fd2_regular_parts(a, q.start_lo, q.start_hi, pl.nunits, pl.chunk, pl.tail, pl.main_blocks);
        if constexpr (!P::N64 && !P::C64) {
            host_digits(((u128)a.start_hi << 64) | a.start_lo, P::B, a.xs, P::NX);
            host_digits(((u128)a.tail_hi << 64) | a.tail_lo, P::B, a.xt, P::NX);
        }
        a.wave_cap = pl.wave_cap;
        NICE_PROBE_ONLY({
            const u64 v[6] = {pl.grid, (u64)P::WG, pl.chunk, pl.nunits, pl.tail, (u64)per_cu};
            for (int k = 0; k < 6; k++) g_last_launch[k] = v[k];
        })
        if ((e = fd2_enqueue<P>(a, q, tabs, left == pl.cnt, pl.grid, s)) != hipSuccess) return e;
        add_u128(q.start_lo, q.start_hi, pl.cnt);
        left -= pl.cnt;
    }
    return hipSuccess;
}

// One batch launch: `n` descriptors (all of this P's combo) from `units`.
template <class P>
static hipError_t launch_batch_cfg(const BatchLaunch &p, const Fd2Unit *units, u32 n, hipStream_t s) {
    if (p.cutoff + 1 < (u32)(P::W0 + P::W)) return hipErrorInvalidValue;
    const uint4 *tabs = nullptr;
    hipError_t e = fd2_tables<P>(s, &tabs);
    if (e != hipSuccess) return e;
    Fd2BatchArgs a{};
    a.units = units;
    a.hist = p.hist;
    a.ncopies = p.ncopies;
    a.cutoff = p.cutoff;
    a.out = p.out;
    a.tabs = tabs;
    hipLaunchKernelGGL(fd2_batch_kernel<P>, dim3(n), dim3(P::WG), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (p.launches) ++*p.launches;
    return hipSuccess;
}

// Sibling-lane launches (Cfg::SIB = M > 1; the layout of a launch is
// described at fd2_plan.hpp plan_sib).
template <class P>
static hipError_t launch_sib(const DetailedLaunch &p, int num_cus, hipStream_t s) {
    const int per_cu_q = fd2_occupancy<P>();
    if (per_cu_q < 0) return hipErrorInvalidDeviceFunction;
    const int per_cu = per_cu_q < 1 ? 1 : per_cu_q;
    if (sib_too_short<P>(p.count)) return launch_cfg<typename P::NoSib>(p, num_cus, s);
    if (p.cutoff + 1 < (u32)(P::W0 + P::W)) return hipErrorInvalidValue;
    const uint4 *tabs = nullptr;
    hipError_t e = fd2_tables<P>(s, &tabs);
    if (e != hipSuccess) return e;
    PlanKnobs<P> knobs = fd2_knobs<P>();
    if constexpr (P::HAS_SIBPERS) {
        knobs.sib_pers_mode = g_force_sib_pers[0].load(std::memory_order_relaxed);
        knobs.sib_pers_max_wg = g_force_sib_pers[1].load(std::memory_order_relaxed);
    }
    const u128 seg_start = ((u128)p.start_hi << 64) | p.start_lo;
    SibShape sh = plan_sib<P>(seg_start, p.count, num_cus, per_cu, p.overlapped != 0,
                              g_force_sib_stride.load(std::memory_order_relaxed), knobs);
    if (sh.kind == SibShape::kNoSib) return launch_cfg<typename P::NoSib>(p, num_cus, s);
    if (sh.kind == SibShape::kError) return hipErrorInvalidValue;
    if (p.sib) {
        p.sib[0] = (uint32_t)P::SIB;
        p.sib[1] = (uint32_t)sh.L;
        p.sib[2] = 0;
    }
    // the persistent twin (same tables, same plan arithmetic) where the
    // segment is long enough for it
    if constexpr (P::HAS_SIBPERS) {
        const int pq = fd2_occupancy<typename P::SibPers>();
        if (pq >= 1) {
            plan_sib_pers<P>(sh, p.count, num_cus, pq, p.overlapped != 0, knobs);
            if (sh.pers) return launch_sib_shape<typename P::SibPers, P>(p, sh, tabs, knobs, num_cus, pq, s);
        }
    }
    return launch_sib_shape<P, P>(p, sh, tabs, knobs, num_cus, per_cu, s);
}

// The launches of a sibling segment of shape sh with kernel K (P, or its
// persistent twin P::SibPers when sh.pers).
template <class K, class P>
static hipError_t launch_sib_shape(const DetailedLaunch &p, const SibShape &sh, const uint4 *tabs,
                                   const PlanKnobs<P> &knobs, int num_cus, int per_cu, hipStream_t s) {
    static_assert(K::SIBPERS || std::is_same<K, P>::value, "the rounds kernel or its persistent twin");
    constexpr u64 SB = (u64)P::SIB * P::B * P::B;
    hipError_t e;
    DetailedLaunch q = p;
    u64 left = p.count;
    while (left) {
        const SibLaunchPlan pl = plan_sib_launch<P>(left, sh, num_cus, per_cu, knobs);
        if (K::SIBPERS && p.sib && pl.sib_blocks) p.sib[2] = (uint32_t)pl.sib_blocks;
        Fd2Args a{};
        a.sib_lo = a.edge_lo = q.start_lo;
        a.sib_hi = a.edge_hi = q.start_hi;
        add_u128(a.edge_lo, a.edge_hi, sh.upb * sh.L);
        a.sib_chunk = (u32)sh.L;
        a.sib_upb = (u32)sh.upb;
        a.sib_units = (u32)pl.sib_units;
        a.sib_blocks = (u32)pl.sib_blocks;
        a.edge_chunk = (u32)sh.r;
        a.edge_units = (u32)pl.edge_units;
        a.edge_blocks = (u32)pl.edge_blocks;
        u64 lo = q.start_lo, hi = q.start_hi;  // the remainder follows the super-blocks
        add_u128(lo, hi, pl.Q * SB);
        fd2_regular_parts(a, lo, hi, pl.nunits, pl.chunk, pl.tail, pl.main_blocks);
        a.wave_cap = pl.wave_cap;
        NICE_PROBE_ONLY({
            const u64 v[6] = {pl.grid, (u64)P::WG, sh.L, pl.sib_units, pl.R, (u64)per_cu};
            for (int k = 0; k < 6; k++) g_last_launch[k] = v[k];
        })
        if ((e = fd2_enqueue<K>(a, q, tabs, left == pl.cnt, pl.grid, s)) != hipSuccess) return e;
        add_u128(q.start_lo, q.start_hi, pl.cnt);
        left -= pl.cnt;
    }
    return hipSuccess;
}

}  // namespace fd2
}  // namespace nice
