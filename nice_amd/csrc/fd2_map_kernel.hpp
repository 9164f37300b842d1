// fd2_map_kernel.hpp -- the per-number unique-count map on the FD kernel's
// arithmetic (gfx950).  fd2_map_kernel<P> has fd2_batch_kernel's shape (fd2_kernel.hpp):
// rounds of workgroups, regular lanes, one descriptor per workgroup -- first
// n, lanes, chunk, the digits for init_at and a 64-bit output offset -- and
// runs the same table load, init / init_at, step and mask building as
// walk_chunk.  Where walk_chunk counts u = popcount(mask) into the windowed
// LDS histogram and lists the near-misses, the map kernel writes u as one
// byte to out[n - start]: no histogram, no OUTL bins, no NumOut.  Callers
// derive those from the map (nice_unique_map, include/nice_hip.h).
//
// The stores.  A lane walks `chunk` consecutive numbers, so at one step the
// 64 lanes of a wave stand `chunk` bytes apart: a byte store per step would be
// 64 partial-line writes per wave-step.  Instead each lane stages its counts
// in a 16-byte LDS ring and the wave flushes every 16 steps, each lane
// storing one whole, 16-byte-aligned piece of its own run:
//
//  * The ring is indexed by the byte's GLOBAL address mod 16, so the ring
//    image is the aligned piece's image whatever the residue r of the lane's
//    first address (out has any byte alignment, a lane's run starts at
//    tid * chunk: any residue mod 16).
//  * After 16 steps the ring holds the upper 16 - r bytes of piece k and the
//    lower r bytes of piece k + 1.  The lower r bytes of piece k were read at
//    the previous flush and wait in four registers: piece k = (prev & low
//    mask) | (cur & ~low mask), one v_bfi_b32 per dword.
//  * A piece that lies wholly inside the lane's run is one 16-byte store.
//    The first piece (its bytes below the run belong to the lane before, or
//    lie before `out`) and the last one or two are clipped byte-exactly to
//    [run start, run end): naturally aligned 1-, 2-, 4- and 8-byte stores, at
//    most seven, never a byte outside the run.
//  * The ring is word-interleaved -- dword d of thread t at (d WG + t) * 4 --
//    so a wave's byte writes and the flush's four dword reads each touch 64
//    distinct banks.
//
// The ring takes the place of the window rows (16 bytes per thread of the
// W * WG * 2 >= 30 bytes the batch kernel keeps there), so the LDS layout,
// LDS_BYTES and with them the occupancy are the batch kernel's, on the
// three-mask-word bases too, whose tables leave room for nothing larger.
#pragma once
#include "fd2_kernel.hpp"

namespace nice {
namespace fd2 {

// The map kernel's configuration: the batch kernel's, as a type of its own, so
// that every device function instantiated for it is the map kernel's own (see
// BatchCfg on what sharing instantiations does to a kernel's registers).
template <int B_, int ND_, int NE_, int NE2_>
struct MapCfg : BatchCfg<B_, ND_, NE_, NE2_> {};

struct Fd2MapUnit {
    u64 lo, hi;   // first n
    u64 off;      // out offset of the first n (bytes = numbers)
    u32 lanes;    // active lanes (<= WG)
    u32 chunk;    // numbers per lane (<= B); 1 for a tail workgroup
    u32 xs[kXDigits];  // radix-B digits of the first n (init_at; bases whose n passes 64 bits)
};
static_assert(sizeof(Fd2MapUnit) == 80, "descriptor layout");

struct Fd2MapArgs {
    const Fd2MapUnit *units;  // one per workgroup
    unsigned char *out;       // any byte alignment
    const uint4 *tabs;
};

constexpr int kMapTile = 16;  // steps between flushes = bytes of a piece

// The piece's bytes from position a (< 16) on, as the low bytes of a u64: the
// piece travels as its two 8-byte halves, so picking one is a select between
// two values (a four-way pick by position turns into an indexed private array,
// i.e. scratch).  A store of s bytes at an s-aligned a never crosses a half.
__device__ __forceinline__ u64 map_bytes_at(u64 h0, u64 h1, u32 a) { return ((a & 8) ? h1 : h0) >> (8 * (a & 7)); }

// Bytes [a, b) (0 <= a < b <= 16, b - a < 16) of the 16-byte-aligned piece at
// p: naturally aligned stores, ascending sizes up to the first 8-byte
// boundary, then descending.
__device__ __forceinline__ void map_store_partial(unsigned char *p, u64 h0, u64 h1, u32 a, u32 b) {
    if ((a & 1) && a + 1 <= b) {
        p[a] = (unsigned char)map_bytes_at(h0, h1, a);
        a += 1;
    }
    if ((a & 2) && a + 2 <= b) {
        *(unsigned short *)(p + a) = (unsigned short)map_bytes_at(h0, h1, a);
        a += 2;
    }
    if ((a & 4) && a + 4 <= b) {
        *(u32 *)(p + a) = (u32)map_bytes_at(h0, h1, a);
        a += 4;
    }
    // a is now a multiple of 8, or fewer bytes are left than its alignment
    if (a + 8 <= b) {
        *(u64 *)(p + a) = map_bytes_at(h0, h1, a);
        a += 8;
    }
    if (a + 4 <= b) {
        *(u32 *)(p + a) = (u32)map_bytes_at(h0, h1, a);
        a += 4;
    }
    if (a + 2 <= b) {
        *(unsigned short *)(p + a) = (unsigned short)map_bytes_at(h0, h1, a);
        a += 2;
    }
    if (a + 1 <= b) p[a] = (unsigned char)map_bytes_at(h0, h1, a);
}

// A lane's output state: its run is bytes [lo, hi) from the workgroup's
// first byte `wout`; q is the next piece's offset from wout (16-byte aligned
// as an address; below lo, even below 0, for the first piece).
struct MapSink {
    unsigned char *wout;  // wave-uniform
    int lo, hi, q;
    u32 ring;             // LDS byte address of this thread's ring dword 0
    u32 pos;              // ring position of the next byte: its global address mod 16
    u32 r;                // the run's first address mod 16
    u32 prev[4];          // the ring as the previous flush read it
};

template <class P>
__device__ __forceinline__ void map_put(MapSink &k, unsigned char *smem, u32 u) {
    // dword pos / 4 of the interleaved ring, byte pos % 4
    smem[k.ring + (k.pos & 12u) * (u32)P::WG + (k.pos & 3u)] = (unsigned char)u;
    k.pos = (k.pos + 1) & 15u;
}

// Piece `w`, clipped to the lane's run.
__device__ __forceinline__ void map_store_piece(const MapSink &k, const u32 (&w)[4]) {
    const int a = k.lo > k.q ? k.lo - k.q : 0;
    const int b = k.hi - k.q < kMapTile ? k.hi - k.q : kMapTile;
    if (b <= a) return;
    // (a == 0 means q >= lo >= 0; a partial piece is addressed from q + a >= lo)
    unsigned char *p = k.wout + (long long)k.q;
    if (a == 0 && b == kMapTile) *(uint4 *)p = make_uint4(w[0], w[1], w[2], w[3]);
    else map_store_partial(p, w[0] | (u64)w[1] << 32, w[2] | (u64)w[3] << 32, (u32)a, (u32)b);
}

// Flush: the piece that the last 16 steps completed.
template <class P>
__device__ __forceinline__ void map_flush(MapSink &k, const unsigned char *smem) {
    u32 cur[4], w[4];
#pragma unroll
    for (int d = 0; d < 4; d++) cur[d] = *(const u32 *)(smem + k.ring + d * 4 * P::WG);
#pragma unroll
    for (int d = 0; d < 4; d++) {
        // bytes below r of this dword come from the previous read
        const int nb = (int)k.r - 4 * d;
        const u32 low = nb >= 4 ? ~0u : nb <= 0 ? 0u : (1u << (8 * nb)) - 1;
        w[d] = (k.prev[d] & low) | (cur[d] & ~low);
        k.prev[d] = cur[d];
    }
    map_store_piece(k, w);
    k.q += kMapTile;
}

// One lane's chunk: walk_chunk's loop with the map's sink.  (walk_chunk keeps
// its own text: its instantiations are not to move for a kernel they do not
// serve.  Keep the mask building in step with it.)
template <class P>
__device__ __forceinline__ void walk_map(State<P> &st, unsigned char *smem, u32 chunk, MapSink &k) {
    recompute_hi<P>(st, smem);
    for (u32 i = 0; i < chunk; i++) {
        u32 m[P::MW], w1 = 0;
#pragma unroll
        for (int w = 0; w < P::MW; w++) m[w] = st.hi[w];
        if constexpr (P::LSD) {
            const uint2 v = *(const uint2 *)(smem + (P::LSDX ? 0 : P::TL) + st.r8);
            m[0] |= v.x;
            if constexpr (P::LSDX) {
                m[1] |= v.y;
                w1 = smem[st.rc];
            } else {
                m[1] |= v.y & P::DMASK;
                w1 = v.y;
            }
        }
#pragma unroll
        for (int q = P::LO; q < P::SL; q++) {
            if (P::vd_s(q) || (P::VDL && q == 0)) or_valu<P>(st.S[q] - P::EBT, m);
            else or_lookup<P, P::TB - (int)P::EBT, P::T2 - (int)P::EBT / 2>(smem, st.S[q], m);
        }
#pragma unroll
        for (int q = P::LO; q < P::CL; q++) {
            if (P::vd_c(q) || (P::VDL && q == 0)) or_valu<P>(st.C[q], m);
            else or_lookup<P, P::TB, P::T2>(smem, st.C[q], m);
        }
        u32 u = __popc(m[0]);
#pragma unroll
        for (int w = 1; w < P::MW; w++) u += __popc(m[w]);
        map_put<P>(k, smem, u);
        if ((i & (kMapTile - 1)) == kMapTile - 1) map_flush<P>(k, smem);  // wave-uniform
        step<P>(st, smem, w1);
    }
    // the steps since the last flush, then the bytes above the last aligned
    // boundary (both clipped to the run's end; stale ring bytes lie beyond it)
    if (chunk & (kMapTile - 1)) map_flush<P>(k, smem);
    map_store_piece(k, k.prev);
}

template <class P>
__global__ void __launch_bounds__(P::WG) __attribute__((amdgpu_waves_per_eu(P::WPE, P::WPE)))
fd2_map_kernel(Fd2MapArgs a) {
    static_assert(!P::PERS && P::SIB == 1 && P::PROBE == 0, "map kernel: rounds, regular lanes");
    static_assert(!(P::MW == 3 && P::WG >= 1024) && P::LGW == 0, "MapCfg: BatchCfg's lookup groups (none)");
    static_assert(!P::SPLIT && P::HB == 0 && P::HIST_BYTES >= kMapTile * P::WG,
                  "the rings take the window rows' place");
    __shared__ __attribute__((aligned(16))) unsigned char smem[P::LDS_BYTES];
    const u32 tid = threadIdx.x;
    // The descriptor, indexed by blockIdx.x only: read before anything is
    // written, so the loads are scalar.
    const Fd2MapUnit *__restrict__ d = a.units + blockIdx.x;
    const u64 start_lo = d->lo, start_hi = d->hi;
    const u32 lanes = d->lanes, chunk = d->chunk;
    unsigned char *wout = a.out + d->off;
    u32 xs[P::NX];
    if constexpr (!P::N64 && !P::C64) {
#pragma unroll
        for (int i = 0; i < P::NX; i++) xs[i] = d->xs[i];
    }
    fd2_load_tables<P>(smem, a.tabs, tid);
    const bool active = tid < lanes;
    const u64 n0_off = (u64)tid * chunk;  // < WG * B < 2^31
    u64 n0_lo = start_lo, n0_hi = start_hi;
    add_u128(n0_lo, n0_hi, n0_off);
    State<P> st;
    if constexpr (P::N64 || P::C64) {
        if (active) init<P>(st, n0_lo, n0_hi);
    } else {
        if (active) init_at<P>(st, xs, n0_off, n0_lo, n0_hi);
    }
    MapSink k;
    k.wout = wout;
    k.lo = (int)n0_off;
    k.hi = k.lo + (int)chunk;
    k.r = ((u32)(unsigned long long)wout + (u32)n0_off) & 15u;
    k.pos = k.r;
    k.q = k.lo - (int)k.r;
    k.ring = tid * 4;
#pragma unroll
    for (int i = 0; i < 4; i++) k.prev[i] = 0;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (active) walk_map<P>(st, smem, chunk, k);
}

}  // namespace fd2
}  // namespace nice
