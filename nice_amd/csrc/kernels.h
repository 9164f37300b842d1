// kernels.h -- host-side launch entry points for the gfx950 kernels
// (implemented in detailed.hip / niceonly.hip / niceonly_part.hip -- the
// niceonly kernel templates: niceonly_cand.hpp and the headers it lists --,
// niceonly_ranges.hip / niceonly_ranges_part.hip; used by the C ABI files,
// abi_*.cpp).  The word layouts host and device share are in
// layout.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "layout.h"

namespace nice {

// Near-miss / nice-number output buffer on the device.
struct NumOut {
    uint64_t *n;     // (lo, hi) pairs
    uint32_t *u;     // num_uniques per entry (may be null for niceonly)
    uint32_t *count; // atomically incremented; may exceed cap (overflow detection)
    uint32_t cap;
};

// In-kernel end of a field (fd2 kernels): the launch's last workgroup sums
// the histogram copies into out_mapped[0..128] (mapped host memory), writes
// the near-miss count to out_mapped[kFinCount] and re-zeroes copies, count and
// *done; then, after a system-scope release, seq to out_mapped[kFinSeq], which the
// host polls instead of waiting for the kernel's completion signal.
// out_mapped == nullptr: the caller runs launch_detailed_finish.
struct FieldFinish {
    uint64_t *out_mapped;
    uint32_t *done;  // kDoneWords arrival counters (layout.h), re-zeroed by the finish
    uint64_t seq;    // the field's sequence number (nonzero)
    // Nonzero (fields of < 2^31 numbers): every result word is published as
    // tag << 32 | value -- bins 0..base and the near-miss count [kFinCount] -- with
    // no ordering among them and no sequence word; the host takes the field
    // as finished once every word carries the tag (one fewer round trip to
    // host memory than stores, wait, release store of the sequence word).
    uint32_t tag;
};

struct DetailedLaunch {
    uint64_t start_lo, start_hi; // first n of the segment
    uint64_t count;              // numbers in the segment
    uint32_t base;
    uint32_t cutoff;             // near-miss cutoff (number_stats.rs:15-17)
    uint64_t *hist;              // kHistCopies x kHistBins u64 bins, accumulated
    uint32_t hist_copies;        // fd2: copies the field's launches use (set by launch_detailed_fd2)
    NumOut out;
    FieldFinish fin;             // fd2 only; see FieldFinish
    uint32_t *launches;          // if set, incremented per kernel launch enqueued
    uint32_t *sib;               // fd2, if set: [0] sibling lanes M of the field's last sibling-lane
                                 // launch (0: none ran), [1] its lane stride L, [2] the workgroups of
                                 // its persistent sibling grid (0: rounds)
    uint32_t overlapped;         // fd2: another field of the device was still running when this one
                                 // was enqueued (the pipelined case), so launches are shaped for
                                 // throughput, not for the latency of a lone field
};

// Production FD kernel (fd2_detailed.hip): bases 40, 50, 80, in-range segments.
bool fd2_supported(uint32_t base);
hipError_t launch_detailed_fd2(const DetailedLaunch &p, int num_cus, hipStream_t s);
// The n where fd2's per-segment limb layout changes (ascending).
size_t fd2_cuts(uint32_t base, unsigned __int128 *out, size_t cap);
// Batched ranges (fd2_batch_kernel, fd2_kernel.hpp): many small in-range
// ranges in one launch per limb layout.  A unit is one workgroup: `lanes`
// lanes walk `chunk` numbers each from n = (lo, hi), and flush into histogram
// row `row`; `combo` indexes the base's cut intervals (fd2_cuts).
struct BatchUnit {
    uint64_t lo, hi;
    uint32_t lanes, chunk;
    uint32_t row, combo;
};
constexpr size_t kBatchDescBytes = 80;  // device descriptor per unit (Fd2Unit)
// Workgroup size and target chunk of a base's batch kernel.
uint32_t fd2_batch_wg(uint32_t base);
uint32_t fd2_batch_chunk(uint32_t base);
// The units of [start, end) (inside the base's valid range): cut at the limb
// layout changes, each piece tiled into main workgroups (one chunk per lane)
// plus at most one tail workgroup (the < chunk numbers left over, one per
// lane).  Appended to `out` in ascending n.  Pure host code (the tiling of a piece: fd2_plan.hpp batch_tile).
void fd2_batch_plan(uint32_t base, unsigned __int128 start, unsigned __int128 end, uint32_t row,
                    std::vector<BatchUnit> &out);
struct BatchLaunch {
    uint32_t base;
    uint32_t cutoff;
    const BatchUnit *units;  // host
    size_t n_units;
    void *h_desc, *d_desc;   // pinned staging / device array, n_units x kBatchDescBytes
    uint64_t *hist;          // rows of kHistBins u64 bins (zeroed by the caller)
    uint32_t ncopies;        // 0: unit.row selects the row; else workgroup b flushes into row b % ncopies
    NumOut out;
    uint32_t *launches;      // if set, incremented per kernel launch enqueued
};
// Groups the units by combo, copies their descriptors (async, on s) and
// enqueues one launch per combo present.
hipError_t launch_detailed_fd2_batch(const BatchLaunch &p, hipStream_t s);
// Test hook: every later sibling-lane launch of the process uses lane stride
// L (odd; 0 restores the production pick, fd2_plan.hpp plan_sib).
void fd2_force_sib_stride(uint32_t L);
// Test hook: the persistent sibling grid (fd2_plan.hpp plan_sib_pers) of every
// later sibling-lane launch: mode 0 production, 1 on for every sibling
// segment (at most max_workgroups workgroups when nonzero), 2 never.
void fd2_force_sib_persistent(uint32_t mode, uint32_t max_workgroups);
// The base's compile-time histogram window [w0, w0 + w) (fd2_cfg.hpp
// window_w0 / window_w); false for a base without an FD kernel.  The FD
// launchers accept a cutoff with cutoff + 1 >= w0 + w.
bool fd2_window(uint32_t base, uint32_t *w0, uint32_t *w);
// Field epilogue on the launch stream: out_mapped[0..128] = the summed
// histogram copies, out_mapped[kFinCount] = *count; copies and counter are zeroed.
hipError_t launch_detailed_finish(uint64_t *hist, uint32_t *count, uint64_t *out_mapped, hipStream_t s);
// Generic per-n kernel: any base 2..128, any n < 2^128.
hipError_t launch_detailed_generic(const DetailedLaunch &p, int num_cus, hipStream_t s);

// Niceonly.  A "leaf" is one MSD-surviving sub-range in stride-index form:
// its candidates are n = b0 + ((g0 + j) / R) * M + residues[(g0 + j) % R],
// j < count (stride_filter.rs:99-155).  Leaves come from the host MSD producer
// or from the device MSD filter below.
struct Leaf {
    uint64_t b0_lo, b0_hi;  // cycle base: range_start - range_start mod M
    uint32_t g0;            // lower_bound(residues, range_start mod M), in [0, R]
    uint32_t count;         // candidates in the range
};

// In-kernel end of a niceonly field (its last candidate launch): the last
// workgroup copies the MSD counters (device MSD) and the nice count into
// mapped host memory, so a field needs no copy launches.
// Every candidate launch ends with its last workgroup re-zeroing the device
// MSD's per-batch leaf-record count (kMsdLeafCount) for the next batch; the
// field's last launch instead copies the counters and the nice count out and
// re-zeroes them for the slot's next field (no memset or copy launches).
struct NiceFinish {
    uint32_t *msd_mapped;          // kMsdMappedWords words (device MSD field end) or null
    uint32_t *count_mapped;        // nice count (field end) or null
    uint32_t *msd_counters;        // device MSD counters, or null (host MSD)
    uint32_t *done;                // kDoneWords arrival counters (layout.h), re-zeroed;
                                   // null: no epilogue
};

struct NiceonlyLaunch {
    const Leaf *leaves;
    const uint32_t *n_leaves_dev;  // leaf count on the device (or null: use n_leaves)
    uint32_t n_leaves;
    const uint32_t *residues;      // R valid residues mod M, ascending
    uint32_t R, M;
    uint32_t base;
    uint32_t in_range;             // every candidate inside the base's valid range
    uint32_t nice_min;             // in-range fields of the compile-time kernels: a square survivor is
                                   // listed when its digit union has >= nice_min members (production:
                                   // base, i.e. nice; nice_debug_set_nice_min lowers it)
    NumOut out;
    NiceFinish fin;
};
// Sound filter (NICE_FILTER_SOUND, radix_fast.hpp): what its kernel variants
// take beside the launch structs.  A leaf carries the digit mask of its
// common leading digits of n^2 and n^3 (all ones: they repeat, every candidate
// goes) and whether it holds >= 2 numbers; leaf_masks[] runs parallel to the
// leaf list, so the reference filter's 24-byte records stay as they are.
struct LeafMask {
    uint32_t w[3];
    uint32_t multi;
};
struct SoundLaunch {
    const uint32_t *residues;     // StrideTable::residues_flagged (bit 31: the low digits repeat)
    const uint32_t *lowmask;      // StrideTable::lowmask, (base + 31) / 32 words per residue
    LeafMask *leaf_masks;         // device MSD: parallel to MsdLaunch::leaves
    unsigned long long *rejected; // candidates the prefix test rejected (counters + kMsdRejected, sticky)
    uint32_t fast;                // the field runs the base's compile-time sound variants
                                  // (sound_prefix_field), else the run-time-base ones
    uint32_t prefix_test;         // 0: the recursion without Filter C only (fields that are not
                                  // `fast`; the probe build's A/B)
};
// snd: the sound variants (null: the reference filter's kernels).  The prefix
// test runs on the compile-time kernels' in-range fields; elsewhere the
// variants only leave Filter C out.
hipError_t launch_niceonly(const NiceonlyLaunch &p, int num_cus, hipStream_t s, const SoundLaunch *snd = nullptr);

// Batched niceonly ranges (niceonly_ranges_kernel, niceonly_ranges.hpp; the
// run-time-base instance in niceonly_ranges.hip, the fast bases' in the
// objects of niceonly_ranges_part.hip): niceonly_kernel's walk over leaves
// that carry the index of the caller's range they belong to.  No MSD filter
// runs: every stride candidate of every leaf gets the full test.
struct RangeLeaf {
    uint64_t b0_lo, b0_hi;  // as Leaf
    uint32_t g0, count;
    uint32_t range;         // range index of the call
    uint32_t mask;          // prefix test: the range's index among the launch's RangeSpan / LeafMask
                            // records (every piece of a range carries the same one); else 0
};
struct NiceRangesLaunch {
    NiceonlyLaunch c;          // residues, R, M, base, in_range, nice_min and out, where out.u receives
                               // each entry's range index; its leaf fields and fin are unused
    const RangeLeaf *leaves;
    uint32_t n_leaves;
    uint32_t *square_ok;       // one counter per range of the call (compile-time kernels only)
    uint32_t *done;            // kDoneWords arrival counters, re-zeroed by the last workgroup
    uint32_t *count_mapped;    // ... which copies *c.out.count here (mapped host memory)
};
// The sound filter's per-candidate prefix test on caller-given ranges
// (nice_process_ranges_niceonly_ex, NICE_RANGES_PREFIX_ON): a range [first,
// last] of a fast base, inside its valid range, has a LeafMask of its own --
// every n of it carries the common leading digits of first^2, last^2 and of
// the two cubes -- made by range_mask_kernel from a RangeSpan before the
// candidate launch, whose prefix variant tests each candidate's residue
// against it ahead of the square test.
struct RangeSpan {
    uint64_t first_lo, first_hi;  // the range's first number
    uint64_t last_lo, last_hi;    // ... and its last (end - 1)
};
struct RangesPrefixLaunch {
    SoundLaunch snd;               // residues (flagged) and lowmask; the other fields unused
    const LeafMask *masks;         // indexed by RangeLeaf::mask
    unsigned long long *rejected;  // one counter per range of the call
};
// c.in_range set: the compile-time kernel of c.base (a niceonly fast base, every
// leaf inside its valid range); else the run-time-base kernel.  pre (in_range
// launches only): the kernel's prefix-testing variant.
hipError_t launch_niceonly_ranges(const NiceRangesLaunch &p, int num_cus, hipStream_t s,
                                  const RangesPrefixLaunch *pre = nullptr);
// masks[i] = the LeafMask of spans[i], i < n, one lane per span (base: a
// niceonly fast base, every span inside its valid range).
hipError_t launch_range_masks(uint32_t base, const RangeSpan *spans, uint32_t n, LeafMask *masks, hipStream_t s);

struct MsdLaunch;
// Whether a device-MSD field (bounds, base, table and in_range set) can run the
// prefix test: a niceonly fast base, in range, on the k = 2 table.
bool sound_prefix_field(const MsdLaunch &p);

// Device MSD filter (msd_prefix_filter.rs:583-658 as a level-synchronous BFS):
// one lane per node; leaves (already in stride-index form) are appended to
// `leaves`.  Nodes: {start lo, hi, size, depth}.
// A level-queue node: numbers [start + off, start + off + size) of the field
// (off < field size < 2^63; the level is the queue's).
struct MsdNode {
    uint64_t off, size;
};
struct MsdLaunch {
    // The batch's level-0 nodes are the field's chunks c_j = deal_offset +
    // (first + j) * deal_stride, j < nchunks: [start + c_j chunk, min(end,
    // start + (c_j + 1) chunk)).  deal_stride 1 / offset 0 is a contiguous run
    // of chunks; a rank of an N-way niceonly job is dealt every N-th chunk.
    uint64_t start_lo, start_hi;  // field start (chunk grid origin)
    uint64_t end_lo, end_hi;      // field end
    uint64_t first;               // first dealt chunk of this batch (index among this caller's chunks)
    uint64_t nchunks;             // chunks in this batch
    uint64_t deal_stride, deal_offset;
    uint64_t chunk;               // MSD chunk size (client rule)
    uint64_t floor_size;          // recursion floor (250)
    MsdNode *q[2];                // ping-pong level queues
    uint32_t *counters;           // kMsdCounterWords words, laid out as layout.h describes
    uint32_t q_cap;
    Leaf *leaves;
    uint32_t leaf_cap;
    const uint32_t *residues;
    const uint32_t *ranks;        // ranks[r] = lower_bound(residues, r), r in [0, M]
    uint32_t R, M;
    uint32_t base;
    uint32_t in_range;            // the batch lies inside the base's valid range
    uint32_t first_batch;         // init zeroes the field's sticky counters and *nice_count
    uint32_t *nice_count;
    uint32_t probe;               // probe build only (NICE_MSD_PROBE): 1 no skip test, 2 no leaf stride math,
                                  // 4 wave kernel: no candidate test
};
// Node of a chunk's fused recursion: offset from the chunk start, size.
struct ChunkNode {
    uint32_t off, size;
};
// Enqueue a batch's MSD recursion (no host sync): with `scratch` (grid x 2 x
// cap ChunkNodes; msd_plan.hpp msd_fused_cap, msd_fused_grid) ONE fused
// launch, one workgroup per chunk; otherwise the init + level kernels.
hipError_t launch_msd_device(const MsdLaunch &p, int num_cus, hipStream_t s, ChunkNode *scratch = nullptr,
                             uint32_t cap = 0, uint32_t grid = 0, const SoundLaunch *snd = nullptr);

// Large chunks: init + the level BFS down to `level0` (nodes <= 2^26 numbers,
// enough roots to fill the chip), then msd_wave_kernel: the recursion below
// level0 AND the candidate test of every leaf in one launch (`c` holds the
// residues, output and finish; its leaf fields are unused), `grid` workgroups
// of msd_wave_waves_per_group() waves, each wave with a kStackCap-node stack
// in `scratch` (msd_wave_scratch_bytes(grid); both msd_plan.hpp).  Leaves of
// the BFS levels go to p.leaves and are tested by the same launch.
hipError_t launch_msd_wave(const MsdLaunch &p, const NiceonlyLaunch &c, uint32_t level0, void *scratch,
                           uint32_t grid, int num_cus, hipStream_t s, const SoundLaunch *snd = nullptr);

// The recursion's range list (nice_msd_ranges; msd_ranges.hpp, the run-time-base
// instances and the sort in msd_ranges.hip, the fast bases' in the objects of
// msd_ranges_part.hip): the roots of a batch, and what one group of them --
// one kernel form, one base placement -- runs with.
struct MsdRangeRoot {
    uint64_t start_lo, start_hi, size;
    uint32_t in_range;  // the root lies inside the base's valid range (MsdLaunch::in_range of its nodes)
    uint32_t pad;
};
struct MsdRangesLaunch {
    const MsdRangeRoot *roots;  // the batch's roots
    const uint32_t *list;       // the group's roots, as indices into `roots`
    uint32_t n;                 // ... and how many
    uint64_t floor_size;
    MsdNode *q[2];              // form 0: ping-pong level queues; a node's off is root << 40 | offset
    uint32_t q_cap;
    uint32_t *ctl;              // kMsdLevels level sizes (per group), kMsdLeafCount and kMsdOverflow (per batch)
    uint64_t *keys, *sizes;     // the leaf records: root << 40 | offset, and the size
    uint32_t leaf_cap;
};
// Enqueue one group.  fast: the compile-time kernels of `base` (a niceonly fast
// base; a missing kernel is an error), else the run-time-base ones.  scratch:
// form 1, one launch of `grid` workgroups (grid x 2 x cap ChunkNodes); null:
// form 0, init + the levels that a root of max_size numbers can reach.
hipError_t launch_msd_ranges(const MsdRangesLaunch &p, uint32_t base, bool fast, bool sound, uint64_t max_size,
                             int num_cus, hipStream_t s, ChunkNode *scratch, uint32_t cap, uint32_t grid,
                             uint32_t *launches);
// The records ordered by key (60 bits) on the device: temporary bytes for n
// records, and the sort (async on s) into keys_out / sizes_out.
hipError_t msd_ranges_sort_bytes(size_t n, size_t *bytes);
hipError_t msd_ranges_sort(void *temp, size_t temp_bytes, uint64_t *keys, uint64_t *keys_out, uint64_t *sizes,
                           uint64_t *sizes_out, size_t n, hipStream_t s);

// Diagnostics used by the parity tests: per-n unique counts / nice flags
// computed by the same device functions the production kernels use.
hipError_t launch_unique_counts(const uint64_t *n_pairs, uint32_t count, uint32_t base,
                                uint32_t *out, hipStream_t s);
hipError_t launch_is_nice(const uint64_t *n_pairs, uint32_t count, uint32_t base,
                          uint32_t *out, hipStream_t s);
// In-range n of a niceonly fast base (niceonly_bases.h): the unique-digit
// count by niceonly_kernel's limb path (radix_fast.hpp unique_fast).
hipError_t launch_unique_fast(const uint64_t *n_pairs, uint32_t count, uint32_t base,
                              uint32_t *out, hipStream_t s);
// ... and the count the niceonly kernels' cube pass compares with
// NiceonlyLaunch::nice_min (niceonly_cand.hpp cube_count: the LDS pair table
// for the two-word bases, VALU for b65/68/80; 0 when n^2 repeats a digit).
hipError_t launch_cube_count(const uint64_t *n_pairs, uint32_t count, uint32_t base,
                             uint32_t *out, hipStream_t s);

}  // namespace nice
