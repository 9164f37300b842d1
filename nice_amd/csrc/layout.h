// layout.h -- the word layouts the host and the kernels share, in one place.
//
// Plain constants (no HIP header), included by the device headers, kernels.h
// and the host ABI files: a word that moves, or a new one, is one edit here.
#pragma once

#include <stdint.h>

namespace nice {

typedef uint32_t u32;
typedef uint64_t u64;
typedef unsigned __int128 u128;

constexpr int cdiv(int a, int b) { return (a + b - 1) / b; }

// Detailed histograms: rows of kHistBins u64 bins (bin u = numbers with u
// unique digits, u <= 128).  A field's state block holds kHistCopies rows
// (summed at its end); a workgroup flushes into copy blockIdx.x % kHistCopies.
constexpr uint32_t kHistBins = 129;
constexpr uint32_t kHistCopies = 64;

// Detailed result words (u64, mapped host memory; FieldFinish::out_mapped,
// Slot::h_fin): the summed histogram in [0, kHistBins), then
constexpr uint32_t kFinCount = 129;  // the near-miss count
constexpr uint32_t kFinSeq = 130;    // the field's sequence word (untagged fields)
constexpr uint32_t kFinWords = 132;

// Arrival counters of the in-kernel finishes (nice_device.hpp
// last_block_arrive): done[0], then one counter per workgroup group.
constexpr uint32_t kDoneGroups = 64, kDoneWords = kDoneGroups + 1;

// Device MSD counter block (u32 words; MsdLaunch::counters):
//   [0, kMsdLevels)   level sizes ([0] the level-0 size; per batch)
//   kMsdLeafCount     leaf records (per batch)
//   kMsdOverflow      overflow flag (sticky over the field, as is all below)
//   kMsdRanges        MSD-surviving ranges
//   kMsdSquareOk      square survivors (written at the field's end)
//   kMsdCandidates    u64 candidates
//   kMsdNumbers       u64 numbers inside the ranges
//   kMsdSquareParts   kMsdSquarePartCount square-survivor partial counts
//                     (workgroup b adds to kMsdSquareParts + b % kMsdSquarePartCount)
//   kMsdRejected      u64 candidates rejected by the sound filter's prefix test
//                     (copied out to mapped words kMsdMappedRejected, +1)
constexpr uint32_t kMsdLevels = 24;
constexpr uint32_t kMsdLeafCount = 24;
constexpr uint32_t kMsdOverflow = 25;
constexpr uint32_t kMsdRanges = 26;
constexpr uint32_t kMsdSquareOk = 27;
constexpr uint32_t kMsdCandidates = 28;
constexpr uint32_t kMsdNumbers = 30;
constexpr uint32_t kMsdSquareParts = 32, kMsdSquarePartCount = 64;
constexpr uint32_t kMsdRejected = 96;
constexpr uint32_t kMsdCounterWords = 98;
// Its mapped copy at a field's end (NiceFinish::msd_mapped, Slot::h_msd):
// words [0, kMsdSquareParts) at the counter block's indices, then the
// rejected pair.
constexpr uint32_t kMsdMappedRejected = 32;
constexpr uint32_t kMsdMappedWords = 34;

// A leaf's candidate count is capped at kLeafPiece: longer runs are stored as
// several leaves, so niceonly_kernel's per-wave sums of 8 leaves fit 32 bits.
constexpr uint32_t kLeafPiece = 1u << 28;

// msd_fused_kernel: the most nodes a level of a chunk's recursion may hold
// (msd_plan.hpp msd_fused_cap).
constexpr uint32_t kFusedMaxCap = 1u << 14;

// msd_wave_kernel (niceonly_wave.hpp): threads per workgroup -- the pair table
// (<= 23 KB) is shared by 8 waves, two workgroups per CU at 4 waves per SIMD.
constexpr uint32_t kWaveWG = 512;
// Its work stack per wave: a pop takes <= 64 nodes off the top and pushes <= 128
// one level deeper, so at most ~64 nodes per level stay behind (23 levels) plus
// one refill of 64 roots; overflow sets the MSD overflow flag (an error).
constexpr uint32_t kStackCap = 2048;
constexpr uint32_t kStackNodeBytes = 16;  // sizeof(StackNode)

static_assert(kFinCount == kHistBins && kFinSeq > kFinCount && kFinWords > kFinSeq, "result words follow the bins");
static_assert(kMsdLeafCount == kMsdLevels && kMsdSquareOk < kMsdCandidates, "u32 counters follow the level sizes");
static_assert(kMsdCandidates % 2 == 0 && kMsdNumbers % 2 == 0 && kMsdRejected % 2 == 0 &&
                  kMsdMappedRejected % 2 == 0,
              "u64 counters are 8-byte aligned");
static_assert(kMsdNumbers + 2 == kMsdSquareParts, "the partials follow the u64 counters");
static_assert(kMsdSquareParts + kMsdSquarePartCount == kMsdRejected, "the partials end where the rejected count begins");
static_assert(kMsdRejected + 2 == kMsdCounterWords, "the rejected count ends the block");
static_assert(kMsdMappedRejected == kMsdSquareParts && kMsdMappedWords == kMsdMappedRejected + 2,
              "the mapped block is the first 32 words plus the rejected pair");

}  // namespace nice
