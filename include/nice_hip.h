/*
 * nice_hip.h -- C ABI of libnice_hip.so, the MI355X (gfx950) field-processing
 * path of wasabipesto/nice.
 *
 * This is the drop-in boundary: plain pointers, sizes and u64 pairs, no torch
 * or HIP types, so a cgo / Rust FFI / ctypes binding can call it directly
 * (INTEGRATION.md shows the Rust `extern "C"` shim the reference would add).
 * Every entry point cites the reference interface it replaces
 * (paths relative to the reference repository root).
 *
 * Conventions
 *  - u128 values are passed as (lo, hi) u64 pairs, the split the reference
 *    GPU path already uses (common/src/client_process_gpu.rs:492-499).
 *  - Ranges are half-open [start, end) like FieldSize (common/src/lib.rs:84-153).
 *  - Every call returns NICE_OK (0) or an error code; nice_last_error() gives
 *    a thread-local message (the reference returns anyhow::Result,
 *    client_process_gpu.rs:777-782, 860-862).
 *  - Output lists are caller-allocated with a capacity; *n_out always receives
 *    the true length.  If it exceeds the capacity the call returns
 *    NICE_ERR_CAPACITY (never a silent truncation) and the caller may retry
 *    with a larger buffer.
 */
#ifndef NICE_HIP_H
#define NICE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NICE_OK 0
#define NICE_ERR_INVALID 1     /* bad argument (empty range, base out of 2..128, ...) */
#define NICE_ERR_HIP 2         /* HIP runtime / kernel failure */
#define NICE_ERR_CAPACITY 3    /* caller's output list too small; *n_out = needed */
#define NICE_ERR_NO_DEVICE 4   /* no usable GPU */
#define NICE_ERR_MSD_OVERFLOW 5 /* device MSD work queues overflowed (msd_floor too small for
                                   chunk_size); not retryable with a larger list */
#define NICE_ERR_BUSY 6         /* *_submit: every slot of the context holds a field in flight;
                                   collect one and submit again (the synchronous calls wait
                                   for a slot instead, see nice_process_range_detailed) */

/* NiceNumberSimple (common/src/lib.rs:182-186). */
typedef struct {
    uint64_t number_lo;
    uint64_t number_hi;
    uint32_t num_uniques;
    uint32_t reserved;
} nice_number;

typedef struct nice_ctx nice_ctx;

/* GpuContext::new(device_ordinal) (client_process_gpu.rs:215-244), extended to a
 * list of devices: a field is sharded into contiguous n-ranges, one per device.
 * No JIT happens here or later: kernels are AOT-built for gfx950. */
int nice_ctx_create(const int *devices, int n_devices, nice_ctx **out);
void nice_ctx_destroy(nice_ctx *ctx);
/* Wait until every stream of the context is idle (the fields in flight have
 * finished on the device; their results still wait for *_collect).  The
 * reference's one-stream context synchronises inside each call
 * (client_process_gpu.rs:858-866); callers timing a pipeline bracket it with this. */
int nice_ctx_synchronize(nice_ctx *ctx);
int nice_device_count(int *out);
const char *nice_last_error(void);

/* process_range_detailed_gpu(&GpuContext, &FieldSize, base) -> FieldResults
 * (client_process_gpu.rs:812-897; CPU semantics client_process.rs:150-191).
 * hist receives base+1 u64 counts indexed by num_uniques (bin 0 is always 0;
 * FieldResults.distribution is bins 1..=base).  out receives the near-misses
 * (num_uniques > floor(base * 0.9f)) in ascending order of number.
 * Thread-safe on a shared context (the reference shares its GpuContext across
 * the client's tasks behind a Mutex, client/src/main.rs:622,
 * client_process_gpu.rs:199-200): when every slot holds a field in flight the
 * call blocks until another thread's collect frees one.  It returns
 * NICE_ERR_BUSY instead only when no other thread could free a slot, which
 * would otherwise deadlock: no field in flight is being collected, and each
 * was submitted by the calling thread or by a thread that is itself blocked
 * in such a call (two threads holding tickets and waiting for each other's
 * slots: the second to call gets NICE_ERR_BUSY). */
int nice_process_range_detailed(nice_ctx *ctx, uint64_t start_lo, uint64_t start_hi,
                                uint64_t end_lo, uint64_t end_hi, uint32_t base,
                                uint64_t *hist, nice_number *out, size_t cap, size_t *n_out);

/* Niceonly tuning (all zero = reference CPU-path semantics, which make the
 * candidate set identical to process_range_niceonly's):
 *   msd_floor  MSD recursion floor; 0 -> NICE_GPU_MSD_FLOOR from the
 *              environment when set to a number >= 1 (the reference's pin,
 *              client_process_gpu.rs:161-172), else 250 (msd_prefix_filter.rs:282);
 *              NICE_MSD_FLOOR_ADAPTIVE -> the reference GPU path's adaptive
 *              floor (AdaptiveFloor, client_process_gpu.rs:96-184, 551-568):
 *              process-wide, pinned by NICE_GPU_MSD_FLOOR, else seeded at
 *              512 000 / logical cores in [250, 256 000]; after 3 warmup
 *              fields every host-MSD field moves it by msd / gpu-tail time
 *              (nice_adaptive_floor_step).  Device-MSD fields use it without
 *              updating it: their recursion is not a host phase to balance.
 *              A floor above 250 checks a superset of the candidates; the
 *              nice list is unchanged.
 *   chunk_size MSD chunking of the field; 0 -> reference client rule
 *              1e6 * clamp(ceil(size / 1e11), 1, 1000) (client/src/main.rs:158-168)
 *   threads    host MSD worker threads; 0 -> available parallelism (the
 *              affinity mask capped by the cgroup cpu.max quota, as Rust's
 *              std::thread::available_parallelism, client_process_gpu.rs:598;
 *              nice_host_threads)
 *   stride_k   LSD digits in the stride table; 0 -> 2 (client/src/main.rs:19)
 *   msd_where  where the MSD recursion runs: 0 auto (device for stride_k 2),
 *              1 host worker threads, 2 device (level-synchronous kernels)
 *   deal_stride, deal_offset
 *              process only the field's chunks c with c % deal_stride ==
 *              deal_offset (0 / 0 -> every chunk).  Rank r of an N-way job
 *              passes (N, r) with the whole field's bounds: the chunk grid and
 *              hence every chunk's MSD ranges are those of the single-process
 *              run, and survival skew along the field is spread over ranks (the
 *              reference deals descriptors from a shared channel,
 *              client_process_gpu.rs:589-709).
 *   filter     NICE_FILTER_REFERENCE (0): the reference's MSD filter bit for
 *              bit, Filter C included -- the MSD x LSD collision check
 *              (msd_prefix_filter.rs:474-559) that drops a whole range when
 *              first / b^2 == last / b^2, judging every number of it by the two
 *              lowest digits of *first*'s square and cube.  That condition
 *              fixes the high digits of n, not n mod b^2, so the reference can
 *              drop numbers it has not ruled out.
 *              NICE_FILTER_SOUND (1): a complete answer.  The recursion ends
 *              after the square / cube / overlap checks (no Filter C, on the
 *              device, the host MSD producer and every base), and on the
 *              compile-time kernels (device MSD, nice_niceonly_fast_base, field
 *              inside the base's range, stride_k 2) each stride candidate is
 *              tested against its own low digits instead: rejected iff the
 *              common leading digits of n^2 and of n^3 over its MSD range plus
 *              the two lowest digits of its n^2 and n^3 hold a repeat (a range
 *              of one number rejects nothing).  ranges / range_numbers /
 *              candidates count as before (every stride candidate of the
 *              surviving ranges); square_ok counts candidates that passed the
 *              prefix test with a repeat-free square;
 *              nice_niceonly_prefix_rejected gives the number rejected.
 *              Any other value: NICE_ERR_INVALID at submit.
 * Both MSD placements produce the same candidate set. */
#define NICE_FILTER_REFERENCE 0
#define NICE_FILTER_SOUND 1
#define NICE_MSD_FLOOR_ADAPTIVE UINT64_MAX
#define NICE_MSD_AUTO 0
#define NICE_MSD_HOST 1
#define NICE_MSD_DEVICE 2
typedef struct {
    uint64_t msd_floor;
    uint64_t chunk_size;
    int32_t threads;
    uint32_t stride_k;
    int32_t msd_where;
    uint32_t deal_stride;
    uint32_t deal_offset;
    uint32_t filter;
} nice_niceonly_opts;

typedef struct {
    uint64_t ranges;        /* MSD-surviving sub-ranges (get_valid_ranges output) */
    uint64_t range_numbers; /* numbers inside them */
    uint64_t candidates;    /* stride candidates checked on the GPU */
    uint32_t launches;
    uint32_t square_ok;     /* device MSD, in-range fast bases: candidates whose square alone
                               has no repeated digit (get_is_nice reached the cube scan),
                               mod 2^32; 0 where not counted (host MSD, other bases) */
    double msd_seconds;     /* until the last MSD worker finished (a field re-run after a
                               list overflow: its last run) */
    double total_seconds;
    uint64_t msd_floor;     /* the MSD recursion floor this field used */
    uint32_t msd_threads;   /* host MSD worker threads the field ran (0: device MSD) */
    uint32_t reruns;        /* times the field re-ran with grown device lists */
} nice_niceonly_stats;

/* AdaptiveFloor::update's step (client_process_gpu.rs:130-157): the floor
 * after a field whose MSD took msd_seconds of total_seconds -- ratio
 * msd / (total - msd), 1.5 when the GPU tail is under 2 ms, 1/1.5 when the
 * MSD is, clamped to [1/1.5, 1.5], the floor to [250, 256 000].  Pure. */
double nice_adaptive_floor_step(double floor, double msd_seconds, double total_seconds);
/* The process-wide adaptive floor now, and the warmup fields left
 * (0xffffffff: pinned by NICE_GPU_MSD_FLOOR). */
int nice_adaptive_floor(double *floor, uint32_t *warmup);

/* process_range_niceonly_gpu(&GpuContext, &FieldSize, base) -> FieldResults
 * (client_process_gpu.rs:515-557; CPU semantics client_process.rs:439-465).
 * Nice numbers (num_uniques = base) ascending.  Residue-empty bases return an
 * empty list (client_process_gpu.rs:525-531). */
int nice_process_range_niceonly(nice_ctx *ctx, uint64_t start_lo, uint64_t start_hi,
                                uint64_t end_lo, uint64_t end_hi, uint32_t base,
                                nice_number *out, size_t cap, size_t *n_out);
int nice_process_range_niceonly_ex(nice_ctx *ctx, uint64_t start_lo, uint64_t start_hi,
                                   uint64_t end_lo, uint64_t end_hi, uint32_t base,
                                   const nice_niceonly_opts *opts, nice_number *out,
                                   size_t cap, size_t *n_out, nice_niceonly_stats *stats);
/* NICE_FILTER_SOUND: the candidates the per-candidate prefix test rejected in
 * the niceonly field the calling thread collected last (nice_niceonly_collect
 * or a synchronous call; thread-local like nice_last_error, so fields collected
 * on other threads do not disturb it), summed over the context's devices; a
 * field re-run after a list overflow counts its last run, like the other
 * statistics.  0 for the reference filter and wherever sound mode runs without
 * the prefix test (run-time-base kernels, fields outside the base's range,
 * host MSD, stride_k != 2). */
uint64_t nice_niceonly_prefix_rejected(void);

/* The coordination server's submit checks for a detailed result
 * (api/src/main.rs:309-359), which nice_process_range_detailed also applies to
 * its own output before returning (plus the server's recompute of every listed
 * number, on the device): the histogram (base+1 bins) sums to the field size
 * (size_lo, size_hi); every listed number lies above the near-miss cutoff; for
 * each bin above the cutoff the count equals the number of listed entries with
 * that num_uniques; the list length equals the sum of those bins.
 * NICE_OK or NICE_ERR_INVALID with the failed check in nice_last_error(). */
int nice_validate_detailed(uint32_t base, uint64_t size_lo, uint64_t size_hi, const uint64_t *hist,
                           const nice_number *list, size_t n);

/* The reference's CPU API on the host cores, for callers without a GPU and
 * the reference client's CPU mode (cpu_path.cpp).  No device is touched, and
 * the GPU entry points above never fall back to these.
 *
 * process_range_detailed (common/src/client_process.rs:150-191): the
 * histogram of unique-digit counts (base+1 bins) and the numbers above the
 * near-miss cutoff, ascending -- same outputs as nice_process_range_detailed.
 *
 * process_range_niceonly (client_process.rs:439-465): get_valid_ranges over
 * the whole range (msd_prefix_filter.rs:665-674, floor 250), then every
 * candidate of the (b-1) * b^k stride table (stride_filter.rs:139-155; k =
 * stride_k, 0 -> 2) tested with get_is_nice; the nice numbers, ascending.
 *
 * threads: host threads (< 1 -> 1, the reference's single-threaded call);
 * the range (detailed) or the surviving MSD ranges (niceonly) are split
 * into contiguous pieces.  Errors: NICE_ERR_INVALID (base outside 2..128,
 * end < start), NICE_ERR_CAPACITY (*n_out = the required capacity). */
int nice_cpu_process_range_detailed(uint64_t start_lo, uint64_t start_hi, uint64_t end_lo,
                                    uint64_t end_hi, uint32_t base, int32_t threads,
                                    uint64_t *hist, nice_number *out, size_t cap, size_t *n_out);
int nice_cpu_process_range_niceonly(uint64_t start_lo, uint64_t start_hi, uint64_t end_lo,
                                    uint64_t end_hi, uint32_t base, uint32_t stride_k,
                                    int32_t threads, nice_number *out, size_t cap, size_t *n_out);
/* The same with nice_niceonly_opts.filter's values: NICE_FILTER_SOUND runs
 * get_valid_ranges without Filter C and tests every stride candidate of the
 * larger set (nice_cpu_process_range_niceonly is filter 0). */
int nice_cpu_process_range_niceonly_ex(uint64_t start_lo, uint64_t start_hi, uint64_t end_lo,
                                       uint64_t end_hi, uint32_t base, uint32_t stride_k,
                                       int32_t threads, uint32_t filter, nice_number *out, size_t cap,
                                       size_t *n_out);

/* Asynchronous fields.  *_submit enqueues a field on the context's devices
 * and returns at once with a ticket; *_collect waits for that field and
 * returns exactly what the synchronous call would (the synchronous entry
 * points above are submit + collect).  Up to three fields per mode may be in
 * flight on a context, each on its own stream, so a caller can keep the GPU
 * busy with fields i+1 and i+2 while it exchanges / submits the results of
 * field i -- the overlap the reference client gets from its pipelined loop
 * (client/src/main.rs:411-562) -- and a field's first workgroups fill the CUs
 * the previous field's last ones leave idle.  Tickets
 * are collected in any order; NICE_ERR_CAPACITY from a collect keeps the
 * results for a retry with a larger list.  Niceonly with msd_where = host runs
 * its host MSD producer inside submit. */
int nice_detailed_submit(nice_ctx *ctx, uint64_t start_lo, uint64_t start_hi, uint64_t end_lo,
                         uint64_t end_hi, uint32_t base, int *ticket);
int nice_detailed_collect(nice_ctx *ctx, int ticket, uint64_t *hist, nice_number *out, size_t cap,
                          size_t *n_out);
int nice_niceonly_submit(nice_ctx *ctx, uint64_t start_lo, uint64_t start_hi, uint64_t end_lo,
                         uint64_t end_hi, uint32_t base, const nice_niceonly_opts *opts, int *ticket);
int nice_niceonly_collect(nice_ctx *ctx, int ticket, nice_number *out, size_t cap, size_t *n_out,
                          nice_niceonly_stats *stats);

/* Device time of the hot kernel(s) of the last collected detailed field on a
 * device, measured with HIP events on the launch stream (kernel_ms 0 when the
 * field ran with kernel timing off). */
typedef struct {
    double kernel_ms;    /* summed over launches; 0 when the field was not timed */
    uint32_t launches;
    uint32_t fd_kernel;  /* 1 if the finite-difference kernel ran */
    uint64_t numbers;    /* numbers processed by those launches */
    uint32_t sib_lanes;  /* sibling lanes M of the FD kernel's last sibling-lane launch (0: none ran) */
    uint32_t sib_stride; /* ... and its lane stride L */
    uint32_t sib_grid;   /* ... and the workgroups of its persistent sibling grid (0: rounds of workgroups) */
} nice_kernel_stats;
int nice_last_kernel_stats(nice_ctx *ctx, int device_index, nice_kernel_stats *out);
/* Kernel timing of later detailed fields on this context (default on): with
 * it off a field records no HIP events -- two fewer runtime calls on the
 * submit path of every field, which is what a latency-bound caller of small
 * fields pays for (the reference client never reads kernel times) -- and
 * nice_last_kernel_stats reports kernel_ms 0. */
int nice_ctx_set_kernel_timing(nice_ctx *ctx, int enable);

/* Host helpers mirroring the reference functions the client calls. */
/* std::thread::available_parallelism() (client_process_gpu.rs:598): the
 * process's CPU affinity mask, capped by the cgroup v2 cpu.max quotas of its
 * cgroup and the cgroup's ancestors (quota / period rounded down, at least 1,
 * as Rust's std does).  The host MSD pool's size when
 * nice_niceonly_opts.threads is 0. */
uint32_t nice_host_threads(void);
/* Test hook: every later sibling-lane launch of the FD kernel in this
 * process uses lane stride L (odd, <= 255) instead of the bank-conflict
 * model's pick, and fields of >= 4 super-blocks take the sibling kernel
 * whatever their size; 0 restores production.  NICE_ERR_INVALID otherwise. */
int nice_debug_force_sib_stride(uint32_t L);
/* Test hook: the persistent grid of the FD kernel's sibling-lane launches in
 * this process (b40, first limb layout).  mode 0: production (the planner's
 * threshold decides); 1: every sibling-lane segment of >= 4 super-blocks runs
 * on it, with at most max_workgroups workgroups when that is nonzero; 2: never
 * (rounds of workgroups).  NICE_ERR_INVALID for another mode. */
int nice_debug_force_sib_persistent(uint32_t mode, uint32_t max_workgroups);
/* Test hook: the compile-time histogram window [w0, w0 + w) of the FD kernel
 * of `base`: unique counts inside it are counted in LDS, the others take the
 * kernel's out-of-window branch, which also lists the near-misses.
 * NICE_ERR_INVALID for a base without an FD kernel.  No device needed. */
int nice_debug_fd_window(uint32_t base, uint32_t *w0, uint32_t *w);
/* Test hook: every later GPU detailed call of this process at `base`
 * (nice_process_range_detailed, nice_detailed_submit / _collect,
 * nice_process_ranges_detailed and its per-range fallbacks) lists the numbers
 * with num_uniques > cutoff instead of > nice_near_miss_cutoff(base) -- the
 * FD and the generic launches of a field alike, and the self-check of the
 * result runs against the same cutoff.  The histograms do not change.  With
 * cutoff = w0 + w - 1 every number on the high out-of-window branch is listed,
 * so a test sees the list code that production takes about once in 1e8
 * numbers.  0 restores production for that base.  NICE_ERR_INVALID when the
 * base has no FD kernel or cutoff is neither 0 nor in [w0 + w - 1, base - 1].
 * Set it with no field of that base in flight (a field submitted under one
 * cutoff and collected under another fails its self-check).  The CPU API,
 * niceonly and nice_validate_detailed keep the production cutoff.  No device
 * needed to set it. */
int nice_debug_set_near_miss_cutoff(uint32_t base, uint32_t cutoff);
/* Test hook: every niceonly field of `base` submitted later in this process
 * that lies wholly inside the base's valid range lists, from the compile-time
 * kernels, every stride candidate whose square is repeat-free and whose digit
 * union of n^2 and n^3 has >= nice_min members, instead of only the nice
 * numbers (production compares with the base; in range the union cannot
 * exceed it, so `== base` and `>= base` are the same).  The candidates, ranges
 * and square_ok statistics do not change.  The listed entries keep
 * num_uniques = base, as every niceonly entry does: the list says which
 * numbers passed, not their counts.  The value is read once, when a field is
 * submitted: a re-run after list growth and a collect after the hook was
 * cleared still use it.  0 restores production for that base; valid non-zero
 * values are 1..base.  NICE_ERR_INVALID for a base that is not a
 * nice_niceonly_fast_base or a value above the base.  Fields that leave the
 * valid range, the run-time-base kernels, nice_cpu_process_range_niceonly and
 * nice_check_is_nice_inrange keep production semantics.  No device needed to
 * set it. */
int nice_debug_set_nice_min(uint32_t base, uint32_t nice_min);
/* Test hook: the cpu.max cap nice_host_threads applies for the cgroup
 * `cgroup_path` under a cgroup2 mount at `root` (0 = no quota). */
uint32_t nice_debug_cgroup_cpus(const char *root, const char *cgroup_path);
/* get_base_range_u128 (base_range.rs:43-54): 1 range, 0 none, -1 exceeds u128. */
int nice_base_range(uint32_t base, uint64_t *start_lo, uint64_t *start_hi, uint64_t *end_lo,
                    uint64_t *end_hi);
/* get_near_miss_cutoff (number_stats.rs:15-17). */
uint32_t nice_near_miss_cutoff(uint32_t base);
/* pub const GPU_BATCH_SIZE / PROCESSING_CHUNK_SIZE (client_process_gpu.rs:54, 59). */
uint64_t nice_gpu_batch_size(void);
uint64_t nice_processing_chunk_size(void);
/* gpu_supports_base (client_process_gpu.rs:473-476): every base 2..128 runs on
 * the GPU here (no CPU fallback). */
int nice_gpu_supports_base(uint32_t base);
/* 1 if detailed fields of this base inside its range use the FD kernel. */
int nice_fd_kernel_base(uint32_t base);
/* 1 if niceonly fields of this base inside its range use the compile-time
 * niceonly kernels (in-range limb paths, square-survivor queue: square_ok is
 * counted): every base with an FD kernel whose k = 2 stride table has a
 * residue -- 40 42 44 45 48 49 50 52 53 54 57 58 60 62 64 65 68 80.  Every
 * other base runs the run-time-base kernels (square_ok stays 0). */
int nice_niceonly_fast_base(uint32_t base);

/* Host MSD filter, get_valid_ranges_recursive (msd_prefix_filter.rs:583-674)
 * with max depth 22 and factor 2: writes (start_lo, start_hi, end_lo, end_hi)
 * quadruples, returns the true count via *n_out. */
int nice_msd_valid_ranges(uint64_t start_lo, uint64_t start_hi, uint64_t end_lo,
                          uint64_t end_hi, uint32_t base, uint64_t floor_size, uint64_t *out,
                          size_t cap, size_t *n_out);
/* The same with nice_niceonly_opts.filter's values (NICE_FILTER_SOUND: no
 * Filter C); nice_msd_valid_ranges is filter 0. */
int nice_msd_valid_ranges_ex(uint64_t start_lo, uint64_t start_hi, uint64_t end_lo,
                             uint64_t end_hi, uint32_t base, uint64_t floor_size, uint32_t filter,
                             uint64_t *out, size_t cap, size_t *n_out);
/* has_duplicate_msd_prefix (msd_prefix_filter.rs:382-563): 1 skippable, 0 not. */
int nice_msd_skippable(uint64_t start_lo, uint64_t start_hi, uint64_t end_lo, uint64_t end_hi,
                       uint32_t base);
/* StrideTable::new(base, k) (stride_filter.rs:40-87): modulus and residue count. */
int nice_stride_table(uint32_t base, uint32_t k, uint64_t *modulus, uint32_t *residues,
                      size_t cap, size_t *n_out);

/* Test hooks (no device needed): the in-range fast paths of the niceonly
 * kernels (radix_fast.hpp) evaluated on the host, for the bases of
 * nice_niceonly_fast_base with n (and [start, end)) inside the base's valid
 * range.  is_nice: 1/0 like get_is_nice
 * (client_process.rs:222-253); msd: 1/0 like has_duplicate_msd_prefix on
 * [start, end - 1] (msd_prefix_filter.rs:382-563); unique: the unique-digit
 * count of n^2 and n^3 by the same limb path (get_num_unique_digits,
 * client_process.rs:47-143).  NICE_ERR_INVALID otherwise. */
int nice_check_is_nice_inrange(uint32_t base, uint64_t n_lo, uint64_t n_hi);
int nice_check_unique_inrange(uint32_t base, uint64_t n_lo, uint64_t n_hi);
int nice_check_msd_skippable_inrange(uint32_t base, uint64_t start_lo, uint64_t start_hi,
                                     uint64_t end_lo, uint64_t end_hi);
/* NICE_FILTER_SOUND's per-candidate prefix test by the device code's leaf-mask
 * and rejection logic (radix_fast.hpp msd_prefix_masks / prefix_rejects, the
 * stride table's low-digit mask): 1 if n of the MSD leaf [start, end) is
 * rejected, 0 if not; NICE_ERR_INVALID unless start <= n < end lie inside the
 * valid range of a nice_niceonly_fast_base base. */
int nice_check_prefix_reject_inrange(uint32_t base, uint64_t start_lo, uint64_t start_hi,
                                     uint64_t end_lo, uint64_t end_hi, uint64_t n_lo, uint64_t n_hi);
/* Limb-count cuts of the production FD kernel (fd2_detailed.hip): the n at
 * which a segment ending there needs a wider (D1, E1, E2) limb layout.  Writes
 * (lo, hi) pairs, returns the count via *n_out.  Bases without an FD kernel: 0. */
int nice_fd_segment_cuts(uint32_t base, uint64_t *out, size_t cap, size_t *n_out);

/* Batched detailed ranges: many (small) ranges in one call.  `bounds` holds
 * four u64 per range -- start_lo, start_hi, end_lo, end_hi, the layout
 * nice_msd_valid_ranges writes, so its output can be passed straight in.
 * Ranges inside the valid range of a base with an FD kernel run together: one
 * kernel launch per limb layout present, each workgroup working for one range
 * and adding to that range's own histogram row.  Every other range (a base
 * without an FD kernel, a range outside the base's valid range or across one
 * of its ends; also a range of more than 2^28 numbers, which fills the GPU as
 * a field of its own) runs through nice_process_range_detailed's path inside
 * the call and is counted in nice_ranges_stats.fallback_ranges.
 *   NICE_RANGES_PER_RANGE: hist receives n_ranges rows of base + 1 u64; row i
 *     is, bin for bin, nice_process_range_detailed's histogram of range i.
 *   NICE_RANGES_SUM: hist receives one row, the sum over the ranges.
 * The list is the concatenation, in range order, of each range's near-misses
 * in ascending order; out_range[j] (may be null) is entry j's range index.
 * Ranges may overlap or repeat: each gets its own complete answer.  Every row
 * passes nice_validate_detailed before the call returns.
 * Errors: NICE_ERR_INVALID (n_ranges 0 or above 2^20, an empty or inverted
 * range -- the message names its index --, base outside 2..128),
 * NICE_ERR_CAPACITY (*n_out = the needed length; the results are kept, and
 * the same call with room returns them without running again).
 * The call has its own stream and buffers per device and its own lock: it
 * takes no detailed slot for the batched ranges and does not wait for fields
 * in flight. */
#define NICE_RANGES_PER_RANGE 0
#define NICE_RANGES_SUM 1
int nice_process_ranges_detailed(nice_ctx *ctx, uint32_t base, const uint64_t *bounds,
                                 size_t n_ranges, uint32_t flags, uint64_t *hist,
                                 nice_number *out, uint32_t *out_range, size_t cap,
                                 size_t *n_out);
typedef struct {
    uint32_t launches;        /* batch-kernel launches of the last call */
    uint32_t fallback_ranges; /* ranges run by the per-field path */
    uint64_t numbers;
    double kernel_ms;         /* HIP events around the batch launches */
} nice_ranges_stats;
int nice_last_ranges_stats(nice_ctx *ctx, nice_ranges_stats *out);
/* The same on the host cores (no device): loops nice_cpu_process_range_detailed. */
int nice_cpu_process_ranges_detailed(uint32_t base, const uint64_t *bounds, size_t n_ranges,
                                     uint32_t flags, int32_t threads, uint64_t *hist,
                                     nice_number *out, uint32_t *out_range, size_t cap,
                                     size_t *n_out);
/* Test hook (no device): the batch plan of nice_process_ranges_detailed for in-range
 * ranges of an FD base.  Writes 6 u64 per workgroup: start_lo, start_hi, lanes, chunk,
 * range index, combo index.  *n_out = the true count. */
int nice_debug_ranges_plan(uint32_t base, const uint64_t *bounds, size_t n_ranges,
                           uint64_t *units, size_t cap, size_t *n_out);

/* Batched niceonly ranges: the niceonly twin of nice_process_ranges_detailed,
 * and the seam for a caller that keeps its own MSD producer (the reference's
 * GPU pipeline hands its kernel only the surviving ranges,
 * client_process_gpu.rs:589-796).  `bounds` holds four u64 per range --
 * start_lo, start_hi, end_lo, end_hi, the layout nice_msd_valid_ranges writes,
 * so its output can be passed straight in.
 * No MSD filter runs on a range: every stride candidate of every range -- the
 * (b - 1) * b^k table with k = stride_k, 0 meaning 2 -- gets the full test,
 * which is the contract of the reference's niceonly_ranges_kernel
 * (nice_kernels.cu:420-470): the caller did the filtering.  So there is no
 * filter option: Filter C belongs to the MSD recursion.  The sound filter's
 * per-candidate prefix test does run on a caller's ranges, through
 * nice_process_ranges_niceonly_ex below.
 *   candidates[i] (may be null): the stride candidates in range i.
 *   square_ok[i] (may be null): how many of them have a repeat-free square,
 *     counted where the field path counts it -- a nice_niceonly_fast_base, the
 *     range wholly inside the base's valid range, k = 2 -- and 0 elsewhere.
 * Those ranges run the base's compile-time kernel and are counted in
 * nice_ranges_niceonly_stats.fast_ranges; every other range runs the
 * run-time-base test (generic_ranges).  Each group's leaves are dealt to the
 * context's devices in contiguous runs balanced by candidates: at most two
 * launches per device.
 * The list is the concatenation, in range order, of each range's passing
 * numbers in ascending order; out_range[j] (may be null) is entry j's range
 * index; num_uniques is the base, as in every niceonly entry.  Ranges may
 * overlap or repeat: each gets its own complete answer, so a number inside two
 * ranges is listed twice.  nice_debug_set_nice_min applies exactly as it does
 * to a field submitted at that moment (the fast ranges list union counts >=
 * nice_min).  A residue-empty base returns all-zero counts and an empty list
 * with no launch.
 * Errors: NICE_ERR_INVALID (n_ranges 0 or above 2^20; an empty or inverted
 * range -- the message names its index --; a range holding more than 2^40
 * candidates, or a call of more than 2^24 leaf records: use a field instead;
 * a stride modulus above u32; a base outside 2..128), NICE_ERR_CAPACITY
 * (*n_out = the needed length; the results are kept, and the same call with
 * room returns them without running again).
 * The call has its own stream, buffers and lock per device: it takes no
 * niceonly slot and does not wait for fields in flight. */
int nice_process_ranges_niceonly(nice_ctx *ctx, uint32_t base, const uint64_t *bounds,
                                 size_t n_ranges, uint32_t stride_k, uint64_t *candidates,
                                 uint32_t *square_ok, nice_number *out, uint32_t *out_range,
                                 size_t cap, size_t *n_out);
typedef struct {
    uint32_t launches;       /* kernel launches of the last call that ran (a retry after
                                NICE_ERR_CAPACITY returns kept results and leaves the statistics) */
    uint32_t fast_ranges;    /* ranges run by the base's compile-time kernel (square_ok counted) */
    uint32_t generic_ranges; /* ranges run by the run-time-base test */
    uint32_t reserved;
    uint64_t candidates;     /* summed over the ranges */
    uint64_t square_ok;
    double kernel_ms;        /* HIP events around the launches (the slowest device) */
} nice_ranges_niceonly_stats;
int nice_last_ranges_niceonly_stats(nice_ctx *ctx, nice_ranges_niceonly_stats *out);

/* nice_process_ranges_niceonly with options: the sound filter's per-candidate
 * prefix test (NICE_FILTER_SOUND above) per caller range, so that
 * nice_msd_ranges(..., NICE_FILTER_SOUND) composed with this call tests what a
 * device-MSD sound field tests.
 * The rule needs no recursion: for any range [s, e) of >= 2 numbers inside a
 * base's valid range every n has n^2 beginning with the common leading digits
 * of s^2 and (e - 1)^2 (P2; none when their digit counts differ) and n^3 with
 * those of the two cubes (P3).  With L the two lowest digits of n^2 and of n^3,
 * n is rejected iff the list P2 + P3 + L holds a repeated value -- then n^2 or
 * n^3 repeats a digit, or they share one, so no rejected n is nice.  A range of
 * one number rejects nothing.
 * prefix_test = NICE_RANGES_PREFIX_ON runs it exactly where the field path runs
 * it: a nice_niceonly_fast_base, the k = 2 table, the range wholly inside the
 * valid range (the ranges nice_ranges_niceonly_stats.fast_ranges counts).
 * There a mask kernel makes each range's digit mask of P2 + P3 in a launch of
 * its own before the candidate launch, whose prefix-testing variant rejects
 * candidates ahead of the square test.  Every other range is tested as
 * nice_process_ranges_niceonly tests it.
 *   candidates[i]: unchanged, every stride candidate of range i.
 *   prefix_rejected[i] (may be null): the candidates of range i the rule
 *     rejects; 0 for a range the test does not run on.
 *   square_ok[i]: the KEPT candidates with a repeat-free square (the sound
 *     field's square_ok).
 *   the list: the kept candidates that pass -- in production the list of the
 *     call with the test off; under nice_debug_set_nice_min the kept square
 *     survivors with a union count >= nice_min.
 * prefix_test = NICE_RANGES_PREFIX_OFF, or opts null (all zero): bit for bit
 * nice_process_ranges_niceonly (prefix_rejected all zero).  Any other value:
 * NICE_ERR_INVALID, as are non-zero reserved words.  Limits, errors, locking,
 * device dealing and the capacity retry (the kept results include
 * prefix_rejected) are nice_process_ranges_niceonly's; both calls share the
 * kept results, so a retry must repeat the options too. */
#define NICE_RANGES_PREFIX_OFF 0
#define NICE_RANGES_PREFIX_ON 1
typedef struct {
    uint32_t stride_k;    /* 0: 2 */
    uint32_t prefix_test; /* NICE_RANGES_PREFIX_* */
    uint32_t reserved[2]; /* zero */
} nice_ranges_niceonly_opts;
int nice_process_ranges_niceonly_ex(nice_ctx *ctx, uint32_t base, const uint64_t *bounds,
                                    size_t n_ranges, const nice_ranges_niceonly_opts *opts,
                                    uint64_t *candidates, uint32_t *square_ok,
                                    uint64_t *prefix_rejected, nice_number *out,
                                    uint32_t *out_range, size_t cap, size_t *n_out);
/* The prefix test's part of the last call that ran (all zero when it was off;
 * nice_last_ranges_niceonly_stats describes the candidate launches as before,
 * its kernel_ms spanning the mask launch too). */
typedef struct {
    uint32_t prefix_ranges; /* ranges the test ran on */
    uint32_t launches;      /* mask-kernel launches: one per device that had such ranges */
    uint64_t rejected;      /* prefix_rejected summed over the ranges */
    double mask_ms;         /* HIP events around the mask launch (the slowest device) */
} nice_ranges_niceonly_prefix_stats;
int nice_last_ranges_niceonly_prefix(nice_ctx *ctx, nice_ranges_niceonly_prefix_stats *out);
/* nice_process_ranges_niceonly_ex on the host cores (no device), `threads`
 * instead of ctx.  The test runs on the same ranges as on the GPU, so
 * prefix_rejected equals the GPU's; square_ok is counted for every range (for
 * the kept candidates where the test ran). */
int nice_cpu_process_ranges_niceonly_ex(uint32_t base, const uint64_t *bounds, size_t n_ranges,
                                        const nice_ranges_niceonly_opts *opts, int32_t threads,
                                        uint64_t *candidates, uint32_t *square_ok,
                                        uint64_t *prefix_rejected, nice_number *out,
                                        uint32_t *out_range, size_t cap, size_t *n_out);

/* nice_process_ranges_niceonly on the host cores (no device): the stride walk of
 * stride_filter.rs:139-155 over each range with get_is_nice, the ranges spread
 * over `threads`.  square_ok is counted for every range. */
int nice_cpu_process_ranges_niceonly(uint32_t base, const uint64_t *bounds, size_t n_ranges,
                                     uint32_t stride_k, int32_t threads, uint64_t *candidates,
                                     uint32_t *square_ok, nice_number *out, uint32_t *out_range,
                                     size_t cap, size_t *n_out);
/* Test hook (no device): the leaf plan of nice_process_ranges_niceonly on a
 * context of n_devices devices.  Writes 7 u64 per leaf: b0_lo, b0_hi (the
 * cycle base start - start mod M), g0, count, range index, group (1: fast, 0:
 * generic), device.  Leaves of the fast group first, each group in range
 * order.  *n_out = the true count. */
int nice_debug_ranges_niceonly_plan(uint32_t base, uint32_t stride_k, const uint64_t *bounds,
                                    size_t n_ranges, uint32_t n_devices, uint64_t *leaves,
                                    size_t cap, size_t *n_out);

/* The per-number map: out[i] = the unique-digit count of n^2 and n^3 of
 * n = start + i, the value get_num_unique_digits returns
 * (client_process.rs:47-143) -- 1..base, one byte for every base <= 128 --
 * for every n of [start, end), at most 2^32 of them.  Every aggregate the
 * other calls return follows from it: bincount(out) is
 * nice_process_range_detailed's histogram of the range, the positions with
 * out[i] > nice_near_miss_cutoff(base) its list; and so does every statistic
 * they do not return (the count against n mod (b - 1), against the low or the
 * leading digits) without further device code.
 * Any base 2..128 and any n: the parts of the range inside the valid range of
 * a base with an FD kernel (nice_fd_kernel_base) run that kernel's arithmetic
 * (fd2_map_kernel: the limb walk of the detailed kernel, a byte stored per n
 * instead of the histogram), cut at the limb layouts nice_fd_segment_cuts
 * reports; every other part runs the generic per-n device function.
 * nice_map_stats says which ran.
 *   NICE_MAP_HOST: `out` is host memory.  The range is sharded contiguously
 *     over the context's devices, as fields are, and each shard copied back.
 *     device_index is ignored.
 *   NICE_MAP_DEVICE: `out` is device memory on the context's device number
 *     device_index (an index into the list the context was created with), of
 *     any byte alignment.  That device writes the map in place; the call
 *     returns after its stream is idle, so any stream of the caller may read
 *     `out` straight away.  No byte outside out[0, end - start) is written.
 * Errors: NICE_ERR_INVALID (an empty or inverted range, base outside 2..128,
 * more than 2^32 numbers, a flag other than the two, a device_index outside
 * the context in device mode, a null out), NICE_ERR_CAPACITY (cap < end -
 * start: nothing is written).
 * The call has its own stream, buffers and lock per device: it takes no
 * detailed or niceonly slot and does not wait for fields in flight.  There is
 * no list, so nice_debug_set_near_miss_cutoff and the other hooks do not
 * apply. */
#define NICE_MAP_HOST 0
#define NICE_MAP_DEVICE 1
int nice_unique_map(nice_ctx *ctx, uint64_t start_lo, uint64_t start_hi, uint64_t end_lo,
                    uint64_t end_hi, uint32_t base, uint8_t *out, size_t cap, uint32_t flags,
                    int device_index);
/* The same on the host cores (no device): get_num_unique_digits per n, the
 * range split contiguously over `threads`.  The same errors. */
int nice_cpu_unique_map(uint64_t start_lo, uint64_t start_hi, uint64_t end_lo, uint64_t end_hi,
                        uint32_t base, int32_t threads, uint8_t *out, size_t cap);
typedef struct {
    uint32_t launches;         /* kernel launches of the last call */
    uint32_t fd_segments;      /* pieces run by the FD map kernel (one per limb layout and device) */
    uint32_t generic_segments; /* pieces run by the generic per-n kernel */
    uint32_t reserved;
    uint64_t fd_numbers;
    uint64_t generic_numbers;
    double kernel_ms;          /* HIP events around the launches (the slowest device) */
} nice_map_stats;
int nice_last_map_stats(nice_ctx *ctx, nice_map_stats *out);
/* Test hook (no device): the plan of nice_unique_map for [start, end) on one
 * device.  Writes 8 u64 per record, in ascending n: kind (0: a workgroup of
 * the FD map kernel, 1: a generic segment), start_lo, start_hi, the output
 * offset of the record's first number (n - start), lanes, chunk (numbers per
 * lane; a generic segment: 0, 0), combo index (the limb layout: the index of
 * the nice_fd_segment_cuts interval), numbers covered (FD: lanes * chunk).
 * *n_out = the true count.  The same argument errors as nice_unique_map. */
int nice_debug_map_plan(uint32_t base, uint64_t start_lo, uint64_t start_hi, uint64_t end_lo,
                        uint64_t end_hi, uint64_t *records, size_t cap, size_t *n_out);

/* The device MSD recursion's range list: what nice_msd_valid_ranges_ex returns,
 * for many roots per call, at device speed.  `roots` holds four u64 per root
 * -- start_lo, start_hi, end_lo, end_hi, the layout every ranges call uses.
 * Root i is one recursion root (depth 0, depth cap 22, factor 2): its answer is
 * exactly nice_msd_valid_ranges_ex(root i, base, floor_size, filter).  `out`
 * receives the concatenation of the roots' answers in root order, each root's
 * ranges ascending, as quadruples in the same layout, so it can be passed
 * unchanged as the `bounds` of nice_process_ranges_niceonly or
 * nice_process_ranges_detailed.  out_root[j] (may be null) is entry j's root
 * index, counts[i] (may be null) the number of ranges of root i.  Roots may
 * overlap or repeat: each gets its own complete answer.
 * The kernels run the node rule of the field kernels (classify_node with the
 * field kernels' template arguments for the base and the root's placement), so
 * the roots of a field's chunk grid give the ranges that field's niceonly run
 * tests.  filter: NICE_FILTER_REFERENCE or NICE_FILTER_SOUND; the sound filter
 * only leaves Filter C out of the recursion -- its per-candidate prefix test
 * is not part of a range list.
 * Roots of at most kFusedMaxCap - 2 floors run one workgroup per root, larger
 * ones a level BFS; the records are ordered on the device and only the ones
 * written are copied back.  On a context of several devices the roots are dealt
 * in contiguous runs balanced by numbers.  Buffers are sized from the bound of
 * size / floor_size + 1 leaves per root (2^22 at most, the depth cap), and a
 * call is cut into batches of roots of 2^27 such nodes (64 bytes of device
 * memory each, allocated as a call needs them): no valid call ends in
 * NICE_ERR_MSD_OVERFLOW.
 * Errors: NICE_ERR_INVALID (n_roots 0 or above 2^20; an empty or inverted
 * root -- the message names its index --; a root of more than 2^40 numbers;
 * floor_size 0; a filter other than the two; a base outside 2..128),
 * NICE_ERR_CAPACITY (*n_out = the needed length; the results are kept, and
 * the same call with room returns them without running again).
 * The call has its own stream, buffers and lock per device: it takes no
 * niceonly slot and does not wait for fields in flight. */
int nice_msd_ranges(nice_ctx *ctx, uint32_t base, const uint64_t *roots, size_t n_roots,
                    uint64_t floor_size, uint32_t filter, uint64_t *out, uint32_t *out_root,
                    uint64_t *counts, size_t cap, size_t *n_out);
/* The same on the host cores (no device): the host recursion root by root, the
 * roots spread over `threads`.  The same outputs and errors. */
int nice_cpu_msd_ranges(uint32_t base, const uint64_t *roots, size_t n_roots, uint64_t floor_size,
                        uint32_t filter, int32_t threads, uint64_t *out, uint32_t *out_root,
                        uint64_t *counts, size_t cap, size_t *n_out);
typedef struct {
    uint32_t launches;    /* recursion kernel launches of the last call that ran (level-0 and level
                             launches and the workgroup-per-root launches; the sort's are not counted;
                             a retry after NICE_ERR_CAPACITY returns kept results and leaves the
                             statistics) */
    uint32_t fused_roots; /* roots run one workgroup per root */
    uint32_t level_roots; /* roots run by the level BFS */
    uint32_t reserved;
    uint64_t ranges;      /* summed over the roots */
    uint64_t numbers;     /* the numbers inside them */
    double kernel_ms;     /* HIP events around the recursion launches, summed over the batches
                             (the slowest device) */
    double order_ms;      /* ... and around the device sort of the records */
} nice_msd_ranges_stats;
int nice_last_msd_ranges_stats(nice_ctx *ctx, nice_msd_ranges_stats *out);
/* Test hook (no device): the plan of nice_msd_ranges on a context of n_devices
 * devices.  Writes 4 u64 per root, in root order: root index, group (1: one
 * workgroup per root, 0: the level BFS), device, batch (counted per device).
 * *n_out = the true count.  The argument errors of nice_msd_ranges. */
int nice_debug_msd_ranges_plan(uint32_t base, const uint64_t *roots, size_t n_roots,
                               uint64_t floor_size, uint32_t n_devices, uint64_t *records,
                               size_t cap, size_t *n_out);

/* Diagnostics: per-n results of the device functions the kernels use. */
int nice_debug_unique_counts(nice_ctx *ctx, const uint64_t *n_pairs, uint32_t count,
                             uint32_t base, uint32_t *out);
int nice_debug_is_nice(nice_ctx *ctx, const uint64_t *n_pairs, uint32_t count, uint32_t base,
                       uint32_t *out);
/* The niceonly kernel's in-range limb path (nice_niceonly_fast_base bases, every n
 * inside the base's valid range, else NICE_ERR_INVALID): the unique-digit
 * count its niceness test compares with the base. */
int nice_debug_unique_fast(nice_ctx *ctx, const uint64_t *n_pairs, uint32_t count, uint32_t base,
                           uint32_t *out);
/* The niceonly kernels' cube pass (same bases and n): the count it compares
 * with the base (or with nice_debug_set_nice_min's value) -- the members of the
 * digit union of n^2 and n^3, 0 when n^2 repeats a digit -- through the LDS
 * pair table for the two-word bases (b <= 64) and by VALU for b65, b68, b80. */
int nice_debug_cube_count(nice_ctx *ctx, const uint64_t *n_pairs, uint32_t count, uint32_t base,
                          uint32_t *out);

#ifdef __cplusplus
}
#endif
#endif
