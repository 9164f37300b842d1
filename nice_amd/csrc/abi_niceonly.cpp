// abi_niceonly.cpp -- niceonly fields: device MSD (level kernels) or a
// multi-threaded host MSD producer -> stride-index leaves -> the candidate
// kernel; gather, submit / collect.
#include <cstdio>
#include <cstring>
#include <deque>

#include "abi_internal.hpp"
#include "msd_plan.hpp"

using namespace nice::abi;
using nice::u128;

namespace {

constexpr uint32_t kBatchRanges = 1u << 16;  // LAUNCH_BATCH_RANGES (client_process_gpu.rs:583)

// nice_niceonly_prefix_rejected(): the calling thread's last collected field
thread_local uint64_t t_prefix_rejected = 0;

// A niceonly job's bounds and options, resolved.
struct NiceField {
    u128 s = 0, e = 0;
    uint32_t base = 0;
    uint64_t floor = 0;  // MSD recursion floor
    uint32_t k = 2;      // stride table depth
    int threads = 1;     // host MSD producer pool
    u128 chunk = 0;      // MSD chunk size (the grid's origin is s)
    uint64_t deal_stride = 1, deal_offset = 0;
    uint64_t mine = 0;   // this caller's chunks of the field's grid: c = deal_offset + i * deal_stride
    bool sound = false;
    bool empty = false;  // nothing to run (residue-empty base, no chunk dealt): nothing below is set
    std::shared_ptr<nice::StrideTable> table;
    uint32_t in_range = 0;  // the whole field inside the base's valid range
    uint32_t nice_min = 0;  // NiceonlyLaunch::nice_min: the base, or the job's lowered value (in range)
    uint32_t R = 0, M = 0;  // residues per cycle, stride modulus

    // the tables' key in Device::residues / ranks / lowtabs
    uint32_t key() const { return base * 8 + k; }
    void chunk_range(uint64_t i, u128 &cs, u128 &ce) const {
        cs = s + (u128)(deal_offset + (u128)i * deal_stride) * chunk;
        ce = std::min(e, cs + chunk);
    }
};

int resolve_field(const NiceJob &job, NiceField &f) {
    const nice_niceonly_opts *opts = job.has_opts ? &job.opts : nullptr;
    f.s = job.s;
    f.e = job.e;
    f.base = job.base;
    f.floor = job.st.msd_floor;
    f.k = opts && opts->stride_k ? opts->stride_k : 2;
    // the reference sizes its MSD producer pool with available_parallelism()
    // (client_process_gpu.rs:598): on a 16-CPU cgroup of a 256-CPU host, 16
    f.threads = opts && opts->threads > 0 ? opts->threads : (int)available_parallelism();
    if (f.threads < 1) f.threads = 1;
    f.chunk = opts && opts->chunk_size ? (u128)opts->chunk_size : nice::client_chunk_size(f.e - f.s);
    f.deal_stride = opts && opts->deal_stride ? opts->deal_stride : 1;
    f.deal_offset = opts ? opts->deal_offset : 0;
    if (f.deal_offset >= f.deal_stride) return fail(NICE_ERR_INVALID, "deal_offset must be < deal_stride");
    f.sound = opts && opts->filter == NICE_FILTER_SOUND;
    const u128 nchunks_field = (f.e - f.s + f.chunk - 1) / f.chunk;
    const u128 mine128 = f.deal_offset < nchunks_field
                             ? (nchunks_field - f.deal_offset + f.deal_stride - 1) / f.deal_stride : 0;
    if (mine128 >> 63) return fail(NICE_ERR_INVALID, "too many MSD chunks");
    f.mine = (uint64_t)mine128;
    if (nice::residue_filter(f.base).empty() || f.mine == 0) {  // client_process_gpu.rs:525-531
        f.empty = true;
        return NICE_OK;
    }
    f.table = g_stride.get(f.base, f.k);
    // Whole field inside the base's valid range: the kernels take their
    // fixed-digit-count fast paths (radix_fast.hpp).
    u128 vr_s = 0, vr_e = 0;
    f.in_range = nice::base_range_cached(f.base, vr_s, vr_e) == 1 && vr_s <= f.s && f.e <= vr_e ? 1u : 0u;
    f.nice_min = f.in_range && job.nice_min ? job.nice_min : f.base;
    f.R = (uint32_t)f.table->residues.size();
    if (f.table->modulus > 0xffffffffull) return fail(NICE_ERR_INVALID, "stride modulus exceeds u32");
    f.M = (uint32_t)f.table->modulus;
    return NICE_OK;
}

int upload_words(const uint32_t *src, size_t n, uint32_t *&dst) {
    HIPCHK(hipMalloc(&dst, n * 4));
    HIPCHK(hipMemcpy(dst, src, n * 4, hipMemcpyHostToDevice));
    return NICE_OK;
}

// The field's stride table on a device, copied once per device and key:
// residues, ranks and (sound filter) the flagged residues + low-digit masks.
int upload_tables(Device &d, const NiceField &f) {
    const nice::StrideTable &table = *f.table;
    HIPCHK(hipSetDevice(d.id));
    const size_t R = table.residues.size();
    if (!d.residues.count(f.key())) {
        uint32_t *p = nullptr;
        if (int rc = upload_words(table.residues.data(), R, p)) return rc;
        d.residues[f.key()] = p;
        // rank[r] = lower_bound(residues, r): the device MSD turns a leaf's
        // end points into stride indices with one load each.
        std::vector<uint32_t> rank((size_t)table.modulus + 1);
        uint32_t g = 0;
        for (uint64_t r = 0; r <= table.modulus; r++) {
            while (g < R && table.residues[g] < r) g++;
            rank[r] = g;
        }
        if (int rc = upload_words(rank.data(), rank.size(), p)) return rc;
        d.ranks[f.key()] = p;
    }
    if (f.sound && !table.lowmask.empty() && !d.lowtabs.count(f.key())) {
        uint32_t *p;
        HIPCHK(hipMalloc(&p, (R + table.lowmask.size()) * 4));
        HIPCHK(hipMemcpy(p, table.residues_flagged.data(), R * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p + R, table.lowmask.data(), table.lowmask.size() * 4, hipMemcpyHostToDevice));
        d.lowtabs[f.key()] = p;
    }
    return NICE_OK;
}

int ensure_desc(LeafBuf &b, uint32_t cap) {
    if (b.cap >= cap) return NICE_OK;
    if (b.pending) HIPCHK(hipEventSynchronize(b.done));
    b.pending = false;
    if (int rc = grow_pinned(b.h, b.cap, cap, (size_t)cap * sizeof(nice::Leaf))) return rc;
    if (int rc = grow_device(b.d, b.cap, cap, (size_t)cap * sizeof(nice::Leaf))) return rc;
    if (!b.done) HIPCHK(hipEventCreateWithFlags(&b.done, hipEventDisableTiming));
    return NICE_OK;
}

// The slot's device MSD buffers, each grown to what the field needs; the
// slot's previous field may still be reading an old one, so its stream is
// drained before a buffer is freed.
int ensure_msd(Slot &sl, uint32_t q_cap, uint32_t leaf_cap, uint64_t scratch_nodes, size_t wscratch_bytes,
               bool masks) {
    MsdBuf &m = sl.msd;
    const uint32_t mask_cap = std::max(leaf_cap, m.leaf_cap);
    if (masks && m.mask_cap < mask_cap)
        if (int rc = grow_device(m.leaf_masks, m.mask_cap, mask_cap, (size_t)mask_cap * sizeof(nice::LeafMask),
                                 sl.nstream))
            return rc;
    if (!m.counters) HIPCHK(hipMalloc(&m.counters, nice::kMsdCounterWords * 4));
    if (m.wscratch_bytes < wscratch_bytes)
        if (int rc = grow_device(m.wscratch, m.wscratch_bytes, wscratch_bytes, wscratch_bytes, sl.nstream)) return rc;
    if (m.scratch_nodes < scratch_nodes)
        if (int rc = grow_device(m.scratch, m.scratch_nodes, scratch_nodes, scratch_nodes * sizeof(nice::ChunkNode),
                                 sl.nstream))
            return rc;
    if (m.q_cap < q_cap) {
        const size_t bytes = (size_t)q_cap * sizeof(nice::MsdNode);
        if (int rc = grow_device(m.q[0], m.q_cap, q_cap, bytes, sl.nstream)) return rc;
        if (int rc = grow_device(m.q[1], m.q_cap, q_cap, bytes)) return rc;
    }
    if (m.leaf_cap < leaf_cap)
        if (int rc = grow_device(m.leaves, m.leaf_cap, leaf_cap, (size_t)leaf_cap * sizeof(nice::Leaf), sl.nstream))
            return rc;
    return NICE_OK;
}

// What every candidate launch of the field on (d, sl) takes: the stride
// table and the output list.
nice::NiceonlyLaunch candidate_launch(const NiceField &f, Device &d, Slot &sl) {
    nice::NiceonlyLaunch p{};
    p.residues = d.residues[f.key()];
    p.R = f.R;
    p.M = f.M;
    p.base = f.base;
    p.in_range = f.in_range;
    p.nice_min = f.nice_min;
    p.out =nice::NumOut{sl.nice.n, nullptr, sl.d_nice_count, sl.nice.cap};
    return p;
}

// A device-MSD candidate launch's epilogue: re-zero the batch's leaf count;
// at the field's end (`last`) the results land in mapped memory instead (no
// copy launches).
nice::NiceFinish launch_finish(Slot &sl, bool last) {
    return nice::NiceFinish{last ? sl.d_msd_mapped : nullptr, last ? sl.d_nice_mapped : nullptr, sl.msd.counters,
                            sl.d_nice_done};
}

// The probe build's plan overrides (the product build reads no knob).
MsdPlanKnobs plan_knobs() {
    MsdPlanKnobs kn;
    if (nice::probe_set("NICE_MSD_CPB")) kn.cpb = std::max<uint64_t>(1, nice::probe_knob("NICE_MSD_CPB", 1));
    kn.nowave = nice::probe_set("NICE_MSD_NOWAVE");
    if (nice::probe_set("NICE_MSD_ROOTS")) kn.roots = nice::probe_knob("NICE_MSD_ROOTS", 1);
    return kn;
}

// Device MSD: batches of this caller's chunks, each run as init + the
// level kernels + the candidate kernel, all stream-ordered (no host sync
// until the end).  Batches alternate over the context's devices.
int run_device_msd(nice_ctx *ctx, int t, NiceJob &job, const NiceField &f, nice_niceonly_stats &st) {
    const size_t nd = ctx->devs.size();
    const uint64_t cnk = (uint64_t)f.chunk;
    const bool chunk_ok = f.chunk <= ((u128)1 << 40);
    const uint32_t fused_cap = !chunk_ok ? 0u
                               : nice::probe_set("NICE_MSD_FCAP") && cnk <= 0xffffffffull
                                   ? (uint32_t)nice::probe_knob("NICE_MSD_FCAP", 0)
                                   : nice::msd_fused_cap(cnk, f.floor);
    int max_cus = 0;
    for (auto &d : ctx->devs) max_cus = std::max(max_cus, d.num_cus);
    const MsdPlan pl = plan_device_msd(f.chunk, f.floor, f.mine, nd, max_cus, fused_cap,
                                                   nice::msd_wave_waves_per_group(), plan_knobs());
    // (reported in this order: chunk size, field size, chunk size against the floor)
    if (pl.error == kMsdChunkTooLarge) return fail(NICE_ERR_INVALID, pl.error);
    if ((f.e - f.s) >> 63) return fail(NICE_ERR_INVALID, "device MSD: field larger than 2^63");
    if (pl.error) return fail(NICE_ERR_INVALID, pl.error);
    // Sound filter: the prefix test where the field allows it (the probe
    // build's NICE_SOUND_NOPREFIX leaves it off, for the A/B)
    bool sound_fast = false;
    if (f.sound && !f.table->lowmask.empty()) {
        nice::MsdLaunch q{};
        q.end_hi = hi64(f.e);
        q.M = f.M;
        q.base = f.base;
        q.in_range = f.in_range;
        sound_fast = nice::sound_prefix_field(q);
    }
    const bool prefix = sound_fast && !nice::probe_set("NICE_SOUND_NOPREFIX");
    for (size_t i = 0; i < nd; i++) {
        Device &d = ctx->devs[i];
        Slot &sl = d.slot[t];
        HIPCHK(hipSetDevice(d.id));
        const uint64_t fgrid = nice::msd_fused_grid(pl.cpb, d.num_cus);
        int r = pl.fcap   ? ensure_msd(sl, 0, (uint32_t)pl.leaf_cap, fgrid * 2 * pl.fcap, 0, prefix)
                : pl.wave ? ensure_msd(sl, (uint32_t)pl.per, (uint32_t)pl.wleaf_cap, 0,
                                       nice::msd_wave_scratch_bytes(pl.wgrid), prefix)
                          : ensure_msd(sl, (uint32_t)pl.per, (uint32_t)pl.leaf_cap, 0, 0, prefix);
        if (r) return r;
        if (i < pl.nbatches) {
            job.used[i] = 1;
            if (sl.msd.dirty) {  // first use / after an interrupted field
                HIPCHK(hipMemsetAsync(sl.msd.counters, 0, nice::kMsdCounterWords * 4, sl.nstream));
                HIPCHK(hipMemsetAsync(sl.d_nice_count, 0, 4, sl.nstream));
            }
            sl.msd.dirty = true;  // until this field's epilogue is seen
        }
    }
    for (uint64_t bi = 0; bi < pl.nbatches; bi++) {
        Device &d = ctx->devs[bi % nd];
        Slot &sl = d.slot[t];
        const MsdBuf &mb = sl.msd;
        HIPCHK(hipSetDevice(d.id));
        const bool first = bi < nd;                // this device's first batch of the field
        const bool last = bi + nd >= pl.nbatches;  // ... and its last
        nice::MsdLaunch mp{};
        mp.first_batch = first ? 1u : 0u;
        mp.nice_count = sl.d_nice_count;
        mp.start_lo = lo64(f.s);
        mp.start_hi = hi64(f.s);
        mp.end_lo = lo64(f.e);
        mp.end_hi = hi64(f.e);
        mp.first = bi * pl.cpb;
        mp.nchunks = std::min(pl.cpb, f.mine - bi * pl.cpb);
        mp.deal_stride = f.deal_stride;
        mp.deal_offset = f.deal_offset;
        mp.chunk = cnk;
        mp.floor_size = f.floor;
        mp.q[0] = mb.q[0];
        mp.q[1] = mb.q[1];
        mp.counters = mb.counters;
        mp.q_cap = mb.q_cap;
        mp.leaves = mb.leaves;
        mp.leaf_cap = mb.leaf_cap;
        mp.residues = d.residues[f.key()];
        mp.ranks = d.ranks[f.key()];
        mp.R = f.R;
        mp.M = f.M;
        mp.base = f.base;
        mp.in_range = f.in_range;
        mp.probe = (uint32_t)nice::probe_knob("NICE_MSD_PROBE", 0);
        nice::SoundLaunch snd_launch{};
        if (f.sound) {
            if (prefix) {
                snd_launch.residues = d.lowtabs[f.key()];
                snd_launch.lowmask = snd_launch.residues + f.R;
                snd_launch.leaf_masks = mb.leaf_masks;
            }
            snd_launch.rejected = (unsigned long long *)(mb.counters + nice::kMsdRejected);
            snd_launch.fast = sound_fast ? 1u : 0u;
            snd_launch.prefix_test = prefix ? 1u : 0u;
        }
        const nice::SoundLaunch *snd = f.sound ? &snd_launch : nullptr;
        nice::NiceonlyLaunch p = candidate_launch(f, d, sl);
        p.fin = launch_finish(sl, last);
        if (pl.wave) {
            hipError_t err =
                nice::launch_msd_wave(mp, p, pl.wlevel, mb.wscratch, pl.wgrid, d.num_cus, sl.nstream, snd);
            if (err != hipSuccess)
                return fail(NICE_ERR_HIP, std::string("msd wave launch: ") + hipGetErrorString(err));
            st.launches++;
            continue;
        }
        const uint32_t fgrid = (uint32_t)nice::msd_fused_grid(mp.nchunks, d.num_cus);
        hipError_t err = pl.fcap ? nice::launch_msd_device(mp, d.num_cus, sl.nstream, mb.scratch, pl.fcap, fgrid, snd)
                                 : nice::launch_msd_device(mp, d.num_cus, sl.nstream, nullptr, 0, 0, snd);
        if (err != hipSuccess) return fail(NICE_ERR_HIP, std::string("msd launch: ") + hipGetErrorString(err));
        p.leaves = mb.leaves;
        p.n_leaves_dev = mb.counters + nice::kMsdLeafCount;
        p.n_leaves = mb.leaf_cap;  // clamp for the device count
        err = nice::launch_niceonly(p, d.num_cus, sl.nstream, snd);
        if (err != hipSuccess) return fail(NICE_ERR_HIP, std::string("niceonly launch: ") + hipGetErrorString(err));
        st.launches++;
    }
    for (size_t i = 0; i < nd; i++) {
        if (!job.used[i]) continue;
        Device &d = ctx->devs[i];
        HIPCHK(hipSetDevice(d.id));
        HIPCHK(hipEventRecord(d.slot[t].nice_done, d.slot[t].nstream));
    }
    return NICE_OK;
}

// The host MSD consumer: surviving ranges waiting for a launch, handed to the
// context's devices round-robin.
struct HostMsd {
    nice_ctx *ctx;
    int t;
    NiceJob &job;
    const NiceField &f;
    nice_niceonly_stats &st;
    size_t dev_rr = 0;
    std::vector<std::pair<u128, u128>> pend;
};

// Build the pending ranges' descriptors and launch them on the next device.
int flush_ranges(HostMsd &h) {
    if (h.pend.empty()) return NICE_OK;
    const NiceField &f = h.f;
    const size_t di = h.dev_rr++ % h.ctx->devs.size();
    Device &d = h.ctx->devs[di];
    Slot &sl = d.slot[h.t];
    h.job.used[di] = 1;
    HIPCHK(hipSetDevice(d.id));
    LeafBuf &b = d.desc[d.desc_next];
    d.desc_next ^= 1;
    // One leaf per range, more for ranges holding over kLeafPiece
    // candidates (the kernel sums 8 leaves' counts in 32 bits).
    constexpr u128 kPiece = nice::kLeafPiece;
    size_t need = 0;
    for (auto &pr : h.pend) {
        const u128 c = f.table->index_of(pr.second) - f.table->index_of(pr.first);
        need += (size_t)((c + kPiece - 1) / kPiece);
    }
    int r = ensure_desc(b, (uint32_t)std::max<size_t>(need, 1));
    if (r) return r;
    if (b.pending) HIPCHK(hipEventSynchronize(b.done));
    uint32_t nr = 0;
    uint64_t total = 0;
    for (auto &pr : h.pend) {
        const u128 i0 = f.table->index_of(pr.first), i1 = f.table->index_of(pr.second);
        h.st.ranges++;
        h.st.range_numbers += (uint64_t)(pr.second - pr.first);
        for (u128 g = i0; g < i1; g += kPiece) {
            // candidate g of the global residue sequence: (g / R) * M + res[g % R]
            const u128 cyc = g / f.R;
            const u128 bs = cyc * f.M;
            const uint32_t cnt = (uint32_t)std::min<u128>(kPiece, i1 - g);
            b.h[nr++] = nice::Leaf{lo64(bs), hi64(bs), (uint32_t)(g - cyc * f.R), cnt};
            total += cnt;
        }
    }
    h.pend.clear();
    if (!nr) return NICE_OK;
    h.st.candidates += total;
    HIPCHK(hipMemcpyAsync(b.d, b.h, (size_t)nr * sizeof(nice::Leaf), hipMemcpyHostToDevice, sl.nstream));
    nice::NiceonlyLaunch p = candidate_launch(f, d, sl);
    p.leaves = b.d;
    p.n_leaves_dev = nullptr;
    p.n_leaves = nr;
    hipError_t err = nice::launch_niceonly(p, d.num_cus, sl.nstream);
    if (err != hipSuccess) return fail(NICE_ERR_HIP, std::string("niceonly launch: ") + hipGetErrorString(err));
    HIPCHK(hipEventRecord(b.done, sl.nstream));
    b.pending = true;
    h.st.launches++;
    return NICE_OK;
}

// Host MSD: worker threads run the MSD filter per chunk and hand the
// surviving ranges to this thread in chunk batches; this thread builds
// descriptors and launches the candidate kernel on the devices round-robin.
int run_host_msd(nice_ctx *ctx, int t, NiceJob &job, const NiceField &f, nice_niceonly_stats &st,
                 std::chrono::steady_clock::time_point t0) {
    for (auto &d : ctx->devs) {
        Slot &sl = d.slot[t];
        HIPCHK(hipSetDevice(d.id));
        // the adaptive floor's GPU-tail clock starts with the field (the
        // stream reaches this event as soon as it is idle)
        if (job.adapt) HIPCHK(hipEventRecord(sl.nt0, sl.nstream));
        HIPCHK(hipMemsetAsync(sl.d_nice_count, 0, 4, sl.nstream));
        sl.msd.dirty = true;  // the nice count is left set
    }
    std::atomic<uint64_t> next{0};
    std::mutex qmu;
    std::condition_variable qcv;
    std::deque<std::vector<std::pair<u128, u128>>> queue;
    const int n_workers = (int)std::min<uint64_t>(f.threads, f.mine);
    st.msd_threads = (uint32_t)n_workers;
    int live = n_workers;  // guarded by qmu
    std::vector<std::thread> workers;
    std::unique_ptr<nice::MsdRunner> filt = nice::make_msd(f.base);
    for (int w = 0; w < n_workers; w++) {
        workers.emplace_back([&]() {
            std::vector<std::pair<u128, u128>> local;
            for (;;) {
                uint64_t i = next.fetch_add(1);
                if (i >= f.mine) break;
                u128 cs, ce;
                f.chunk_range(i, cs, ce);
                filt->ranges(cs, ce, f.floor, local, f.sound);
                if (local.size() >= 4096) {
                    std::lock_guard<std::mutex> g(qmu);
                    queue.push_back(std::move(local));
                    local = {};
                    qcv.notify_one();
                }
            }
            std::lock_guard<std::mutex> g(qmu);
            if (!local.empty()) queue.push_back(std::move(local));
            live--;
            qcv.notify_one();
        });
    }
    HostMsd h{ctx, t, job, f, st};
    int rc = NICE_OK;
    for (;;) {
        std::vector<std::pair<u128, u128>> item;
        {
            std::unique_lock<std::mutex> g(qmu);
            qcv.wait(g, [&] { return !queue.empty() || live == 0; });
            if (queue.empty() && live == 0) break;
            item = std::move(queue.front());
            queue.pop_front();
        }
        if (rc) continue;  // drain the producers after a failure
        h.pend.insert(h.pend.end(), item.begin(), item.end());
        if (h.pend.size() >= kBatchRanges) rc = flush_ranges(h);
    }
    for (auto &w : workers) w.join();
    st.msd_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!rc) rc = flush_ranges(h);
    // End of the field on every device: its list count, then a marker.
    for (size_t i = 0; i < ctx->devs.size() && !rc; i++) {
        Device &d = ctx->devs[i];
        Slot &sl = d.slot[t];
        job.used[i] = 1;
        HIPCHK(hipSetDevice(d.id));
        HIPCHK(hipMemcpyAsync(sl.h_nice, sl.d_nice_count, 4, hipMemcpyDeviceToHost, sl.nstream));
        HIPCHK(hipEventRecord(sl.nice_done, sl.nstream));
        if (job.adapt) HIPCHK(hipEventRecord(sl.nt1, sl.nstream));
    }
    return rc;
}

// Enqueue niceonly field `job` (bounds, base, options and floor already set)
// into slot t of the context's devices.  Called under ctx->mu by submit, and
// again by collect when a device's nice list overflowed and was grown: the
// whole field re-runs (the reference CPU path returns a list of any length,
// client_process.rs:439-465; its GPU path bails at 2^16,
// client_process_gpu.rs:777-782).
int niceonly_enqueue(nice_ctx *ctx, int t, NiceJob &job) {
    const auto t0 = std::chrono::steady_clock::now();
    NiceField f;
    if (int rc = resolve_field(job, f)) return rc;
    nice_niceonly_stats st{};
    st.msd_floor = f.floor;
    job.used.assign(ctx->devs.size(), 0);
    job.all.clear();
    job.empty = f.empty;
    job.collected = false;
    job.rejected = 0;
    job.st = st;
    if (f.empty) return NICE_OK;
    for (auto &d : ctx->devs)
        if (int rc = upload_tables(d, f)) return rc;

    const int where = job.has_opts ? job.opts.msd_where : NICE_MSD_AUTO;
    if (where < NICE_MSD_AUTO || where > NICE_MSD_DEVICE) return fail(NICE_ERR_INVALID, "bad msd_where");
    job.on_device = where == NICE_MSD_DEVICE || (where == NICE_MSD_AUTO && f.k == 2 && !((f.e - f.s) >> 63) &&
                                                 f.chunk <= ((u128)1 << 40));
    // the floor balances the host MSD producer against the GPU
    job.adapt = job.has_opts && job.opts.msd_floor == NICE_MSD_FLOOR_ADAPTIVE && !job.on_device;
    const int rc = job.on_device ? run_device_msd(ctx, t, job, f, st) : run_host_msd(ctx, t, job, f, st, t0);
    if (rc) return rc;
    job.st = st;
    return NICE_OK;
}

// Read a finished niceonly field's results from the devices (its events have
// completed).  counts receives every device's list length; *over is set when
// one exceeded its device's list capacity (that device's list was not read).
int niceonly_gather(nice_ctx *ctx, NiceJob &job, int t, std::vector<uint32_t> &counts, bool *over_out) {
    counts.assign(ctx->devs.size(), 0);
    bool over = false;
    *over_out = false;
    for (size_t i = 0; i < ctx->devs.size(); i++) {
        Device &d = ctx->devs[i];
        Slot &sl = d.slot[t];
        if (!job.used[i]) continue;  // no batch of this field ran there
        HIPCHK(hipSetDevice(d.id));
        HIPCHK(hipEventSynchronize(sl.nice_done));
        if (job.on_device) {
            const uint32_t *c = sl.h_msd;
            sl.msd.dirty = false;  // the epilogue re-zeroed counters and count
            if (nice::probe_set("NICE_MSD_TRACE")) {  // level sizes of the last batch (diagnostics)
                fprintf(stderr, "msd levels:");
                for (uint32_t lv = 0; lv < nice::kMsdLevels; lv++) fprintf(stderr, " %u", c[lv]);
                fprintf(stderr, " | ranges %u\n", c[nice::kMsdRanges]);
            }
            if (c[nice::kMsdOverflow])
                return fail(NICE_ERR_MSD_OVERFLOW, "device MSD queue overflow (msd_floor too small "
                                               "for chunk_size); use msd_where = host");
            uint64_t cand, nums;
            std::memcpy(&cand, c + nice::kMsdCandidates, 8);
            std::memcpy(&nums, c + nice::kMsdNumbers, 8);
            job.st.ranges += c[nice::kMsdRanges];
            job.st.candidates += cand;
            job.st.range_numbers += nums;
            job.st.square_ok += c[nice::kMsdSquareOk];
            if (job.has_opts && job.opts.filter == NICE_FILTER_SOUND) {
                uint64_t rj;
                std::memcpy(&rj, c + nice::kMsdMappedRejected, 8);
                job.rejected += rj;
            }
        }
        const uint32_t cnt = *sl.h_nice;
        counts[i] = cnt;
        if (cnt > sl.nice.cap) {
            // more nice numbers than the device list holds (the kernels count
            // every hit, store those below the capacity): grow and re-run
            over = true;
            *over_out = true;
            continue;
        }
        if (cnt && !over) {
            std::vector<uint64_t> nbuf((size_t)cnt * 2);
            HIPCHK(hipMemcpy(nbuf.data(), sl.nice.n, (size_t)cnt * 16, hipMemcpyDeviceToHost));
            for (uint32_t q = 0; q < cnt; q++) job.all.push_back({mk(nbuf[2 * q], nbuf[2 * q + 1]), job.base});
        }
    }
    return NICE_OK;
}

int niceonly_submit_args(nice_ctx *ctx, uint64_t start_lo, uint64_t start_hi, uint64_t end_lo, uint64_t end_hi,
                         uint32_t base, const nice_niceonly_opts *opts, bool wait, int *ticket) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!ctx || !ticket) return fail(NICE_ERR_INVALID, "null argument");
    if (base < 3 || base > 128) return fail(NICE_ERR_INVALID, "base must be in 3..=128");
    const u128 s = mk(start_lo, start_hi), e = mk(end_lo, end_hi);
    if (s >= e)
        return fail(NICE_ERR_INVALID, "Range has invalid bounds, range_start must be < range_end");
    if (opts && opts->deal_offset >= (opts->deal_stride ? opts->deal_stride : 1u))
        return fail(NICE_ERR_INVALID, "deal_offset must be < deal_stride");
    if (opts && opts->filter > NICE_FILTER_SOUND)
        return fail(NICE_ERR_INVALID, "filter must be NICE_FILTER_REFERENCE or NICE_FILTER_SOUND");
    const uint64_t floor_size = resolve_floor(opts);
    std::unique_lock<std::mutex> lock(ctx->mu);
    int t = -1;
    if (int rc = acquire_slot(ctx, lock, ctx->nice, ctx->nice_next, wait, "niceonly", &t)) return rc;
    NiceJob &job = ctx->nice[t];
    job = NiceJob{};
    job.owner = std::this_thread::get_id();
    job.s = s;
    job.e = e;
    job.base = base;
    job.has_opts = opts != nullptr;
    if (opts) job.opts = *opts;
    job.st.msd_floor = floor_size;
    job.nice_min = g_nice_min_override[base].load(std::memory_order_relaxed);
    job.t0 = t0;
    const int rc = niceonly_enqueue(ctx, t, job);
    if (rc) return rc;
    job.active = true;
    ctx->nice_next = (t + 1) % slots_used();
    *ticket = t;
    return NICE_OK;
}

// Wait for the field's devices WITHOUT the context lock, so other threads can
// submit and collect other fields meanwhile (the slot stays reserved: the job
// is active).
int niceonly_wait(nice_ctx *ctx, std::unique_lock<std::mutex> &lock, NiceJob &job, int t) {
    int rc = NICE_OK;
    job.waiting = true;
    lock.unlock();
    for (size_t i = 0; i < ctx->devs.size() && !rc; i++) {
        if (!job.used[i]) continue;
        Slot &sl = ctx->devs[i].slot[t];
        hipError_t err = hipSetDevice(ctx->devs[i].id);
        if (err == hipSuccess) err = sync_event(sl.nice_done);
        if (err != hipSuccess) rc = fail(NICE_ERR_HIP, std::string("niceonly field: ") + hipGetErrorString(err));
    }
    lock.lock();
    job.waiting = false;
    return rc;
}

// update_msd_floor (client_process_gpu.rs:551, 563-568, 130-157) for a
// collected host-MSD field.  The GPU tail ends when the field's last device
// work does (its end event), not when the caller gets round to collecting: the
// reference times both phases inside one call (:541-551).
void niceonly_adapt(nice_ctx *ctx, const NiceJob &job, int t) {
    double gpu_end = 0;
    for (size_t i = 0; i < ctx->devs.size(); i++) {
        if (!job.used[i]) continue;
        Slot &sl = ctx->devs[i].slot[t];
        float ms = 0;
        if (hipSetDevice(ctx->devs[i].id) == hipSuccess && hipEventElapsedTime(&ms, sl.nt0, sl.nt1) == hipSuccess)
            gpu_end = std::max(gpu_end, ms * 1e-3);
    }
    adapt_floor(job.st.msd_seconds, std::max(job.st.msd_seconds, gpu_end));
}

int niceonly_collect_locked(nice_ctx *ctx, int t, nice_number *out, size_t cap, size_t *n_out,
                            nice_niceonly_stats *stats) {
    std::unique_lock<std::mutex> lock(ctx->mu);
    if (t < 0 || t >= kSlots || !ctx->nice[t].active)
        return fail(NICE_ERR_INVALID, "no niceonly field in flight under this ticket");
    NiceJob &job = ctx->nice[t];
    if (job.waiting) return fail(NICE_ERR_INVALID, "another thread is collecting this niceonly field");
    if (!job.collected) {
        int rc = job.empty ? NICE_OK : niceonly_wait(ctx, lock, job, t);
        std::vector<uint32_t> counts;
        bool over = false;
        if (!rc && !job.empty) rc = niceonly_gather(ctx, job, t, counts, &over);
        for (uint32_t attempt = 0; !rc && !job.empty && over; attempt++) {
            if (attempt) {
                rc = fail(NICE_ERR_HIP, "niceonly list overflowed again after growing it to the field's count");
                break;
            }
            // Grow EVERY device's list to the whole field's count and re-run
            // the field (under the lock: rare).  The host MSD producer hands
            // batches to devices in the order its threads finish chunks (and
            // the re-run clears job.used), so a re-run can put the hits on a
            // device the first run never used; no device can hold more than
            // the field's total.
            uint64_t total = 0;
            for (uint32_t c : counts) total += c;
            if (total > 0xfffff000ull) {
                rc = fail(NICE_ERR_HIP, "niceonly list longer than 2^32 entries");
                break;
            }
            for (size_t i = 0; i < ctx->devs.size() && !rc; i++)
                rc = ensure_listbuf(ctx->devs[i], ctx->devs[i].slot[t].nice, ((uint32_t)total + 4095u) & ~4095u,
                                    false);
            if (!rc) rc = niceonly_enqueue(ctx, t, job);
            if (!rc) job.reruns++;
            if (!rc) rc = niceonly_gather(ctx, job, t, counts, &over);
        }
        if (rc) {
            job.active = false;
            return rc;
        }
        job.st.total_seconds =
            std::chrono::duration<double>(std::chrono::steady_clock::now() - job.t0).count();
        job.st.reruns = job.reruns;
        job.collected = true;
        // A re-run field's MSD time covers its last run only while its total
        // spans every run: the two do not balance, so it does not move the floor.
        if (job.adapt && job.reruns == 0) niceonly_adapt(ctx, job, t);
    }
    if (stats) *stats = job.st;
    t_prefix_rejected = job.rejected;
    const int rc = emit_list(job.all, out, cap, n_out);
    if (rc == NICE_ERR_CAPACITY) return rc;  // kept: the caller retries with room
    job.active = false;
    job.all = {};
    return rc;
}

}  // namespace

extern "C" {

int nice_niceonly_submit(nice_ctx *ctx, uint64_t start_lo, uint64_t start_hi, uint64_t end_lo,
                         uint64_t end_hi, uint32_t base, const nice_niceonly_opts *opts, int *ticket) {
    return niceonly_submit_args(ctx, start_lo, start_hi, end_lo, end_hi, base, opts, false, ticket);
}

uint64_t nice_niceonly_prefix_rejected(void) { return t_prefix_rejected; }

int nice_niceonly_collect(nice_ctx *ctx, int t, nice_number *out, size_t cap, size_t *n_out,
                          nice_niceonly_stats *stats) {
    if (!ctx) return fail(NICE_ERR_INVALID, "null ctx");
    const int rc = niceonly_collect_locked(ctx, t, out, cap, n_out, stats);
    ctx->freed.notify_all();  // the ticket's slot may be free now
    return rc;
}

int nice_process_range_niceonly_ex(nice_ctx *ctx, uint64_t start_lo, uint64_t start_hi,
                                   uint64_t end_lo, uint64_t end_hi, uint32_t base,
                                   const nice_niceonly_opts *opts, nice_number *out, size_t cap,
                                   size_t *n_out, nice_niceonly_stats *stats) {
    int t = -1;
    int rc = niceonly_submit_args(ctx, start_lo, start_hi, end_lo, end_hi, base, opts, true, &t);
    if (rc) return rc;
    rc = nice_niceonly_collect(ctx, t, out, cap, n_out, stats);
    if (rc == NICE_ERR_CAPACITY) {
        {
            std::lock_guard<std::mutex> lock(ctx->mu);
            ctx->nice[t].active = false;
            ctx->nice[t].all = {};
        }
        ctx->freed.notify_all();
    }
    return rc;
}

int nice_process_range_niceonly(nice_ctx *ctx, uint64_t start_lo, uint64_t start_hi,
                                uint64_t end_lo, uint64_t end_hi, uint32_t base, nice_number *out,
                                size_t cap, size_t *n_out) {
    return nice_process_range_niceonly_ex(ctx, start_lo, start_hi, end_lo, end_hi, base, nullptr,
                                          out, cap, n_out, nullptr);
}

}  // extern "C"
