// abi_map.cpp -- the per-number unique-count map (nice_unique_map): one byte
// per n of a range, written by the FD map kernel where the base has one and
// the range lies inside its valid range, by the generic per-n kernel
// elsewhere (the plan: fd2_map_plan.hpp), into host memory -- sharded over the
// context's devices -- or in place into a caller's device buffer.
#include "abi_internal.hpp"
#include "unique_map.h"

using namespace nice::abi;
using nice::u128;

namespace {

// What the GPU call, its plan hook and (but for the context) the CPU twin
// refuse; `size` out.
int map_check_args(uint32_t base, u128 s, u128 e, const void *out, u128 &size) {
    if (!out) return fail(NICE_ERR_INVALID, "null out");
    if (base < 2 || base > 128) return fail(NICE_ERR_INVALID, "base must be in 2..=128");
    if (s >= e) return fail(NICE_ERR_INVALID, "range is empty or inverted");
    size = e - s;
    if (size > nice::kMapMaxNumbers) return fail(NICE_ERR_INVALID, "more than 2^32 numbers: map the range in pieces");
    return NICE_OK;
}

// Enqueue the map of [s, e) on device d (async on its map stream): the plan's
// launches write out[off0 ...), device memory of d.
int map_enqueue(Device &d, MapDev &r, uint32_t base, const nice::MapBase &mb, u128 s, u128 e, uint8_t *out,
                nice_map_stats &st, uint32_t *launches) {
    HIPCHK(hipSetDevice(d.id));
    nice::MapPlan pl;
    nice::map_plan(mb, s, e, 0, pl);
    size_t nu = 0;
    for (const nice::MapRec &q : pl.recs) nu += q.kind == nice::kMapFd;
    if (int rc = r.desc.ensure(nu, nice::kMapDescBytes, r.side.stream)) return rc;
    st.fd_segments += pl.fd_segments;
    st.generic_segments += pl.generic_segments;
    st.fd_numbers += pl.fd_numbers;
    st.generic_numbers += pl.generic_numbers;
    nice::MapLaunch p{};
    p.base = base;
    p.recs = pl.recs.data();
    p.n_recs = pl.recs.size();
    p.h_desc = r.desc.h;
    p.d_desc = r.desc.d;
    p.out = out;
    p.launches = launches;
    HIPCHK(hipEventRecord(r.side.ev0, r.side.stream));
    const hipError_t err = nice::launch_unique_map(p, r.side.stream);
    if (err != hipSuccess) return fail(NICE_ERR_HIP, std::string("map launch: ") + hipGetErrorString(err));
    HIPCHK(hipEventRecord(r.side.ev1, r.side.stream));
    return NICE_OK;
}

}  // namespace

void nice::abi::map_dev_free(Device &d, MapDev &r) {
    if (!r.side.stream) return;
    (void)r.side.drain(d);
    r.desc.free();
    if (r.d_out) (void)hipFree(r.d_out);
    r.side.destroy(d);
}

extern "C" {

int nice_debug_map_plan(uint32_t base, uint64_t start_lo, uint64_t start_hi, uint64_t end_lo, uint64_t end_hi,
                        uint64_t *records, size_t cap, size_t *n_out) {
    if (!n_out || (cap && !records)) return fail(NICE_ERR_INVALID, "null argument");
    u128 size = 0;
    if (int rc = map_check_args(base, mk(start_lo, start_hi), mk(end_lo, end_hi), n_out, size)) return rc;
    nice::MapPlan pl;
    nice::map_plan(nice::map_base(base), mk(start_lo, start_hi), mk(end_lo, end_hi), 0, pl);
    for (size_t i = 0; i < pl.recs.size() && i < cap; i++) {
        const nice::MapRec &q = pl.recs[i];
        uint64_t *o = records + 8 * i;
        o[0] = q.kind, o[1] = q.lo, o[2] = q.hi, o[3] = q.off, o[4] = q.lanes, o[5] = q.chunk, o[6] = q.combo,
        o[7] = q.count;
    }
    *n_out = pl.recs.size();
    return NICE_OK;
}

int nice_last_map_stats(nice_ctx *ctx, nice_map_stats *out) {
    if (!ctx || !out) return fail(NICE_ERR_INVALID, "bad args");
    std::lock_guard<std::mutex> lock(ctx->map_mu);
    *out = ctx->map.stats;
    return NICE_OK;
}

int nice_unique_map(nice_ctx *ctx, uint64_t start_lo, uint64_t start_hi, uint64_t end_lo, uint64_t end_hi,
                    uint32_t base, uint8_t *out, size_t cap, uint32_t flags, int device_index) {
    if (!ctx) return fail(NICE_ERR_INVALID, "null context");
    const u128 s = mk(start_lo, start_hi), e = mk(end_lo, end_hi);
    u128 size = 0;
    if (int rc = map_check_args(base, s, e, out, size)) return rc;
    if (flags > NICE_MAP_DEVICE) return fail(NICE_ERR_INVALID, "bad flags");
    const size_t nd = ctx->devs.size();
    const bool in_place = flags == NICE_MAP_DEVICE;
    if (in_place && (device_index < 0 || (size_t)device_index >= nd))
        return fail(NICE_ERR_INVALID, "device_index is not a device of the context");
    if ((u128)cap < size)
        return fail(NICE_ERR_CAPACITY, "the map needs " + std::to_string((uint64_t)size) + " bytes, capacity " +
                                           std::to_string(cap));
    std::lock_guard<std::mutex> lock(ctx->map_mu);
    MapState &st = ctx->map;
    st.dev.resize(nd);
    st.stats = nice_map_stats{};
    const nice::MapBase mb = nice::map_base(base);
    // the shards: device mode one, the whole range on its device; host mode
    // contiguous and equal over the devices
    struct Shard {
        size_t dv;
        u128 s, e;
    };
    std::vector<Shard> shards;
    if (in_place) {
        shards.push_back({(size_t)device_index, s, e});
    } else {
        for (size_t i = 0; i < nd; i++) {
            const u128 a = s + size * i / nd, b = s + size * (i + 1) / nd;
            if (a < b) shards.push_back({i, a, b});
        }
    }
    std::vector<uint32_t> launches(shards.size(), 0);
    int rc = NICE_OK;
    size_t enq = 0;
    for (; enq < shards.size() && !rc; enq++) {
        const Shard &h = shards[enq];
        Device &d = ctx->devs[h.dv];
        MapDev &r = st.dev[h.dv];
        rc = r.side.init(d);
        uint8_t *dst = out;
        if (!rc && !in_place) {
            const size_t need = (size_t)(h.e - h.s);
            if (r.out_cap < need) {
                (void)hipSetDevice(d.id);
                rc = grow_device(r.d_out, r.out_cap, need, need, r.side.stream);
            }
            dst = r.d_out;
        }
        if (!rc) rc = map_enqueue(d, r, base, mb, h.s, h.e, dst, st.stats, &launches[enq]);
        if (!rc && !in_place) {
            const hipError_t err = hipMemcpyAsync(out + (size_t)(h.s - s), r.d_out, (size_t)(h.e - h.s),
                                                  hipMemcpyDeviceToHost, r.side.stream);
            if (err != hipSuccess) rc = fail(NICE_ERR_HIP, std::string("map copy: ") + hipGetErrorString(err));
        }
    }
    // wait for everything enqueued, also after an error
    for (size_t i = 0; i < enq; i++) {
        MapDev &r = st.dev[shards[i].dv];
        if (!r.side.stream) continue;
        const hipError_t err = r.side.drain(ctx->devs[shards[i].dv]);
        if (err != hipSuccess && !rc) rc = fail(NICE_ERR_HIP, std::string("map: ") + hipGetErrorString(err));
        if (rc) continue;
        float t = 0;
        if (r.side.elapsed(&t) == hipSuccess) st.stats.kernel_ms = std::max(st.stats.kernel_ms, (double)t);
        st.stats.launches += launches[i];
    }
    return rc;
}

}  // extern "C"
