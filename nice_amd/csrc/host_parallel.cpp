// host_parallel.cpp -- how many host threads the MSD producer gets, and the
// MSD floor of a niceonly field: plain host code, no HIP.
#include "host_parallel.hpp"

#include <sched.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>

namespace {

// CPUs a cgroup v2 cpu.max line grants: quota / period rounded DOWN (Rust's
// cgroups::quota_v2), 0 for "max" or an unreadable line.
unsigned cpu_max_cpus(const char *text) {
    char q[32] = {0};
    unsigned long period = 0;
    if (!text || sscanf(text, "%31s %lu", q, &period) != 2 || strcmp(q, "max") == 0 || period == 0) return 0;
    char *end = nullptr;
    const unsigned long quota = strtoul(q, &end, 10);
    if (end == q) return 0;
    const unsigned long c = quota / period;
    return c > 0xffffffffUL ? 0xffffffffu : (unsigned)c;
}

// The tightest cpu.max of the cgroup `rel` (a path below `root`) and of its
// ancestors up to root, as Rust walks them; 0 if none limits.
unsigned cgroup_cpus(const std::string &root, std::string rel) {
    unsigned best = 0;
    bool limited = false;
    for (;;) {
        while (!rel.empty() && rel.back() == '/') rel.pop_back();
        if (FILE *f = fopen((root + rel + "/cpu.max").c_str(), "r")) {
            char line[128] = {0};
            if (fgets(line, sizeof line, f)) {
                char q[32] = {0};
                if (sscanf(line, "%31s", q) == 1 && strcmp(q, "max") != 0) {
                    const unsigned c = cpu_max_cpus(line);
                    best = limited ? std::min(best, c) : c;
                    limited = true;
                }
            }
            fclose(f);
        }
        if (rel.empty()) break;
        const size_t p = rel.rfind('/');
        rel = p == std::string::npos ? std::string() : rel.substr(0, p);
    }
    return limited ? std::max(best, 1u) : 0u;
}

// NICE_GPU_MSD_FLOOR pins the reference GPU path's MSD floor
// (client_process_gpu.rs:161-172: parsed as f64, used when >= 1, otherwise
// ignored with a warning).  Read once, like the reference's OnceLock.
uint64_t env_msd_floor() {
    static const uint64_t v = [] {
        const char *e = getenv("NICE_GPU_MSD_FLOOR");
        if (!e) return (uint64_t)0;
        char *end = nullptr;
        const double f = strtod(e, &end);
        if (end == e || *end != 0 || !(f >= 1.0) || f > 1e18) {
            fprintf(stderr, "nice: ignoring invalid NICE_GPU_MSD_FLOOR '%s'\n", e);
            return (uint64_t)0;
        }
        return (uint64_t)f;
    }();
    return v;
}

// The reference GPU path's AdaptiveFloor (client_process_gpu.rs:96-184),
// selected by msd_floor = NICE_MSD_FLOOR_ADAPTIVE.  Process-wide, like the
// reference's OnceLock: NICE_GPU_MSD_FLOOR pins it (no adaptation); otherwise
// the seed is 512 000 / logical cores clamped to [250, 256 000], the first 3
// fields do not adapt, and after each host-MSD field the floor moves by
// msd / gpu_tail, clamped to [1/1.5, 1.5] (nice_adaptive_floor_step).
constexpr double kFloorMin = 250.0, kFloorMax = 256000.0, kAdaptMaxStep = 1.5, kAdaptMinSecs = 0.002,
                 kAdaptBaseCoreProduct = 512000.0;
constexpr uint32_t kAdaptWarmup = 3, kAdaptPinned = 0xffffffffu;
struct AdaptiveFloor {
    double floor;
    uint32_t warmup;  // fields left before adapting; kAdaptPinned: fixed by the environment
};
std::mutex g_af_mu;

AdaptiveFloor &adaptive_floor() {  // call under g_af_mu
    static AdaptiveFloor af = [] {
        if (const uint64_t pin = env_msd_floor()) return AdaptiveFloor{(double)pin, kAdaptPinned};
        const double seed =
            std::min(kFloorMax, std::max(kFloorMin, kAdaptBaseCoreProduct / nice::abi::available_parallelism()));
        return AdaptiveFloor{seed, kAdaptWarmup};
    }();
    return af;
}

}  // namespace

namespace nice {
namespace abi {

// std::thread::available_parallelism on Linux (library/std/src/sys/pal/unix/
// thread.rs): the affinity mask, capped by the cgroup v2 cpu.max quotas of
// the process's own cgroup (/proc/self/cgroup "0::<path>") and its ancestors
// under /sys/fs/cgroup, each quota / period rounded down, at least 1.
unsigned available_parallelism() {
    unsigned n = std::thread::hardware_concurrency();
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0 && CPU_COUNT(&set) > 0) n = (unsigned)CPU_COUNT(&set);
    std::string rel;
    if (FILE *f = fopen("/proc/self/cgroup", "r")) {
        char line[4096];
        while (fgets(line, sizeof line, f))
            if (strncmp(line, "0::", 3) == 0) {
                rel = line + 3;
                while (!rel.empty() && (rel.back() == '\n' || rel.back() == '\r')) rel.pop_back();
                break;
            }
        fclose(f);
    }
    const unsigned c = cgroup_cpus("/sys/fs/cgroup", rel);
    if (c >= 1 && c < n) n = c;
    return n ? n : 4;
}

uint64_t resolve_floor(const nice_niceonly_opts *opts) {
    uint64_t floor_size = opts && opts->msd_floor ? opts->msd_floor : env_msd_floor();
    if (opts && opts->msd_floor == NICE_MSD_FLOOR_ADAPTIVE) {
        std::lock_guard<std::mutex> g(g_af_mu);
        floor_size = (uint64_t)adaptive_floor().floor;  // gpu_msd_floor(), client_process_gpu.rs:559-561
    }
    return floor_size ? floor_size : 250;
}

void adapt_floor(double msd_seconds, double total_seconds) {
    std::lock_guard<std::mutex> g(g_af_mu);
    AdaptiveFloor &af = adaptive_floor();
    if (af.warmup == kAdaptPinned) {
    } else if (af.warmup > 0) {
        af.warmup--;
    } else {
        af.floor = nice_adaptive_floor_step(af.floor, msd_seconds, total_seconds);
    }
}

}  // namespace abi
}  // namespace nice

extern "C" {

double nice_adaptive_floor_step(double floor, double msd_seconds, double total_seconds) {
    const double gpu_tail = std::max(0.0, total_seconds - msd_seconds);
    const double ratio = gpu_tail < kAdaptMinSecs ? kAdaptMaxStep
                         : msd_seconds < kAdaptMinSecs ? 1.0 / kAdaptMaxStep
                                                       : msd_seconds / gpu_tail;
    const double factor = std::min(kAdaptMaxStep, std::max(1.0 / kAdaptMaxStep, ratio));
    return std::min(kFloorMax, std::max(kFloorMin, floor * factor));
}

int nice_adaptive_floor(double *floor, uint32_t *warmup) {
    std::lock_guard<std::mutex> g(g_af_mu);
    const AdaptiveFloor &af = adaptive_floor();
    if (floor) *floor = af.floor;
    if (warmup) *warmup = af.warmup;
    return NICE_OK;
}

uint32_t nice_host_threads(void) { return nice::abi::available_parallelism(); }

uint32_t nice_debug_cgroup_cpus(const char *root, const char *cgroup_path) {
    return root ? cgroup_cpus(root, cgroup_path ? cgroup_path : "") : 0u;
}

}  // extern "C"
