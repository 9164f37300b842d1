"""On against off: the batched niceonly ranges call with the sound prefix test
(nice_process_ranges_niceonly_ex, NICE_RANGES_PREFIX_ON: range_mask_kernel +
the prefix-testing niceonly_ranges_kernel) against the same call with the test
off, which is the parent's kernel, on the same ranges in one process.

The ranges are the sound range list (ctx.msd_ranges, floor 250) of as many 1e8
chunk roots of the base as stay under 2^20 ranges (at most ROOTS_MAX roots).
The two sides alternate call by call; reported per base: the median, minimum
and maximum of kernel_ms (HIP events around the side's launches, the mask
launch included) over the calls after the warm-up, and of mask_ms.

    python scripts/ranges_prefix_ab.py [--bases 40 50 57 80] [--reps 11] > profiles/ranges_prefix/on_off_ab.txt
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARMUP = 3
CHUNK = 10 ** 8
RANGES_MAX = 1 << 20
ROOTS_MAX = 256


# Where the roots begin, in 256ths of the valid range: stretches with MSD
# survivors (large parts of a range have none), the sound tests' windows
# (tests/test_sound_filter.py K).
START_256 = {40: 2, 50: 3, 57: 31}


def first_root(N, base):
    """... and b80 at the dense stretch scripts/ranges_niceonly_ab.py uses."""
    r = N.get_base_range_u128(base)
    if base == 80:
        return r.range_start + int((r.range_end - r.range_start) * 0.9) + 2 * 10 ** 9
    return r.range_start + START_256.get(base, 64) * (r.range_end - r.range_start) // 256


def range_list(ctx, api, N, base):
    a = first_root(N, base)
    one, _ = ctx.msd_ranges(api.chunk_roots(a, a + CHUNK, CHUNK), base, 250, "sound")
    roots = max(1, min(ROOTS_MAX, RANGES_MAX // max(1, len(one))))
    while True:
        bounds, _ = ctx.msd_ranges(api.chunk_roots(a, a + roots * CHUNK, CHUNK), base, 250, "sound")
        if len(bounds) <= RANGES_MAX:
            return roots, bounds
        roots = roots * 9 // 10


def spread(v):
    return f"median {statistics.median(v):8.3f}  min {min(v):8.3f}  max {max(v):8.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, nargs="+", default=[40, 50, 57, 80])
    ap.add_argument("--reps", type=int, default=11)
    args = ap.parse_args()
    import nice_amd as N
    from nice_amd import api
    ctx = N.GpuContext(0)
    print(f"# kernel_ms per call, {args.reps} calls per side after {WARMUP} warm-up calls, the sides alternating")
    for base in args.bases:
        roots, bounds = range_list(ctx, api, N, base)
        if not len(bounds):
            print(f"b{base}: no MSD survivor in {roots} roots of 1e8 from {first_root(N, base)}")
            continue
        ms = {"off": [], "on": [], "mask": []}
        for i in range(WARMUP + args.reps):
            for side in ("off", "on"):
                cand, sq, rej, lst = ctx.niceonly_ranges_ex(bounds, base, prefix_test=side == "on")
                if side == "on":
                    kept = (sum(cand), sum(rej), sum(sq))
                else:
                    plain_sq = sum(sq)
                if i >= WARMUP:
                    ms[side].append(ctx.ranges_niceonly_stats().kernel_ms)
                    if side == "on":
                        ms["mask"].append(ctx.ranges_niceonly_prefix_stats().mask_ms)
        on, off = statistics.median(ms["on"]), statistics.median(ms["off"])
        print(f"b{base}: {roots} roots of 1e8, {len(bounds)} ranges, {kept[0]} candidates, {kept[1]} rejected "
              f"({100 * kept[1] / max(1, kept[0]):.1f} %), square_ok {kept[2]} on / {plain_sq} off, list {len(lst)}")
        print(f"  off      ms: {spread(ms['off'])}")
        print(f"  on       ms: {spread(ms['on'])}   (mask launch included)")
        print(f"  mask     ms: {spread(ms['mask'])}")
        print(f"  on / off = {on / off:.3f} ({'faster' if on < off else 'slower'})")
    ctx.close()


if __name__ == "__main__":
    main()
