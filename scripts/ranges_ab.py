"""A/B of the batched detailed ranges against the per-field paths, one GPU,
one process, kernel timing on, every shape warmed up first.  The same b40
ranges go through

  (a) a loop of detailed_submit / detailed_collect kept three deep (the best
      the per-field interface offers for many ranges),
  (b) ONE detailed_ranges call (per-range rows),
  (c) the contiguous field of the same size in one detailed_raw call,

alternated for --reps repetitions each, on two workloads: 1024 consecutive
ranges of 1e6 from the default benchmark start, and 4096 MSD-survivor-sized
ranges of 300.  Prints the median and the spread (min .. max) of the wall time
of each, the batch's kernel time, and (b)/(a), (b)/(c).

    python scripts/ranges_ab.py [--reps 20] [--out profiles/ranges/ranges_ab.txt]
"""
import argparse
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import nice_amd as N  # noqa: E402

BASE = 40


def path_a(ctx, ranges):
    """submit / collect, three fields in flight."""
    tickets, total = [], [0] * (BASE + 1)
    for a, b in ranges:
        if len(tickets) == 3:
            hist, _ = ctx.detailed_collect(tickets.pop(0), BASE)
            for i, v in enumerate(hist):
                total[i] += v
        tickets.append(ctx.detailed_submit(a, b, BASE))
    for t in tickets:
        hist, _ = ctx.detailed_collect(t, BASE)
        for i, v in enumerate(hist):
            total[i] += v
    return total


def path_b(ctx, ranges):
    rows, _ = ctx.detailed_ranges(ranges, BASE)
    return [sum(col) for col in zip(*rows)]


def path_c(ctx, field):
    return ctx.detailed_raw(*field, BASE)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = N.GpuContext(0)
    ctx.set_kernel_timing(True)
    f = N.get_benchmark_field(N.BenchmarkMode.DEFAULT)
    s0 = f.range_start
    big = [(s0 + 10 ** 6 * k, s0 + 10 ** 6 * (k + 1)) for k in range(1024)]
    r = N.get_base_range_u128(BASE)
    rng = random.Random(1)
    starts = sorted(rng.sample(range(r.range_start, r.range_end - 1000, 1000), 4096))
    small = [(a, a + 300) for a in starts]
    lines = []
    for name, ranges, field in (("1024 x 1e6", big, (s0, s0 + 1024 * 10 ** 6)),
                                ("4096 x 300", small, (s0, s0 + 4096 * 300))):
        numbers = sum(b - a for a, b in ranges)
        paths = {"a submit/collect x3": lambda: path_a(ctx, ranges),
                 "b detailed_ranges": lambda: path_b(ctx, ranges),
                 "c one field": lambda: path_c(ctx, field)}
        got = {k: fn() for k, fn in paths.items()}  # warm-up of every shape
        assert got["a submit/collect x3"] == got["b detailed_ranges"], "paths disagree"
        if field[1] - field[0] == numbers and ranges is big:
            assert got["c one field"] == got["b detailed_ranges"]
        times = {k: [] for k in paths}
        kern = []
        for _ in range(max(20, args.reps)):
            for k, fn in paths.items():  # alternated
                t0 = time.perf_counter()
                fn()
                times[k].append((time.perf_counter() - t0) * 1e3)
                if k.startswith("b"):
                    kern.append(ctx.ranges_stats().kernel_ms)
        st = ctx.ranges_stats()
        lines.append(f"workload {name} (b{BASE}, {numbers:.3e} numbers), {len(kern)} repetitions each, "
                     f"batch launches {st.launches}")
        med = {}
        for k, v in times.items():
            med[k] = statistics.median(v)
            lines.append(f"  ({k:22s}) wall median {med[k]:9.3f} ms  spread {min(v):9.3f} .. {max(v):9.3f} ms  "
                         f"{numbers / med[k] / 1e6:8.2f} e9 n/s")
        lines.append(f"  (b) kernel time by HIP events: median {statistics.median(kern):.3f} ms  "
                     f"spread {min(kern):.3f} .. {max(kern):.3f} ms")
        lines.append(f"  (b)/(a) = {med['b detailed_ranges'] / med['a submit/collect x3']:.3f}   "
                     f"(b)/(c) = {med['b detailed_ranges'] / med['c one field']:.3f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
