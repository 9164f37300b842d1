"""Kernel A/B of the batched niceonly ranges against niceonly_kernel on the
same leaves: the client's 1000 chunks of a 1e9 field through
nice_msd_valid_ranges at floor 250 give the ranges; side "ranges" hands them
to ONE niceonly_ranges call (niceonly_ranges_kernel), side "field" runs the
field with msd_where="host", whose host MSD producer builds the same leaves
for niceonly_kernel.  One side per process, to be run under

    rocprofv3 --kernel-trace --output-format csv -d DIR -- \\
        python scripts/ranges_niceonly_ab.py run --side ranges --base 40

(the field side also from a checkout of the parent commit: it uses nothing
newer), and then

    python scripts/ranges_niceonly_ab.py report DIR... > profiles/ranges_niceonly/kernel_ab.txt

which reads every kernel trace below the directories and prints, per kernel
and directory, the median and spread of the dispatch times after the warm-up.
"""
import argparse
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARMUP = 5
KERNELS = ("niceonly_ranges_kernel", "niceonly_kernel")


def field_of(base):
    import nice_amd as N
    if base == 40:
        f = N.get_benchmark_field(N.BenchmarkMode.EXTRA_LARGE)
        return f.range_start, f.range_end
    # (b80: most of the range has no MSD survivor; 2e9 past 0.9 of it lies the densest
    # stretch tests/nice_min_windows.py found: 24 087 ranges, 247 964 candidates)
    r = N.get_base_range_u128(base)
    a = r.range_start + int((r.range_end - r.range_start) * 0.9) + 2 * 10 ** 9
    return a, a + 10 ** 9


def run(args):
    import nice_amd as N
    from nice_amd import api
    from nice_amd.dist import client_chunk_size
    a, e = field_of(args.base)
    ctx = N.GpuContext(0)
    if args.side == "ranges":
        chunk = client_chunk_size(e - a)
        ranges = [(r.range_start, r.range_end) for s in range(a, e, chunk)
                  for r in api.get_valid_ranges(N.FieldSize(s, min(e, s + chunk)), args.base, 250)]
        for _ in range(WARMUP + args.reps):
            cand, sq, lst = ctx.niceonly_ranges(ranges, args.base)
        st = ctx.ranges_niceonly_stats()
        print(f"ranges b{args.base}: {len(ranges)} ranges, {sum(cand)} candidates, {sum(sq)} square_ok, "
              f"{st.launches} launch(es), list {len(lst)}")
    else:
        for _ in range(WARMUP + args.reps):
            lst, st = ctx.niceonly_raw(a, e, args.base, msd_where="host", threads=16)
        print(f"field b{args.base}: {st.ranges} ranges, {st.candidates} candidates, {st.launches} launch(es), "
              f"list {len(lst)}")
    ctx.close()


def report(dirs):
    for d in dirs:
        rows = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as fh:
                for r in csv.DictReader(fh):
                    name = next((k for k in KERNELS if k + "<" in r["Kernel_Name"] or
                                 r["Kernel_Name"].startswith(k)), None)
                    if name:
                        rows.setdefault(name, []).append((int(r["Start_Timestamp"]),
                                                          int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
        for name, v in sorted(rows.items()):
            us = [dur / 1e3 for _, dur in sorted(v)][WARMUP:]
            if not us:
                continue
            print(f"{d:40s} {name:24s} {len(us):4d} dispatches  median {statistics.median(us):9.2f} us  "
                  f"min {min(us):9.2f}  max {max(us):9.2f}  p10 {sorted(us)[len(us) // 10]:9.2f}  "
                  f"p90 {sorted(us)[len(us) * 9 // 10]:9.2f}")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--side", choices=["ranges", "field"], required=True)
    r.add_argument("--base", type=int, default=40)
    r.add_argument("--reps", type=int, default=60)
    p = sub.add_parser("report")
    p.add_argument("dirs", nargs="+")
    args = ap.parse_args()
    if args.cmd == "run":
        run(args)
    else:
        report(args.dirs)


if __name__ == "__main__":
    main()
