"""Niceonly wall time per field of the new fast bases under several builds of
the library, interleaved on one box.

    python scripts/niceonly_bases_ab.py --out FILE.jsonl [--rounds 5] LABEL=DIR ...

DIR holds a `nice_amd` package with its built library: '.' is this tree,
ab_parent/ a checkout of the parent commit built there, ab_waves3/ this
tree's package built with CXXFLAGS += -DNICE_WIDE_WAVES=3 (the wave kernel of
b57..64 at three waves per SIMD, no scratch).  A process loads one library,
so every (round, build) is a fresh child process; the rounds go build by
build, so the builds' repeats interleave.  A child runs every field once
untimed and once timed: device MSD, floor 250, the client chunk rule (1e11 ->
1e6 chunks, the fused per-chunk MSD + niceonly_kernel; 1e13 -> 1e8 chunks, the
level BFS + msd_wave_kernel), window start s + K (e - s) // 256.

One JSON line per (round, build, base, size) goes to FILE; the table at the
end has per build the median and the min-max over the rounds, and each
build's median over the first build's.  Any child that fails or overruns its
time limit ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = {45: 2, 57: 31, 58: 7, 60: 8, 65: 21}
SIZES = (10 ** 11, 10 ** 13)


def child(d):
    sys.path.insert(0, ROOT if d == "." else os.path.join(ROOT, d))
    import nice_amd as N
    ctx = N.GpuContext(0)
    try:
        for base, k in K.items():
            r = N.get_base_range_u128(base)
            a = r.range_start + k * (r.range_end - r.range_start) // 256
            for size in SIZES:
                ctx.niceonly_raw(a, a + size, base, msd_where="device")
                t = time.perf_counter()
                lst, st = ctx.niceonly_raw(a, a + size, base, msd_where="device")
                dt = time.perf_counter() - t
                print(json.dumps({"base": base, "size": size, "seconds": dt, "candidates": st.candidates,
                                  "ranges": st.ranges, "square_ok": st.square_ok, "nice": len(lst),
                                  "launches": st.launches}), flush=True)
    finally:
        ctx.close()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--child")
    p.add_argument("--out")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--limit", type=float, default=120.0, help="seconds per child process")
    p.add_argument("builds", nargs="*")
    a = p.parse_args()
    if a.child:
        return child(a.child)
    builds = [b.split("=", 1) for b in a.builds]
    rows = []
    with open(a.out, "w") as out:
        for rnd in range(a.rounds):
            for label, d in builds:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", d], cwd=ROOT,
                                   capture_output=True, text=True, timeout=a.limit)
                if r.returncode != 0:
                    sys.exit(f"{label} round {rnd}: exit {r.returncode}\n{r.stderr[-2000:]}")
                for line in r.stdout.splitlines():
                    row = dict(json.loads(line), build=label, round=rnd)
                    rows.append(row)
                    out.write(json.dumps(row) + "\n")
                    out.flush()
    first = builds[0][0]
    print(f"{'base':>4} {'size':>6} {'build':>10} {'median s':>10} {'min':>10} {'max':>10} {'/' + first:>8}  counts")
    for base in K:
        for size in SIZES:
            med = {}
            for label, _ in builds:
                sel = [r for r in rows if (r["base"], r["size"], r["build"]) == (base, size, label)]
                t = [r["seconds"] for r in sel]
                med[label] = statistics.median(t)
                counts = {(r["candidates"], r["ranges"], r["square_ok"], r["nice"]) for r in sel}
                print(f"{base:>4} {size:>6.0e} {label:>10} {med[label]:>10.5f} {min(t):>10.5f} {max(t):>10.5f} "
                      f"{med[label] / med[first]:>8.3f}  {sorted(counts)}")


if __name__ == "__main__":
    main()
