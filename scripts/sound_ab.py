"""Niceonly wall time per field under the reference filter, the sound filter,
and the sound filter with its per-candidate prefix test off, interleaved in
one process.

    NICE_LIB_PATH=nice_amd/libnice_hip_probe.so python scripts/sound_ab.py --out FILE.jsonl [--rounds 5]

Fields, all device MSD: the b40 1e9 extra-large field (client chunk 1e6: the
fused per-chunk MSD + niceonly_kernel), the msd-effective field (b50 1e12,
chunk 1e7: level BFS + msd_wave_kernel) and the whole massive field (b50 1e13,
chunk 1e8).  Every mode runs at floors 250 and 64; sound also sweeps the floor
on the massive field (--sweep), since the best floor moves with the filter.

"sound-noprefix" needs the probe build (make -C nice_amd probe): its
NICE_SOUND_NOPREFIX switch, read at every submit, leaves the prefix test off
while the same compile-time kernels run.  With the product library that mode
is skipped.

Each (field, floor, mode) runs once untimed, then --rounds timed rounds go
mode by mode, so the modes' repeats interleave.  One JSON line per timed run
goes to FILE; the table at the end has the median and the min-max over the
rounds, the counts, and the nice list."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import nice_amd as N  # noqa: E402
from nice_amd.benchmark import BenchmarkMode as BM, get_benchmark_field  # noqa: E402

MODES = ("reference", "sound", "sound-noprefix")


def run(ctx, f, chunk, floor, mode):
    if mode == "sound-noprefix":
        os.environ["NICE_SOUND_NOPREFIX"] = "1"
    else:
        os.environ.pop("NICE_SOUND_NOPREFIX", None)
    t = time.perf_counter()
    lst, st = ctx.niceonly_raw(f.range_start, f.range_end, f.base, chunk_size=chunk, msd_floor=floor,
                               msd_where="device", filter="reference" if mode == "reference" else "sound")
    dt = time.perf_counter() - t
    os.environ.pop("NICE_SOUND_NOPREFIX", None)
    return {"seconds": dt, "ranges": st.ranges, "candidates": st.candidates, "square_ok": st.square_ok,
            "prefix_rejected": st.prefix_rejected, "nice": [str(x) for x in lst]}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", required=True)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--sweep", default="16,32,64,125,250,500,1000", help="sound floors on the massive field")
    p.add_argument("--fields", default="extra-large,msd-effective,massive")
    a = p.parse_args()
    probe = "probe" in os.path.basename(N._lib.LIB_PATH)
    modes = [m for m in MODES if probe or m != "sound-noprefix"]
    if not probe:
        print("product library: sound-noprefix skipped (needs NICE_LIB_PATH=.../libnice_hip_probe.so)")
    fields = {"extra-large": (get_benchmark_field(BM.EXTRA_LARGE), 0),
              "msd-effective": (get_benchmark_field(BM.MSD_EFFECTIVE), 0),
              "massive": (get_benchmark_field(BM.MASSIVE), 10 ** 8)}
    cases = []  # (field, floor, mode)
    for name in a.fields.split(","):
        for floor in (250, 64):
            cases += [(name, floor, m) for m in modes]
        if name == "massive":
            cases += [(name, int(fl), "sound") for fl in a.sweep.split(",") if int(fl) not in (250, 64)]
    ctx = N.GpuContext(0)
    rows = []
    try:
        for case in list(cases):  # warm-up: buffers, tables, clocks
            name, floor, mode = case
            try:
                run(ctx, *fields[name], floor, mode)
            except N.NiceError as e:  # e.g. the device MSD queues overflow at a low floor
                print(f"dropped {case}: {e}")
                cases.remove(case)
        with open(a.out, "w") as out:
            for rnd in range(a.rounds):
                for name, floor, mode in cases:
                    row = dict(run(ctx, *fields[name], floor, mode), field=name, floor=floor, mode=mode, round=rnd)
                    rows.append(row)
                    out.write(json.dumps(row) + "\n")
                    out.flush()
    finally:
        ctx.close()
    print(f"{'field':>14} {'floor':>5} {'mode':>15} {'median s':>9} {'min':>9} {'max':>9} {'/ref':>6} "
          f"{'ranges':>9} {'candidates':>11} {'rejected':>11} {'square_ok':>10}  nice")
    for name, floor, mode in cases:
        sel = [r for r in rows if (r["field"], r["floor"], r["mode"]) == (name, floor, mode)]
        ref = [r["seconds"] for r in rows if (r["field"], r["floor"], r["mode"]) == (name, floor, "reference")]
        t = [r["seconds"] for r in sel]
        counts = {(r["ranges"], r["candidates"], r["prefix_rejected"], r["square_ok"], tuple(r["nice"])) for r in sel}
        assert len(counts) == 1, counts
        c = sel[0]
        rel = f"{statistics.median(t) / statistics.median(ref):6.2f}" if ref else "      "
        print(f"{name:>14} {floor:>5} {mode:>15} {statistics.median(t):>9.5f} {min(t):>9.5f} {max(t):>9.5f} {rel} "
              f"{c['ranges']:>9} {c['candidates']:>11} {c['prefix_rejected']:>11} {c['square_ok']:>10}  {c['nice']}")


if __name__ == "__main__":
    main()
