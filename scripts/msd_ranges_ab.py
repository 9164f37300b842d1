"""The device MSD range list against its three baselines, one JSON line per
measurement (profiles/msd_ranges/):

    python scripts/msd_ranges_ab.py [--root TREE] SIDE...

  ranges         GpuContext.msd_ranges over the slice's chunk grid: wall time (a
                 host clock around the call, which ends in a synchronise),
                 kernel_ms and order_ms from the statistics, the rest -- the
                 copy back, the expansion to quadruples, the retry with room
                 after NICE_ERR_CAPACITY (the default cap), the Python buffers
                 -- as their difference
  field          the device-MSD niceonly field of the same slice (niceonly_raw,
                 msd_where="device"): msd_seconds and total_seconds
  cpu            api.msd_ranges_cpu on 16 threads over the same roots
  survey-host    survey_niceonly_base on the default 4096 windows, host MSD
  survey-device  ... with msd_where="device"

The slice is 1e12 numbers of the massive b50 field (tests/golden/massive_b50.json;
from its 1e11 window 66, where 1.6e7 ranges survive) at chunk 1e8 and floor 250.  --root: the tree whose package runs (a checkout of
the parent commit for `field` and `survey-host`).  Each side runs once to warm
up and then --reps times; every repetition is printed.
"""
import argparse
import json
import os
import sys
import time

p = argparse.ArgumentParser()
p.add_argument("sides", nargs="+", choices=["ranges", "field", "cpu", "survey-host", "survey-device"])
p.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
p.add_argument("--reps", type=int, default=3)
p.add_argument("--window", type=int, default=66, help="the slice starts at this 1e11 window of the field's 100")
p.add_argument("--size", type=int, default=10 ** 12)
p.add_argument("--label", default="")
args = p.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import nice_amd as N  # noqa: E402
from nice_amd import api, survey  # noqa: E402

BASE, CHUNK, FLOOR = 50, 10 ** 8, 250
START = 26_507_984_537_059_635 + args.window * 10 ** 11
END = START + args.size


def emit(side, **kw):
    print(json.dumps(dict(side=side, label=args.label, **kw)), flush=True)


ctx = None if args.sides == ["cpu"] else N.GpuContext(0)
for side in args.sides:
    for rep in range(-1, args.reps):  # -1: the warm-up
        t0 = time.perf_counter()
        if side == "ranges":
            roots = api.chunk_roots(START, END, CHUNK)
            t1 = time.perf_counter()
            bounds, counts = ctx.msd_ranges(roots, BASE, FLOOR)
            wall = time.perf_counter() - t1
            st = ctx.msd_ranges_stats()
            out = dict(roots=len(roots), ranges=len(bounds), numbers=st.numbers, launches=st.launches,
                       fused_roots=st.fused_roots, level_roots=st.level_roots, wall_ms=wall * 1e3,
                       kernel_ms=st.kernel_ms, order_ms=st.order_ms,
                       copy_back_and_host_ms=wall * 1e3 - st.kernel_ms - st.order_ms)
        elif side == "field":
            nice, st = ctx.niceonly_raw(START, END, BASE, msd_floor=FLOOR, chunk_size=CHUNK, msd_where="device")
            out = dict(ranges=st.ranges, numbers=st.range_numbers, candidates=st.candidates, launches=st.launches,
                       msd_ms=st.msd_seconds * 1e3, total_ms=st.total_seconds * 1e3, found=len(nice))
        elif side == "cpu":
            if rep >= 1:
                break  # tens of seconds a run: the warm-up and one repetition
            roots = api.chunk_roots(START, END, CHUNK)
            t1 = time.perf_counter()
            bounds, counts = api.msd_ranges_cpu(roots, BASE, FLOOR, threads=16)
            out = dict(roots=len(roots), ranges=len(bounds), threads=16, wall_ms=(time.perf_counter() - t1) * 1e3)
        else:
            kw = dict(msd_where="device") if side == "survey-device" else {}
            r = survey.survey_niceonly_base(ctx, BASE, threads=16, **kw)
            out = dict(windows=len(r.windows), reference=r.reference.counts(), sound=r.sound.counts())
        emit(side, rep=rep, seconds=time.perf_counter() - t0, **out)
if ctx is not None:
    ctx.close()
