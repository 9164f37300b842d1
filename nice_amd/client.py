"""nice_client drop-in for the offline path (client/src/main.rs).

Supports the reference client's flag surface for field processing
(main.rs:60-116): mode (detailed | niceonly, env NICE_MODE), --benchmark,
--gpu, --gpu-device (extended: a list "0,1,2" or "all" shards one field over
several GPUs), --threads (host MSD workers for niceonly), --no-progress,
--log-level, --username, --repeat.  Fields come from --benchmark or from an
explicit --range/--base; the reference's HTTP claim/submit/validate transport
(client_api_*.rs) is out of scope, so --validate
compares against a JSON file of a canonical submission instead of the server.

With --gpu a field runs on the HIP path (process_range_*_gpu, one call per
field).  Without it, the reference's CPU mode (main.rs:154-207): the field is
cut into client chunks (1e6 * clamp(ceil(size / 1e11), 1, 1000)), the chunks
are processed by --threads workers through the library's CPU API
(nice_cpu_process_range_detailed / _niceonly, the reference's
process_range_detailed / process_range_niceonly), and the per-chunk results are
merged in chunk order (compile_results).  No GPU is touched in that mode.

    python -m nice_amd detailed --benchmark extra-large --gpu
    python -m nice_amd --benchmark base-ten            # CPU mode
    python -m nice_amd --survey --base 50 --gpu        # distribution of a sampled base range
    python -m nice_amd --survey-niceonly --base 50 --gpu   # what a niceonly search of the base would cost
    python -m nice_amd --survey-classes 49 --base 50 --gpu # the distribution split by n mod 49
    python -m nice_amd --map out.npy --base 40 --range S E --gpu   # the unique count of every n of a range
"""
from __future__ import annotations

import argparse
import json
import logging
import os
import sys
import time

from . import api
from .benchmark import BenchmarkMode, get_benchmark_field
from .types import DataToClient, DataToServer, SearchMode

log = logging.getLogger("nice_client")


def _msd_floor(v: str):
    return v if v == "adaptive" else int(v)


def parse_args(argv=None):
    env = os.environ.get
    p = argparse.ArgumentParser(prog="nice_client", description=__doc__.split("\n")[0])
    p.add_argument("mode", nargs="?", default=env("NICE_MODE", "detailed"),
                   choices=["detailed", "niceonly"])
    p.add_argument("--api-base", default=env("NICE_API_BASE", "https://api.nicenumbers.net"))
    p.add_argument("--api-max-retries", type=int, default=int(env("NICE_API_MAX_RETRIES", 10)))
    p.add_argument("-u", "--username", default=env("NICE_USERNAME", "anonymous"))
    p.add_argument("-r", "--repeat", action="store_true", default=bool(env("NICE_REPEAT")))
    p.add_argument("-n", "--no-progress", action="store_true", default=bool(env("NICE_NO_PROGRESS")))
    p.add_argument("-t", "--threads", type=int, default=int(env("NICE_THREADS", 4)))
    p.add_argument("-b", "--benchmark", default=env("NICE_BENCHMARK"),
                   choices=[m.value for m in BenchmarkMode])
    p.add_argument("--validate", default=env("NICE_VALIDATE"),
                   help="JSON file with the canonical submission to compare against")
    p.add_argument("--gpu", action="store_true", default=bool(env("NICE_GPU")))
    p.add_argument("--gpu-device", default=env("NICE_GPU_DEVICE", "0"),
                   help="device ordinal, comma list, or 'all'")
    p.add_argument("-l", "--log-level", default=env("NICE_LOG_LEVEL", "info"),
                   choices=["off", "error", "warn", "info", "debug", "trace"])
    p.add_argument("--base", type=int, help="explicit field: base")
    p.add_argument("--range", nargs=2, type=int, metavar=("START", "END"),
                   help="explicit field: half-open [START, END)")
    p.add_argument("--hi-base-size", type=int, default=None,
                   help="hi-base field size (code: 1e9, doc/BASELINE: 1e6)")
    p.add_argument("--msd-floor", type=_msd_floor, default=0,
                   help="niceonly MSD floor: a number (0 = 250, or NICE_GPU_MSD_FLOOR), or "
                        "'adaptive' for the reference GPU path's adaptive floor "
                        "(client_process_gpu.rs:96-184)")
    p.add_argument("--sound", action="store_true", default=bool(env("NICE_SOUND")),
                   help="niceonly: the sound filter (no Filter C, which can drop numbers it has not "
                        "ruled out; a per-candidate prefix test instead) -- a complete answer")
    p.add_argument("--survey", action="store_true",
                   help="survey --base: the unique-digit distribution of a stratified sample of its "
                        "valid range in one batched call (nice_amd/survey.py); with --gpu on the GPU")
    p.add_argument("--survey-niceonly", action="store_true",
                   help="survey --base for a niceonly search: MSD survival, stride candidates, square survivors "
                        "and numbers found in the same stratified windows, under the reference and the sound "
                        "filter (nice_amd/survey.py survey_niceonly_base); with --gpu on the GPU; --msd-floor "
                        "as a number (0 = 250)")
    p.add_argument("--survey-msd", choices=("host", "device"), default="host",
                   help="--survey-niceonly: where the windows' MSD filter runs -- the host recursion per "
                        "window, or (with --gpu) one device range-list call per filter (GpuContext.msd_ranges)")
    p.add_argument("--survey-prefix", action="store_true",
                   help="--survey-niceonly: run the sound filter's per-candidate prefix test on the sound "
                        "column's ranges too (prefix_rejected; square_ok then counts the kept candidates)")
    p.add_argument("--survey-classes", type=int, default=None, metavar="M",
                   help="survey --base by residue class: the table [n mod M][num_uniques] of the same "
                        "stratified windows, from the per-number map (nice_amd/survey.py class_distribution); "
                        "with --gpu computed on the GPU")
    p.add_argument("--map", default=None, metavar="OUT.npy",
                   help="write the per-number map of --range/--base (one uint8 per n: its unique-digit count) "
                        "as a .npy file; with --gpu on the GPU, else on --threads host threads")
    p.add_argument("--windows", type=int, default=4096, help="--survey, --survey-niceonly: sample windows (strata)")
    p.add_argument("--window-size", type=int, default=None,
                   help="numbers per window (--survey: 100000, --survey-niceonly: 1000000)")
    p.add_argument("--seed", type=int, default=0, help="--survey, --survey-niceonly: seed of the window offsets")
    args = p.parse_args(argv)
    if args.window_size is None:
        args.window_size = 100_000 if args.survey or not args.survey_niceonly else 1_000_000
    return args


def _devices(spec: str):
    if spec == "all":
        import ctypes
        n = ctypes.c_int()
        api.lib().nice_device_count(n)
        return list(range(max(1, n.value)))
    return [int(x) for x in str(spec).split(",") if x.strip() != ""]


def compile_results(results, claim: DataToClient, username: str, mode: SearchMode) -> DataToServer:
    """compile_results (client/src/main.rs:212-254)."""
    nice = [n for r in results for n in r.nice_numbers]
    if mode is SearchMode.NICEONLY:
        dist = None
    else:
        acc = {}
        for r in results:
            for d in r.distribution:
                acc[d.num_uniques] = acc.get(d.num_uniques, 0) + d.count
        from .types import UniquesDistributionSimple
        dist = [UniquesDistributionSimple(k, v) for k, v in sorted(acc.items())]
    return DataToServer(claim.claim_id, username, api.CLIENT_VERSION, dist, nice)


def validate_results(submit: DataToServer, canon: dict, mode: SearchMode) -> bool:
    """validate_results (client/src/main.rs:258-292), against a canonical JSON."""
    ok = True
    ours = sorted((n.number, n.num_uniques) for n in submit.nice_numbers)
    theirs = sorted((int(n["number"]), int(n["num_uniques"])) for n in canon["nice_numbers"])
    if ours != theirs:
        log.error("VALIDATION FAILED: Semi-nice numbers don't match!")
        ok = False
    if mode is SearchMode.DETAILED and submit.unique_distribution is not None:
        a = sorted((d.num_uniques, d.count) for d in submit.unique_distribution)
        b = sorted((int(d["num_uniques"]), int(d["count"])) for d in canon["unique_distribution"])
        if a != b:
            log.error("VALIDATION FAILED: Distribution doesn't match!")
            ok = False
    return ok


def process_field_sync(claim: DataToClient, mode: SearchMode, args, ctx=None):
    """process_field_sync (client/src/main.rs:120-208): the GPU call for the
    whole field with --gpu, else the CPU path per client chunk on --threads
    workers (rayon par_iter in the reference), results in chunk order."""
    field = claim.field()
    if args.gpu:
        if mode is SearchMode.DETAILED:
            return [api.process_range_detailed_gpu(ctx, field, claim.base)]
        return [api.process_range_niceonly_gpu(ctx, field, claim.base, threads=args.threads,
                                               msd_floor=args.msd_floor,
                                               filter="sound" if args.sound else "reference")]
    from concurrent.futures import ThreadPoolExecutor
    from .dist import client_chunk_size
    from .types import FieldSize
    chunk = client_chunk_size(field.range_size)
    chunks = [FieldSize(a, min(field.range_end, a + chunk))
              for a in range(field.range_start, field.range_end, chunk)]
    if mode is SearchMode.DETAILED:
        def work(c):
            return api.process_range_detailed_cpu(c, claim.base)
    else:
        # main.rs:173-180: one stride table for the field (k = 2, main.rs:19)
        table = api.StrideTable.new(claim.base, 2)

        def work(c):
            return api.process_range_niceonly_cpu(c, claim.base, table,
                                                  filter="sound" if args.sound else "reference")
    # ctypes releases the GIL inside the library call, so the workers run the
    # chunks in parallel on the host cores
    with ThreadPoolExecutor(max(1, args.threads)) as pool:
        return list(pool.map(work, chunks))


def run_once(args, ctx) -> int:
    mode = SearchMode.DETAILED if args.mode == "detailed" else SearchMode.NICEONLY
    if args.benchmark:
        claim = get_benchmark_field(BenchmarkMode(args.benchmark), args.hi_base_size)
        log.info("Beginning benchmark:  %s", args.benchmark)
    elif args.range and args.base:
        s, e = args.range
        claim = DataToClient(0, args.base, s, e, e - s)
        log.info("Processing field: base %d [%d, %d)", args.base, s, e)
    else:
        log.error("no field: the server claim path is out of scope offline; "
                  "use --benchmark or --base/--range")
        return 2
    t0 = time.perf_counter()
    results = process_field_sync(claim, mode, args, ctx)
    elapsed = time.perf_counter() - t0
    # The reference prints this line with --no-progress or --gpu (main.rs:358-371);
    # this client has no progress bar, so it always does.
    log.info("✓ Processed %.2e numbers in %.2fs (%.2e numbers/sec)",
             claim.range_size, elapsed, claim.range_size / elapsed)
    submit = compile_results(results, claim, args.username, mode)
    log.debug("Submit Data: %s", json.dumps(submit.to_json()))
    for n in submit.nice_numbers:
        log.info("Nice number: %d (%d uniques)", n.number, n.num_uniques)
    if args.validate:
        with open(args.validate) as f:
            canon = json.load(f)
        if validate_results(submit, canon, mode):
            print("\nValidation passed! Results match the canoncical submission.")
        else:
            print("\nValidation failed! Results do not match the canoncical submission.")
            return 1
    return 0


def run_survey(args, ctx) -> int:
    """--survey: print the sampled distribution of --base as one JSON line."""
    from .survey import survey_base
    if not args.base:
        log.error("--survey needs --base")
        return 2
    t0 = time.perf_counter()
    r = survey_base(ctx, args.base, args.windows, args.window_size, args.seed, threads=max(1, args.threads))
    elapsed = time.perf_counter() - t0
    log.info("✓ Surveyed %.2e numbers of base %d in %.2fs", r.numbers, args.base, elapsed)
    print(json.dumps({"base": r.base, "windows": len(r.windows), "window_size": args.window_size,
                      "seed": args.seed, "numbers": r.numbers, "mean": r.mean, "stdev": r.stdev,
                      "distribution": r.distribution,
                      "near_misses": [[str(n), u] for n, u in r.near_misses]}))
    return 0


def run_survey_niceonly(args, ctx) -> int:
    """--survey-niceonly: print the niceonly survey of --base as one JSON line."""
    from .survey import survey_niceonly_base
    if not args.base:
        log.error("--survey-niceonly needs --base")
        return 2
    if args.msd_floor == "adaptive":
        log.error("--survey-niceonly needs a numeric --msd-floor")
        return 2
    if args.survey_msd == "device" and ctx is None:
        log.error("--survey-msd device needs --gpu")
        return 2
    floor = args.msd_floor or 250
    t0 = time.perf_counter()
    r = survey_niceonly_base(ctx, args.base, args.windows, args.window_size, args.seed, floor,
                             threads=max(1, args.threads), msd_where=args.survey_msd,
                             prefix_test=args.survey_prefix)
    elapsed = time.perf_counter() - t0
    log.info("✓ Surveyed %.2e numbers of base %d for niceonly in %.2fs", r.sampled, args.base, elapsed)
    out = {"base": r.base, "windows": len(r.windows), "window_size": args.window_size, "seed": args.seed,
           "msd_floor": floor, "range_size": str(r.range_size), "sampled": r.sampled}
    for which in ("reference", "sound"):
        f = getattr(r, which)
        out[which] = dict(f.counts(), numbers_found=[str(n) for n in f.found], scaled=r.scaled(which))
    print(json.dumps(out))
    return 0


def run_survey_classes(args, ctx) -> int:
    """--survey-classes M: print the table [n mod M][num_uniques] of --base as one JSON line."""
    from .survey import class_distribution
    if not args.base or args.survey_classes < 1:
        log.error("--survey-classes needs --base and a positive modulus")
        return 2
    t0 = time.perf_counter()
    table = class_distribution(ctx, args.base, args.survey_classes, args.windows, args.window_size, args.seed,
                               threads=max(1, args.threads))
    elapsed = time.perf_counter() - t0
    numbers = sum(sum(row) for row in table)
    log.info("✓ Surveyed %.2e numbers of base %d by n mod %d in %.2fs", numbers, args.base, args.survey_classes,
             elapsed)
    print(json.dumps({"base": args.base, "modulus": args.survey_classes, "windows": args.windows,
                      "window_size": args.window_size, "seed": args.seed, "numbers": numbers, "table": table}))
    return 0


def run_map(args, ctx) -> int:
    """--map OUT.npy: the per-number map of --range/--base."""
    import numpy as np
    if not (args.range and args.base):
        log.error("--map needs --base and --range")
        return 2
    s, e = args.range
    t0 = time.perf_counter()
    m = ctx.unique_map(s, e, args.base) if ctx is not None else api.unique_map_cpu(s, e, args.base,
                                                                                   max(1, args.threads))
    elapsed = time.perf_counter() - t0
    np.save(args.map, m)
    log.info("✓ Mapped %.2e numbers of base %d in %.2fs -> %s", e - s, args.base, elapsed, args.map)
    return 0


def main(argv=None) -> int:
    args = parse_args(argv)
    level = {"off": logging.CRITICAL + 10, "error": logging.ERROR, "warn": logging.WARNING,
             "info": logging.INFO, "debug": logging.DEBUG, "trace": logging.DEBUG}[args.log_level]
    logging.basicConfig(level=level, format="%(asctime)s %(levelname)s %(message)s")
    ctx = None
    if args.gpu:  # main.rs:592-625: the GPU context only in GPU mode
        log.info("GPU_BATCH_SIZE = %d", api.GPU_BATCH_SIZE)
        if args.survey_classes is not None:
            # the class survey bins the map with torch on the device: torch has to load its HIP
            # runtime before the library loads, so that the two share one (survey.class_distribution)
            import torch
            torch.cuda.init()
        try:
            ctx = api.GpuContext(_devices(args.gpu_device))
        except api._lib.NiceError as e:
            log.error("GPU processing error: %s", e)
            return 1
    else:
        log.info("CPU mode: %d threads", args.threads)
    if args.survey:
        return run_survey(args, ctx)
    if args.survey_niceonly:
        return run_survey_niceonly(args, ctx)
    if args.survey_classes is not None:
        return run_survey_classes(args, ctx)
    if args.map:
        return run_map(args, ctx)
    while True:
        rc = run_once(args, ctx)
        if rc or not args.repeat:
            return rc


if __name__ == "__main__":
    sys.exit(main())
