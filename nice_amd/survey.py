"""Survey of a base: the unique-digit distribution of a stratified sample of
its valid range, in ONE batched detailed call (GpuContext.detailed_ranges with
sum=True; the library's CPU twin when no context is given).

The base range is cut into `windows` equal strata; window j covers
`window_size` numbers from a seeded offset inside stratum j (clipped to the
range), so the sample follows the whole range instead of one place in it.
The result is what places the FD kernel's histogram windows
(scripts/fd2_windows.py) and what the reference fits its per-base
distributions to: mean and standard deviation of niceness = uniques / base,
weighted by count (distribution_stats.rs:75-90).

    python -m nice_amd --survey --base 50 --windows 4096 --window-size 100000 --gpu

survey_niceonly_base asks the other question of the same windows: what a
niceonly search of the base would have to do -- how much of it survives the MSD
filter, how dense the stride candidates are, how many squares survive --
under the reference filter and under the sound one, through batched niceonly
calls (GpuContext.niceonly_ranges).

    python -m nice_amd --survey-niceonly --base 50 --windows 4096 --gpu
"""
from __future__ import annotations

import dataclasses
import math
import random
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import List, Optional, Tuple

from . import api


@dataclass
class SurveyResult:
    base: int
    windows: List[Tuple[int, int]]        # the sampled [start, end)
    distribution: List[int]               # bins 0..base, summed over the windows
    near_misses: List[Tuple[int, int]]    # (n, uniques), window by window
    mean: float                           # of niceness = uniques / base
    stdev: float

    @property
    def numbers(self) -> int:
        return sum(self.distribution)


def survey_windows(base: int, windows: int, window_size: int, seed: int = 0) -> List[Tuple[int, int]]:
    """Window j: window_size numbers from a seeded offset inside the j-th of
    `windows` equal strata of the base range, clipped to the range."""
    r = api.get_base_range_u128(base)
    if r is None:
        raise ValueError(f"base {base} has no valid range")
    if windows < 1 or window_size < 1:
        raise ValueError("windows and window_size must be positive")
    s, e = r.range_start, r.range_end
    size = e - s
    windows = min(windows, size)
    rng = random.Random(seed)
    out = []
    for j in range(windows):
        a, b = s + size * j // windows, s + size * (j + 1) // windows  # stratum j
        start = a + rng.randrange(b - a)
        out.append((start, min(e, start + window_size)))
    return out


def mean_stdev(distribution: List[int], base: int) -> Tuple[float, float]:
    """Count-weighted mean and standard deviation of niceness = uniques / base
    (the rule of distribution_stats.rs:75-90)."""
    total = sum(distribution)
    if total <= 0:
        raise ValueError("empty distribution")
    mean = sum(u / base * c for u, c in enumerate(distribution)) / total
    second = sum((u / base) ** 2 * c for u, c in enumerate(distribution)) / total
    return mean, math.sqrt(max(0.0, second - mean * mean))


def survey_base(ctx: Optional[api.GpuContext], base: int, windows: int = 4096,
                window_size: int = 100_000, seed: int = 0, threads: int = 1) -> SurveyResult:
    """The summed distribution of a stratified sample of the base's range.
    Deterministic in `seed`.  ctx=None: the CPU twin (`threads` host threads)."""
    w = survey_windows(base, windows, window_size, seed)
    if ctx is None:
        rows, lst = api.detailed_ranges_cpu(w, base, sum=True, threads=threads)
    else:
        rows, lst = ctx.detailed_ranges(w, base, sum=True)
    dist = rows[0]
    # (windows of neighbouring strata can overlap: a number in two windows is
    # counted and listed once per window)
    near = [(n, u) for n, u, _ in lst]
    mean, stdev = mean_stdev(dist, base)
    return SurveyResult(base, w, dist, near, mean, stdev)


def class_distribution(ctx: Optional[api.GpuContext], base: int, modulus: int, windows: int = 4096,
                       window_size: int = 100_000, seed: int = 0, threads: int = 1) -> List[List[int]]:
    """The unique-digit distribution of survey_windows' sample split by residue
    class: table[c][u] = the sampled numbers n with n % modulus == c and u unique
    digits (rows 0..modulus-1, bins 0..base).  Summed over the classes it is
    survey_base's distribution for the same windows and seed.  This is the
    conditioning behind the reference's residue filter (modulus = base - 1) and
    its low-digit filters (modulus = base, base^2).

    On a GPU context everything stays on the device: each window's map
    (GpuContext.unique_map into a torch tensor) is binned with torch.bincount
    of cls * (base + 1) + u; no device code beyond the map.  For that, torch
    and the library must share one HIP runtime: import torch (and let it find
    the GPU) BEFORE the library is first loaded, as bench.py does -- a library
    loaded first brings the system's runtime, torch then loads its own copy
    and finds no device.  ctx=None: the CPU twin's maps (`threads` host
    threads), binned with numpy.  Deterministic in `seed`."""
    if modulus < 1:
        raise ValueError("modulus must be positive")
    w = survey_windows(base, windows, window_size, seed)
    nb = base + 1
    if ctx is None:
        import numpy as np
        table = np.zeros(modulus * nb, dtype=np.int64)
        for s, e in w:
            u = api.unique_map_cpu(s, e, base, threads).astype(np.int64)
            cls = (np.arange(e - s, dtype=np.int64) + s % modulus) % modulus
            table += np.bincount(cls * nb + u, minlength=modulus * nb)
        return table.reshape(modulus, nb).tolist()
    import torch
    dev = torch.device("cuda", ctx.devices[0])
    table = torch.zeros(modulus * nb, dtype=torch.int64, device=dev)
    longest = max(e - s for s, e in w)
    buf = torch.empty(longest, dtype=torch.uint8, device=dev)
    idx = torch.arange(longest, dtype=torch.int64, device=dev)
    for s, e in w:
        u = ctx.unique_map(s, e, base, out=buf)[: e - s].to(torch.int64)
        cls = (idx[: e - s] + s % modulus) % modulus
        # (the next unique_map waits for this stream before it overwrites buf)
        table += torch.bincount(cls * nb + u, minlength=modulus * nb)
    return table.reshape(modulus, nb).tolist()


# ranges per batched niceonly call (the library takes at most 2^20)
NICEONLY_BATCH = 1 << 20


@dataclass
class NiceonlyFilterSurvey:
    """What one MSD filter leaves of the sampled windows."""
    filter: str          # "reference" or "sound"
    msd_ranges: int      # MSD-surviving ranges
    msd_numbers: int     # numbers inside them
    candidates: int      # their stride candidates (k = 2)
    square_ok: int       # ... with a repeat-free square
    found: List[int]     # the numbers that passed, window by window
    # survey_niceonly_base(prefix_test=True), the sound column: the candidates
    # the per-candidate prefix test rejected; square_ok then counts the kept ones
    prefix_rejected: int = 0
    with_prefix: bool = False  # the survey was asked for the prefix test: counts() shows prefix_rejected

    def counts(self) -> dict:
        out = {"msd_ranges": self.msd_ranges, "msd_numbers": self.msd_numbers, "candidates": self.candidates,
               "square_ok": self.square_ok, "found": len(self.found)}
        if self.with_prefix:
            out["prefix_rejected"] = self.prefix_rejected
        return out


@dataclass
class NiceonlySurveyResult:
    base: int
    windows: List[Tuple[int, int]]   # the sampled [start, end)
    msd_floor: int
    range_size: int                  # numbers in the base's valid range
    sampled: int                     # numbers in the windows
    reference: NiceonlyFilterSurvey
    sound: NiceonlyFilterSurvey

    def scaled(self, which: str) -> dict:
        """A filter's counts (and the sampled numbers) scaled to the whole base
        range: count * range_size / sampled."""
        out = {k: v * self.range_size / self.sampled for k, v in getattr(self, which).counts().items()}
        out["sampled"] = float(self.range_size)
        return out


def _msd_ranges(window, base, floor, filt):
    s, e = window
    if e - s <= floor:  # get_valid_ranges_recursive emits such a range untested
        return [window]
    return [(r.range_start, r.range_end)
            for r in api.get_valid_ranges(api.FieldSize(s, e), base, floor, filt)]


def _niceonly_batch(ctx, part, base, threads, prefix):
    """(candidates, square_ok, prefix_rejected, found) of one batched call."""
    if prefix:
        c, q, rej, lst = (api.niceonly_ranges_ex_cpu(part, base, prefix_test=True, threads=threads) if ctx is None
                          else ctx.niceonly_ranges_ex(part, base, prefix_test=True))
    else:
        c, q, lst = (api.niceonly_ranges_cpu(part, base, threads=threads) if ctx is None
                     else ctx.niceonly_ranges(part, base))
        rej = ()
    return sum(c), sum(q), sum(rej), [n for n, _ in lst]


def _device_filter_survey(ctx, w, base, floor, filt, prefix=False) -> NiceonlyFilterSurvey:
    """One filter's column with the MSD recursion on the device: the windows
    are the roots of ctx.msd_ranges, its bounds the ranges of niceonly_ranges."""
    n_ranges = numbers = cand = sq = rej = 0
    found: List[int] = []
    for i in range(0, len(w), NICEONLY_BATCH):
        bounds, _ = ctx.msd_ranges(w[i:i + NICEONLY_BATCH], base, floor, filt)
        n_ranges += len(bounds)
        numbers += bounds.numbers()
        for j in range(0, len(bounds), NICEONLY_BATCH):
            part = bounds if len(bounds) <= NICEONLY_BATCH else bounds.part(j, j + NICEONLY_BATCH)
            c, q, r, f = _niceonly_batch(ctx, part, base, 1, prefix)
            cand, sq, rej, found = cand + c, sq + q, rej + r, found + f
    return NiceonlyFilterSurvey(filt, n_ranges, numbers, cand, sq, found, rej, prefix)


def survey_niceonly_base(ctx: Optional[api.GpuContext], base: int, windows: int = 4096,
                         window_size: int = 10 ** 6, seed: int = 0, msd_floor: int = 250,
                         threads: int = 1, msd_where: str = "host",
                         prefix_test: bool = False) -> NiceonlySurveyResult:
    """What a niceonly search of `base` would cost, from the stratified windows
    of survey_windows.  Per window the MSD filter (nice_msd_valid_ranges_ex,
    floor msd_floor) runs on `threads` host threads, once under the reference
    filter and once under the sound one; the surviving ranges of all windows
    go through batched niceonly calls (ctx.niceonly_ranges; ctx=None: the CPU
    twin on `threads` threads).  Reported per filter: MSD-surviving ranges and
    numbers, stride candidates, square survivors and the numbers found, and
    through scaled() each of these scaled to the whole base range.  No time
    estimate: nothing here has measured one.

    msd_where="device" (needs ctx): the MSD filter of all windows runs on the
    GPU instead, one ctx.msd_ranges call per filter (per 2^20 windows), and its
    range list goes to ctx.niceonly_ranges as it is.  Both placements return
    equal results.

    The sound column counts the candidates of the ranges the sound MSD filter
    leaves, i.e. BEFORE the field path's per-candidate prefix test, which
    rejects some of them ahead of the square test.  prefix_test=True runs that
    test too, per range (niceonly_ranges_ex: a mask per range handed in, on
    the ranges the field path tests -- a niceonly fast base, k = 2): the sound
    column's prefix_rejected counts the rejected candidates, its square_ok
    only the kept ones -- the sound field's figures -- and both columns'
    counts() gain a prefix_rejected entry (0 under the reference filter, where
    no such test exists).  The default leaves every figure as it was.
    square_ok is counted on the GPU only for a niceonly fast base (k = 2,
    ranges inside the valid range -- every window is); elsewhere it reads 0
    there, while the CPU twin counts it for every base.
    Deterministic in `seed`."""
    if msd_where not in ("host", "device"):
        raise ValueError("msd_where must be 'host' or 'device'")
    if msd_where == "device" and ctx is None:
        raise ValueError("msd_where='device' needs a GpuContext")
    w = survey_windows(base, windows, window_size, seed)
    r = api.get_base_range_u128(base)
    # windows no larger than the floor: the MSD recursion emits each untested
    # (see _msd_ranges), under either filter
    small = all(e - s <= msd_floor for s, e in w)
    per_filter = {}
    with ThreadPoolExecutor(max(1, threads)) as pool:
        for filt in ("reference", "sound"):
            prefix = prefix_test and filt == "sound"
            if small and per_filter and not prefix_test:
                per_filter[filt] = dataclasses.replace(per_filter["reference"], filter=filt)
                continue
            if small:
                ranges = list(w)
            elif msd_where == "device":
                per_filter[filt] = dataclasses.replace(_device_filter_survey(ctx, w, base, msd_floor, filt, prefix),
                                                       with_prefix=prefix_test)
                continue
            else:
                ranges = [x for rs in pool.map(lambda win: _msd_ranges(win, base, msd_floor, filt), w)
                          for x in rs]
            cand = sq = rej = 0
            found: List[int] = []
            for i in range(0, len(ranges), NICEONLY_BATCH):
                c, q, r_, f = _niceonly_batch(ctx, ranges[i:i + NICEONLY_BATCH], base, threads, prefix)
                cand, sq, rej, found = cand + c, sq + q, rej + r_, found + f
            per_filter[filt] = NiceonlyFilterSurvey(filt, len(ranges), sum(b - a for a, b in ranges), cand, sq,
                                                    found, rej, prefix_test)
    return NiceonlySurveyResult(base, w, msd_floor, r.range_end - r.range_start, sum(b - a for a, b in w),
                                per_filter["reference"], per_filter["sound"])
