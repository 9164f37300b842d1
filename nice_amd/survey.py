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
"""
from __future__ import annotations

import math
import random
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
