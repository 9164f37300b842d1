"""Shared by test_nice_min_hook.py (CPU) and test_gpu_nice_list.py (GPU): the
windows on which the niceonly kernels' nice list is not empty once
nice_debug_set_nice_min lowers the threshold, and what the list must hold.

No nice number is known on any niceonly fast base, so in production every
in-range list is [].  With the hook at nice_min a compile-time kernel lists
every stride candidate whose square is repeat-free (a "square survivor") and
whose digit union of n^2 and n^3 has >= nice_min members.  The expectation is
the oracle's at the same threshold (process_field_niceonly_sq(nice_min=)); for
filter="sound" it is the Python restatement's (sound_restatement.sound_field).

Every window here must give, by the oracle alone, >= MIN_SURVIVORS square
survivors with >= MIN_COUNTS distinct union counts: test_nice_min_hook.py
checks that on the CPU, so no GPU comparison is [] against [].
"""
import contextlib
import functools
import os

from nice_amd import _lib
from oracle import oracle as O

import sound_restatement as SR
from test_sound_filter import FAST, K

THREADS = min(16, os.cpu_count() or 1)
MIN_SURVIVORS = 8
MIN_COUNTS = 3

FUSED = (3 * 10 ** 6, 10 ** 6)   # msd_fused_kernel + niceonly_kernel; with msd_where="host", niceonly_kernel alone
WAVE = (4 * 10 ** 7, 10 ** 7)    # level BFS + msd_wave_kernel
# b64 has no stride candidate anywhere (nice_debug_cube_count reaches it)
BASES = [b for b in FAST if b != 64]
# window start a = s + K[b] (e - s) // 256 with test_sound_filter's K, except
# b80: at K = 88 its windows hold 1 and 8 square survivors, and most of its
# range holds none.  The densest 3e6 (on 1e6 chunks) and 4e7 (on 1e7 chunks) of
# the 1e10 numbers from 0.9 of the range on, found with the oracle, hold 17 and 56.
B80_OFFSET = {"fused": 2190 * 10 ** 6, "wave": 167 * 10 ** 7}
# the wave path's three candidate walks: narrow lane walk, wide lane walk
# (n past 64 bits), packed groups (three-word bases)
WAVE_WALKS = (45, 57, 65)

# (start, size) of the b40 field whose list at nice_min 1 outgrows the device
# list's first 2^16 entries: 170 413 on 1e8 chunks (test_nice_min_hook.py)
GROW_FIELD = (O.base_range(40)[0], 2 * 10 ** 9)


def start(base, kind):
    s, e = O.base_range(base)
    if base == 80:
        return s + int((e - s) * 0.9) + B80_OFFSET[kind]
    return s + K[base] * (e - s) // 256


def window(base, kind):
    """(a, size, chunk) of the base's "fused" or "wave" window."""
    size, chunk = FUSED if kind == "fused" else WAVE
    return start(base, kind), size, chunk


@functools.lru_cache(maxsize=None)
def reference_field(a, size, base, chunk):
    """(ranges, candidates, square_ok, [(n, union count)] of every square
    survivor, ascending) of the reference-filter field, by the oracle."""
    O.lib().oracle_set_filter_c(1)
    res, cands, ranges, sq = O.process_field_niceonly_sq(a, a + size, base, THREADS, chunk, nice_min=1)
    assert len(res.nice_numbers) == sq
    return ranges, cands, sq, res.nice_numbers


@functools.lru_cache(maxsize=None)
def sound_survivors(a, size, base, chunk):
    """[(n, union count)] of the sound field's square survivors, ascending, by
    the restatement."""
    try:
        return [(n, SR.union_count(n, base)) for n in SR.sound_field(a, size, base, chunk, 250, 1)[4]]
    finally:
        O.lib().oracle_set_filter_c(1)


def thresholds(surv):
    """Every distinct union count of the survivors, and max + 1 (nothing listed)."""
    counts = sorted({u for _, u in surv})
    return counts + [counts[-1] + 1]


def listed(surv, nice_min):
    return [n for n, u in surv if u >= nice_min]


@contextlib.contextmanager
def lowered(base, nice_min):
    """Niceonly fields of `base` submitted inside the block list union counts
    >= nice_min; production is restored on the way out, whatever happens."""
    L = _lib.lib()
    assert L.nice_debug_set_nice_min(base, nice_min) == _lib.NICE_OK
    try:
        yield nice_min
    finally:
        assert L.nice_debug_set_nice_min(base, 0) == _lib.NICE_OK
