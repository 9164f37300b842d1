"""Shared by test_near_miss_hook.py (CPU) and test_gpu_near_miss_list.py (GPU):
where the FD kernels' near-miss list is not empty once the cutoff is lowered
with nice_debug_set_near_miss_cutoff, and the oracle calls that say what it
must hold.

In production a listed number is a once-in-1e8 event (u > floor(0.9 b)).  At
cutoff W0 + W - 1, the top of the base's compile-time histogram window, every
number on the kernels' high out-of-window branch is listed: tens to thousands
per 1e6 numbers at the fractions below.
"""
import contextlib
import ctypes
import os

from nice_amd import _lib
from oracle import oracle as O

THREADS = min(16, os.cpu_count() or 1)

# base -> fraction of the base's range where a 1e6 window has >= 8 numbers
# above the histogram window (the range start is a bad place: n^2 starts
# 1 0 0 0 ... there and most bases list nothing).  Fractions only: the counts
# come from the oracle at run time, and test_near_miss_hook.py checks the >= 8.
WINDOW_FRAC = {40: 0.5, 42: 0.5, 43: 0.5, 44: 0.5, 45: 0.5, 47: 0.5, 48: 0.8, 49: 0.7, 50: 0.5,
               52: 0.5, 53: 0.5, 54: 0.4, 55: 0.5, 57: 0.5, 58: 0.5, 59: 0.5, 60: 0.5, 62: 0.5,
               63: 0.5, 64: 0.7, 65: 0.45, 67: 0.4, 68: 0.55, 80: 0.5}
WINDOW = 10 ** 6
MIN_ENTRIES = 8


def fd_bases():
    return [b for b in range(2, 129) if _lib.lib().nice_fd_kernel_base(b) == 1]


def fd_window(base):
    """(W0, W) of the base's FD kernel (nice_debug_fd_window)."""
    w0, w = ctypes.c_uint32(), ctypes.c_uint32()
    assert _lib.lib().nice_debug_fd_window(base, w0, w) == _lib.NICE_OK
    return w0.value, w.value


def low_cutoff(base):
    """The lowest cutoff the FD launchers take: the window's last bin."""
    w0, w = fd_window(base)
    return w0 + w - 1


def at(base, frac):
    s, e = O.base_range(base)
    return s + int((e - s) * frac)


def window(base, size=WINDOW):
    a = at(base, WINDOW_FRAC[base])
    return a, a + size


def cuts_of(base):
    buf = (ctypes.c_uint64 * 16)()
    n = ctypes.c_size_t()
    assert _lib.lib().nice_fd_segment_cuts(base, buf, 8, n) == 0
    return [buf[2 * i] | (buf[2 * i + 1] << 64) for i in range(n.value)]


def oracle(a, e, base, cutoff=None):
    """(hist with base + 1 bins, [(n, u)]) of [a, e) by the oracle on THREADS
    threads, listing u > cutoff (None: production)."""
    r = O.process_field_detailed_mt(a, e, base, THREADS, cap=min(e - a, 1 << 22), cutoff=cutoff,
                                    chunk=max(1000, (e - a) // (8 * THREADS)))
    return [0] + [c for _, c in r.distribution], r.nice_numbers


@contextlib.contextmanager
def lowered(base, cutoff=None):
    """The GPU detailed paths of `base` list u > cutoff (default: low_cutoff)
    inside the block; production is restored on the way out, whatever happens."""
    L = _lib.lib()
    c = low_cutoff(base) if cutoff is None else cutoff
    assert L.nice_debug_set_near_miss_cutoff(base, c) == _lib.NICE_OK
    try:
        yield c
    finally:
        assert L.nice_debug_set_near_miss_cutoff(base, 0) == _lib.NICE_OK
