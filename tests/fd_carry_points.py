"""Shared by test_fd_carry_points.py (CPU) and test_gpu_fd_carry_points.py
(GPU): the numbers at which the FD kernels' incremental n^2, n^3, 2n+1 and
3n+1 (radix B = b^2 limbs, fd2_kernel.hpp) carry DEEP -- past the top stepped
limb into the cached limbs, or into the upper limbs of 2n+1 and 3n+1.

A quantity Q crosses level k at n when floor(Q(n) / B^k) = floor(Q(n-1) / B^k)
+ 1: stepping n-1 -> n then carries into limb k.  Crossings of a high level
are rarer than any window the suite compares with the oracle (b80: a carry
past the top stepped limb of n^2 once per 1.8e11 steps, each deeper level 6400
times rarer), but they are deterministic: isqrt and an integer cube root find
them.  points(base) lists, per limb layout (cut interval) of the base's valid
range and per quantity, one crossing of every level that a 1e6 window is not
expected to hold; window_for() places such an n in the middle of one lane's
run, so the step n-1 -> n is taken by the kernel's stepping code and not by a
lane's from-scratch start.
"""
import functools
from math import isqrt

from oracle import oracle as O

import near_miss_windows as W

MARGIN = 50_000       # a point lies at least this far inside its cut interval
RARE = 10 ** 6        # a level is kept when its crossings come less often than once per RARE numbers
WINDOW = 20_001       # the map / batch window around a point: chunk 41 at 512 threads, 21 at 1024
LANE = 100

QUANTITIES = {
    "S": lambda n: n * n,
    "C": lambda n: n * n * n,
    "D1": lambda n: 2 * n + 1,
    "N3": lambda n: 3 * n + 1,
}


def limbs(x, base):
    """Radix-b^2 limbs of x >= 1."""
    B, k = base * base, 0
    while x >= B ** k:
        k += 1
    return k


def icbrt_ceil(x):
    """The least r with r^3 >= x."""
    if x <= 1:
        return max(x, 0)
    r = 1 << ((x.bit_length() + 2) // 3)  # >= the root: Newton descends to its floor
    while True:
        nr = (2 * r + x // (r * r)) // 3
        if nr >= r:
            break
        r = nr
    return r if r ** 3 == x else r + 1


def first_reaching(q, v):
    """The least n >= 0 with Q(n) >= v."""
    if v <= QUANTITIES[q](0):
        return 0
    if q == "S":
        return isqrt(v - 1) + 1
    if q == "C":
        return icbrt_ceil(v)
    return -((1 - v) // (2 if q == "D1" else 3))  # ceil((v - 1) / 2 or 3)


def crosses(q, k, n, base):
    """The crossing identity."""
    Bk = (base * base) ** k
    return QUANTITIES[q](n) // Bk == QUANTITIES[q](n - 1) // Bk + 1


def layout_cuts(base):
    """The limb-layout cuts by their definition (fd2_detailed.hip; the
    arithmetic of test_gpu_parity._fd2_cuts): the n at which the limb counts of
    2e+1, 3e^2+3e+1 and 6e+6 at a segment end e change inside the valid range."""
    def combo(e):
        return limbs(2 * e + 1, base), limbs(3 * e * e + 3 * e + 1, base), limbs(6 * e + 6, base)

    s, e = O.base_range(base)
    cuts, a = [], s
    while combo(a + 1) != combo(e):
        lo, hi, cur = a + 1, e, combo(a + 1)
        while lo < hi:
            mid = (lo + hi) // 2
            if combo(mid) == cur:
                lo = mid + 1
            else:
                hi = mid
        cuts.append(lo - 1)
        a = lo - 1
    return cuts


def intervals(base):
    """[(first n, end)] of the base's limb layouts: the valid range split at
    its cuts (a segment's layout is that of its end, so the cut itself is the
    first n of the next interval)."""
    s, e = O.base_range(base)
    edges = [s] + W.cuts_of(base) + [e]
    return list(zip(edges, edges[1:]))


def first_crossing(q, k, lo, hi, base):
    """The first n in [lo, hi] at which Q crosses level k, or None."""
    Bk = (base * base) ** k
    n = first_reaching(q, (QUANTITIES[q](lo - 1) // Bk + 1) * Bk)
    return n if n <= hi else None


@functools.lru_cache(maxsize=None)
def points(base):
    """[((first n, end), quantity, level, n*)]: per cut interval and quantity,
    for every level k >= 1 crossed at least MARGIN inside the interval but
    less often than once per RARE numbers of it, the first crossing at or after
    the interval's middle (the first one inside, if none comes after)."""
    B = base * base
    out = []
    for a, e in intervals(base):
        lo, hi = a + MARGIN, e - MARGIN - 1
        if lo > hi:
            continue
        for q, Q in QUANTITIES.items():
            for k in range(1, limbs(Q(e), base) + 1):
                Bk = B ** k
                first = first_crossing(q, k, lo, hi, base)
                if first is None:
                    continue
                crossings = Q(e - 1) // Bk - Q(a) // Bk
                if crossings * RARE >= e - a:
                    continue
                n = first_crossing(q, k, max(lo, (a + e) // 2), hi, base)
                n = first if n is None else n
                assert lo <= n <= hi and crosses(q, k, n, base)
                out.append(((a, e), q, k, n))
    return out


def deepest(base, q, interval=None):
    """The point of the highest level of quantity q (in one interval, or in the
    base's first one)."""
    iv = intervals(base)[0] if interval is None else interval
    return max((p for p in points(base) if p[0] == iv and p[1] == q), key=lambda p: p[2])


def window_for(n_star, chunk, lane=LANE):
    """The first number of a window tiled in lanes of `chunk` numbers in which
    n* is number chunk // 2 of lane `lane`'s run."""
    return n_star - (lane * chunk + chunk // 2)
