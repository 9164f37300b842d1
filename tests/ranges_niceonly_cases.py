"""Shared by test_ranges_niceonly.py (CPU) and test_gpu_ranges_niceonly.py
(GPU): the small range sets of the batched niceonly call and what it must
answer for them, built in Python from the oracle's primitives --
O.stride_residues enumerates the candidates of a range, O.scan_depth says
whether a candidate's square is repeat-free, O.is_nice whether it is listed.
"""
import bisect
import functools
import random

from oracle import oracle as O


def ndigits(v, base):
    n = 0
    while v:
        v //= base
        n += 1
    return n


def square_free(n, base):
    """The oracle's scan passed every digit of n^2: no repeat among them."""
    return O.scan_depth(n, base) > ndigits(n * n, base)


@functools.lru_cache(maxsize=None)
def table(base, k=2):
    return O.stride_residues(base, k)


def candidates(s, e, base, k=2):
    """The stride candidates of [s, e), ascending."""
    M, res = table(base, k)
    out = []
    c = s - s % M
    i = bisect.bisect_left(res, s % M)
    while True:
        if i == len(res):
            i, c = 0, c + M
            continue
        n = c + res[i]
        if n >= e:
            return out
        out.append(n)
        i += 1


def count_candidates(s, e, base, k=2):
    """... and their number by arithmetic alone."""
    M, res = table(base, k)
    idx = lambda x: x // M * len(res) + bisect.bisect_left(res, x % M)
    return idx(e) - idx(s)


@functools.lru_cache(maxsize=None)
def range_set(base, k=2):
    """Seeded ranges of 1 to 2e5 numbers with every edge the leaf arithmetic
    has: see the comments.  Returns a tuple of (start, end)."""
    M, res = table(base, k)
    R = len(res)
    assert R >= 2
    s, e = O.base_range(base)
    big = e - s >= 3 * 10 ** 6
    lo, hi = (s, e) if big else (1, 2 * 10 ** 6)  # b10, b12: ranges outside the tiny valid range too
    rng = random.Random(1000 + base)
    c = (lo + (hi - lo) // 3) // M * M + M  # a multiple of M well inside
    assert lo < c and c + 8 * M + 2 * 10 ** 5 < hi
    out = []
    # seeded sizes, 1 to 2e5 numbers
    for size in (1, 7, 250, 1000, 20_000, 200_000, rng.randrange(2, 50_000)):
        a = rng.randrange(lo, hi - size)
        out.append((a, a + size))
    # shorter than one stride gap: no candidate
    gap = next(i for i in range(R - 1) if res[i + 1] - res[i] >= 2)
    out.append((c + res[gap] + 1, c + res[gap + 1]))
    # one number, a candidate
    j = rng.randrange(R)
    out.append((c + res[j], c + res[j] + 1))
    # a start exactly on a candidate and an exclusive end exactly on one
    a = rng.randrange(R // 2)
    b = max(i for i in range(a + 1, R) if res[i] - res[a] <= 150_000)
    out.append((c + res[a], c + res[b]))
    # start mod M above the last residue: g0 = R (where the table's last residue is not M - 1)
    if res[-1] + 1 < M:
        out.append((c + res[-1] + 1, c + M + res[0] + 1))
    out.append((c + M - 1, c + M - 1 + min(2 * M, 150_000)))
    # across a multiple of M
    out.append((c + M - 5, c + M + 5))
    out.append((c + 4 * M - 1000, c + 4 * M + 1000))
    # across both ends of the valid range, and wholly outside it
    out.append((max(1, s - 500), s + 500))
    out.append((max(1, e - 1000), e + 1000))
    out.append((e + 10, e + 5000))
    if base == 10:
        out += [(47, 100), (10 ** 6, 10 ** 6 + 3000)]
    # overlapping and repeated ranges
    a0, e0 = out[5]
    out += [(a0 + (e0 - a0) // 2, e0 + 100), out[5], out[9], out[9]]
    if len(out) % 8 == 0:
        out.append((c + 5 * M, c + 5 * M + 100))
    assert all(1 <= e1 - s1 <= 2 * 10 ** 5 + 100 for s1, e1 in out)
    return tuple(out)


def expected_of(ranges, base, k=2):
    """(candidates, square_ok, [(n, range index)]) of the ranges."""
    cand, sq, lst = [], [], []
    for i, (s, e) in enumerate(ranges):
        ns = candidates(s, e, base, k)
        cand.append(len(ns))
        sq.append(sum(1 for n in ns if square_free(n, base)))
        lst += [(n, i) for n in ns if O.is_nice(n, base)]
    return cand, sq, lst


@functools.lru_cache(maxsize=None)
def expected(base, k=2):
    """expected_of(range_set(base, k)): computed once, shared, not modified."""
    return expected_of(range_set(base, k), base, k)


def in_range(rng_, base):
    s, e = O.base_range(base)
    return s <= rng_[0] and rng_[1] <= e
