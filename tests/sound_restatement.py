"""Python-integer restatement of the sound niceonly filter's per-candidate
prefix test (include/nice_hip.h NICE_FILTER_SOUND), shared by
test_sound_filter.py and test_gpu_sound_filter.py.

A leaf is [a, e), first = a, last = e - 1.  P2 is the common leading base-b
digits of first^2 and last^2 (empty when their digit counts differ), P3 the
same for the cubes.  For a candidate n of the leaf, L is the two lowest digits
of n^2 and the two lowest digits of n^3.  n is rejected iff the list
P2 + P3 + L contains a repeated value.  A leaf of one number rejects nothing.

Every function that asks the oracle for Filter-C-free ranges switches
oracle_set_filter_c(0); the test files restore 1 in a fixture finaliser.
"""
import bisect
import functools

from oracle import oracle as O


def digits(x, base):
    """Base-b digits of x, most significant first."""
    d = []
    while x:
        d.append(x % base)
        x //= base
    return d[::-1]


def common_prefix(x, y):
    if len(x) != len(y):
        return []
    out = []
    for p, q in zip(x, y):
        if p != q:
            break
        out.append(p)
    return out


def leaf_prefix(a, e, base):
    """P2 + P3 of the leaf [a, e), or None for a leaf of one number."""
    if e - a == 1:
        return None
    f, l = a, e - 1
    return (common_prefix(digits(f * f, base), digits(l * l, base)) +
            common_prefix(digits(f ** 3, base), digits(l ** 3, base)))


def rejected(prefix, n, base):
    if prefix is None:
        return False
    sq, cu = n * n, n ** 3
    lst = prefix + [sq % base, sq // base % base, cu % base, cu // base % base]
    return len(set(lst)) != len(lst)


def square_repeat_free(n, base):
    d = digits(n * n, base)
    return len(set(d)) == len(d)


@functools.lru_cache(maxsize=None)
def stride(base):
    return O.stride_residues(base, 2)


def candidates(a, e, base):
    """The k = 2 stride candidates of [a, e), ascending."""
    M, res = stride(base)
    c, i = divmod(a, M)
    i = bisect.bisect_left(res, i)
    out = []
    while True:
        if i == len(res):
            i = 0
            c += 1
        n = c * M + res[i]
        if n >= e:
            return out
        out.append(n)
        i += 1


def oracle_ranges(a, e, base, floor, filter_c, chunk=0):
    """The oracle's MSD-surviving ranges of [a, e), recursed per chunk, with
    Filter C on (the reference) or off (the sound filter's recursion)."""
    O.lib().oracle_set_filter_c(1 if filter_c else 0)
    chunk = chunk or (e - a)
    out = []
    for cs in range(a, e, chunk):
        out += O.valid_ranges(cs, min(e, cs + chunk), base, floor)
    return out


def union_count(n, base):
    """Members of the digit union of n^2 and n^3."""
    return len(set(digits(n * n, base)) | set(digits(n ** 3, base)))


@functools.lru_cache(maxsize=None)
def _sound_core(a, size, base, chunk, floor):
    """(ranges, candidates, prefix_rejected, the kept candidates whose square
    is repeat-free, the oracle's nice list) of the sound field [a, a + size)."""
    leaves = oracle_ranges(a, a + size, base, floor, False, chunk)
    res, cands, ranges, _ = O.process_field_niceonly_sq(a, a + size, base, 16, chunk, floor)
    n_cand = n_rej = 0
    kept = []
    for s, e in leaves:
        pre = leaf_prefix(s, e, base)
        for n in candidates(s, e, base):
            n_cand += 1
            if rejected(pre, n, base):
                n_rej += 1
            elif square_repeat_free(n, base):
                kept.append(n)
    assert (len(leaves), n_cand) == (ranges, cands)
    return ranges, cands, n_rej, tuple(kept), [n for n, _ in res.nice_numbers]


def sound_field(a, size, base, chunk, floor=250, nice_min=0):
    """What a sound niceonly field of [a, a + size) must report: (ranges,
    candidates, prefix_rejected, square_ok, nice list).  Ranges, candidates and
    the list are the oracle's with Filter C off; the rejected and square counts
    come from the restatement above.

    nice_min (nice_debug_set_nice_min's threshold; 0: production): the list
    holds instead every candidate the prefix test keeps whose square is
    repeat-free and whose union_count is >= nice_min, by the restatement."""
    ranges, cands, n_rej, kept, nice = _sound_core(a, size, base, chunk, floor)
    if nice_min:
        nice = sorted(n for n in kept if union_count(n, base) >= nice_min)
    return ranges, cands, n_rej, len(kept), list(nice)
