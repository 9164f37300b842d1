"""Shared by test_ranges_prefix.py (CPU) and test_gpu_ranges_prefix.py (GPU):
the range sets of the batched niceonly call with the prefix test on
(nice_process_ranges_niceonly_ex) and what it must answer for them, by the
Python-integer restatement of the rule (sound_restatement.py leaf_prefix /
rejected) applied per range -- never by the library.

Every set lies inside a fast base's valid range, where the test runs.
"""
import functools
import random

from oracle import oracle as O

import nice_min_windows as W
import sound_restatement as SR

BASES = W.BASES  # every fast base but 64, which has no candidate


def cut(a, size, pieces, seed):
    """[a, a + size) in `pieces` ranges of uneven size."""
    rng = random.Random(seed)
    cuts = sorted(rng.sample(range(1, size), pieces - 1))
    edges = [a] + [a + c for c in cuts] + [a + size]
    return list(zip(edges, edges[1:]))


@functools.lru_cache(maxsize=None)
def expected(ranges, base):
    """Per range of the tuple `ranges`: (candidates, prefix_rejected, square_ok
    of the kept, ((n, union count) of the kept square survivors)).  Computed
    once per set, shared, not modified."""
    out = []
    for s, e in ranges:
        pre = SR.leaf_prefix(s, e, base)
        ns = SR.candidates(s, e, base)
        kept = [n for n in ns if not SR.rejected(pre, n, base)]
        surv = tuple((n, SR.union_count(n, base)) for n in kept if SR.square_repeat_free(n, base))
        out.append((len(ns), len(ns) - len(kept), len(surv), surv))
    return tuple(out)


def columns(ranges, base):
    """(candidates, square_ok, prefix_rejected) lists, as the call returns them."""
    ex = expected(tuple(ranges), base)
    return [x[0] for x in ex], [x[2] for x in ex], [x[1] for x in ex]


def listed(ranges, base, nice_min):
    """[(n, range index)] the call lists with the hook at nice_min."""
    return [(n, i) for i, x in enumerate(expected(tuple(ranges), base)) for n, u in x[3] if u >= nice_min]


@functools.lru_cache(maxsize=None)
def window_leaves(base):
    """The sound recursion's leaves (Filter C off, floor 250) of the base's
    "fused" window, by the oracle."""
    a, size, chunk = W.window(base, "fused")
    try:
        return tuple(SR.oracle_ranges(a, a + size, base, 250, False, chunk))
    finally:
        O.lib().oracle_set_filter_c(1)


def repeats(prefix):
    return prefix is not None and len(set(prefix)) != len(prefix)


@functools.lru_cache(maxsize=None)
def hand_made(base):
    """Ranges an MSD recursion never hands over, of the base's "fused" window:
    its 300 uneven pieces; one-number ranges on a stride candidate; two- and
    three-number ranges around a candidate whose P2 + P3 repeats; the window
    as one range.  Returns (ranges, kinds) with kinds[i] in "piece", "one",
    "dup", "whole"."""
    a, size, _ = W.window(base, "fused")
    rng = random.Random(4000 + base)
    ranges = cut(a, size, 300, base)
    kinds = ["piece"] * len(ranges)
    cands = SR.candidates(a + 10, a + size - 10, base)
    for n in rng.sample(cands, 6):
        ranges.append((n, n + 1))
        kinds.append("one")
    dups = 0
    for n in rng.sample(cands, 40):
        for r in ((n, n + 2), (n - 1, n + 2), (n - 1, n + 1)):
            if repeats(SR.leaf_prefix(*r, base)) and dups < 9:
                ranges.append(r)
                kinds.append("dup")
                dups += 1
    ranges.append((a, a + size))
    kinds.append("whole")
    return tuple(ranges), tuple(kinds)


def check_kinds(base):
    """No comparison of the hand-made set is 0 against 0: every kind holds a
    range with candidates, behaving as its kind says.  Returns the columns."""
    ranges, kinds = hand_made(base)
    cand, sq, rej = columns(ranges, base)
    by = lambda k: [i for i, x in enumerate(kinds) if x == k]
    assert all(cand[i] == 1 and rej[i] == 0 for i in by("one")) and len(by("one")) == 6
    assert len(by("dup")) == 9 and all(cand[i] >= 1 and rej[i] == cand[i] and sq[i] == 0 for i in by("dup"))
    assert {ranges[i][1] - ranges[i][0] for i in by("dup")} == {2, 3}
    (w,) = by("whole")
    assert 0 < rej[w] < cand[w] and sq[w] > 0
    # the whole window's prefix is shorter than its pieces': it rejects fewer
    pieces = by("piece")
    assert len(pieces) == 300 and sum(cand[i] for i in pieces) == cand[w]
    assert rej[w] < sum(rej[i] for i in pieces) < cand[w]
    return cand, sq, rej
