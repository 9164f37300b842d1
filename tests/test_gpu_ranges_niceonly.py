"""Batched niceonly ranges on the GPU (nice_process_ranges_niceonly,
niceonly_ranges_kernel): against the CPU test's Python expectations, with
non-empty in-range lists under nice_debug_set_nice_min, against the field path
on the b40 extra-large field, across the leaf-piece split, and beside fields
in flight.

Run on the MI355X box:  python -m pytest tests/test_gpu_ranges_niceonly.py -m gpu -q
"""
import bisect
import ctypes
import json
import os
import random

import pytest

import nice_amd as N
from nice_amd import _lib, api, dist, survey
from oracle import oracle as O

import nice_min_windows as W
import ranges_niceonly_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = W.THREADS
LEAF_PIECE = 1 << 28


@pytest.fixture(scope="module")
def ctx():
    c = N.GpuContext(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _restore():
    """The oracle's Filter C switch and the hook are process-global."""
    yield
    O.lib().oracle_set_filter_c(1)
    for b in W.FAST:
        _lib.lib().nice_debug_set_nice_min(b, 0)


def gpu_expected(base):
    """The CPU test's expectation as the GPU reports it: square_ok only where
    the compile-time kernel runs (a fast base's ranges inside its valid range)."""
    ranges = C.range_set(base)
    cand, sq, lst = C.expected(base)
    fast = [N.niceonly_fast_base(base) and C.in_range(r, base) for r in ranges]
    return ranges, cand, [q if f else 0 for q, f in zip(sq, fast)], lst, fast


# --- the CPU test's range sets ---------------------------------------------------------------------
@pytest.mark.parametrize("base", [10, 40, 45, 50, 57, 62, 65, 80, 97])
def test_matches_the_cpu_expectations(ctx, base):
    """10 and 97: the run-time-base kernel alone; 40..50 two-word bases, 57 and
    62 with n past 64 bits, 65 and 80 three-word; every fast base's set mixes
    in-range ranges with ranges across and outside the valid range, so both
    kernels run in one call."""
    ranges, cand, sq, lst, fast = gpu_expected(base)
    got = ctx.niceonly_ranges(ranges, base)
    assert got[0] == cand
    assert got[1] == sq
    assert got[2] == lst
    st = ctx.ranges_niceonly_stats()
    assert (st.fast_ranges, st.generic_ranges) == (sum(fast), len(fast) - sum(fast))
    assert (st.candidates, st.square_ok) == (sum(cand), sum(sq))
    assert st.launches == (1 if sum(fast) else 0) + (1 if sum(c for c, f in zip(cand, fast) if not f) else 0)
    if N.niceonly_fast_base(base):
        assert 0 < sum(fast) < len(fast) and (sum(sq) > 0 or base == 62), "mixed groups, and something counted"
    if base in (57, 62):
        assert any(e >> 64 for (_, e), f in zip(ranges, fast) if f)
    rs = N.process_ranges_niceonly_gpu(ctx, ranges, base)
    assert [[x.number for x in r.nice_numbers] for r in rs] == [[n for n, i in lst if i == j]
                                                               for j in range(len(ranges))]


def test_b10_and_other_stride_depths(ctx):
    assert ctx.niceonly_ranges([(47, 100), (60, 70)], 10)[2] == [(69, 0), (69, 1)]
    s, e = O.base_range(12)
    ranges = [(1, 3000), (s, e), (10 ** 5, 10 ** 5 + 40_000), (7, 8)]
    for k in (1, 3):
        cand, _, lst = C.expected_of(ranges, 12, k)
        got = ctx.niceonly_ranges(ranges, 12, stride_k=k)
        assert (got[0], got[2]) == (cand, lst) and lst
    # k = 3 on a fast base inside its range: the run-time-base kernel, nothing counted
    s, _ = O.base_range(40)
    r40 = [(s + 10 ** 9, s + 10 ** 9 + 50_000)]
    cand, _, lst = C.expected_of(r40, 40, 3)
    assert ctx.niceonly_ranges(r40, 40, stride_k=3) == (cand, [0], lst)
    assert ctx.ranges_niceonly_stats().fast_ranges == 0
    # a residue-empty base: zeros, no launch
    s, _ = O.base_range(43)
    assert ctx.niceonly_ranges([(s, s + 10 ** 5), (1, 1000)], 43) == ([0, 0], [0, 0], [])
    assert ctx.ranges_niceonly_stats().launches == 0


def test_invalid_arguments_on_the_gpu_entry_point(ctx):
    L = _lib.lib()

    def call(base, ranges, k=0, n_ranges=None):
        flat = [x for s, e in ranges for x in (s & C_MASK, s >> 64, e & C_MASK, e >> 64)]
        b = (ctypes.c_uint64 * max(4, len(flat)))(*flat)
        n = ctypes.c_size_t()
        return L.nice_process_ranges_niceonly(ctx._h, base, b, len(ranges) if n_ranges is None else n_ranges, k,
                                              None, None, None, None, 0, n)

    INV = _lib.NICE_ERR_INVALID
    assert call(10, [(47, 60)]) == _lib.NICE_OK
    assert call(10, [(47, 60)], n_ranges=0) == INV and call(10, [(47, 60)], n_ranges=(1 << 20) + 1) == INV
    assert call(10, [(47, 60), (9, 9)]) == INV and b"range 1" in L.nice_last_error()
    assert call(10, [(47, 60), (1, 1 << 60)]) == INV and b"2^40" in L.nice_last_error()
    assert call(97, [(1, 1000)], k=4) == INV and b"modulus" in L.nice_last_error()
    assert call(1, [(47, 60)]) == INV and call(129, [(47, 60)]) == INV


C_MASK = (1 << 64) - 1


# --- non-empty in-range lists ---------------------------------------------------------------------
def cut(a, size, pieces, seed):
    """[a, a + size) in `pieces` ranges of uneven size."""
    rng = random.Random(seed)
    cuts = sorted(rng.sample(range(1, size), pieces - 1))
    edges = [a] + [a + c for c in cuts] + [a + size]
    return list(zip(edges, edges[1:]))


def all_survivors(a, size, base):
    """[(n, union count)] of every stride candidate of [a, a + size) with a
    repeat-free square, by the oracle: with the floor at the field size its MSD
    recursion emits the field untested."""
    O.lib().oracle_set_filter_c(1)
    chunk = -(-size // THREADS)
    res, cands, ranges, sq = O.process_field_niceonly_sq(a, a + size, base, THREADS, chunk, chunk, nice_min=1)
    assert len(res.nice_numbers) == sq and cands == C.count_candidates(a, a + size, base)
    return res.nice_numbers


def attribute(surv, ranges, t):
    """What the call must list at threshold t, and every range's square_ok."""
    starts = [s for s, _ in ranges]
    lst, sq = [], [0] * len(ranges)
    for n, u in surv:
        i = bisect.bisect_right(starts, n) - 1
        assert ranges[i][0] <= n < ranges[i][1]
        sq[i] += 1
        if u >= t:
            lst.append((n, i))
    return lst, sq


@pytest.mark.parametrize("base", [40, 57, 65])
def test_in_range_lists_under_a_lowered_threshold(ctx, base):
    a, size, _ = W.window(base, "fused")
    surv = all_survivors(a, size, base)
    ranges = cut(a, size, 300, base)
    ts = W.thresholds(surv)
    # the lowest threshold (every survivor) and the highest that still lists MIN_SURVIVORS
    picks = [ts[0], max(t for t in ts if len(W.listed(surv, t)) >= W.MIN_SURVIVORS)]
    assert picks[0] < picks[1]
    for t in picks:
        want, sq = attribute(surv, ranges, t)
        assert len(want) >= W.MIN_SURVIVORS, "never [] against []"
        assert len(want) == len(surv) or t != ts[0]
        if base >= 57:
            assert all(n >> 64 for n, _ in want)
        with W.lowered(base, t):
            got = ctx.niceonly_ranges(ranges, base)
        assert got[2] == want, (base, t, len(got[2]), len(want))
        assert got[1] == sq and got[0] == [C.count_candidates(s, e, base) for s, e in ranges]
        assert t != ts[0] or len({i for _, i in want}) > 20, "entries in many ranges"
    # production again once the hook is cleared
    assert ctx.niceonly_ranges(ranges, base)[2] == []


# --- parity with the field path -----------------------------------------------------------------------
def extra_large():
    with open(os.path.join(ROOT, "tests", "golden", "oracle_fields.json")) as fh:
        return next(c for c in json.load(fh)["niceonly"] if c["name"] == "b40_extra_large_1e9")


def client_ranges(a, e, base):
    """The client's chunks of the field, each through nice_msd_valid_ranges at
    floor 250: the ranges a host MSD producer would hand over."""
    chunk = dist.client_chunk_size(e - a)
    chunks = [N.FieldSize(s, min(e, s + chunk)) for s in range(a, e, chunk)]
    return chunks, [(r.range_start, r.range_end) for c in chunks for r in api.get_valid_ranges(c, base, 250)]


def test_parity_with_the_field_path_on_the_extra_large_field(ctx):
    fx = extra_large()
    a, e = int(fx["start"]), int(fx["end"])
    chunks, ranges = client_ranges(a, e, 40)
    assert len(chunks) == 1000
    cand, sq, lst = ctx.niceonly_ranges(ranges, 40)
    st = ctx.ranges_niceonly_stats()
    assert sum(cand) == fx["candidates"] == 1_389_117 == st.candidates
    assert [n for n, _ in lst] == [int(n) for n in fx["nice_numbers"]]
    field_lst, fst = ctx.niceonly_raw(a, e, 40, msd_where="host")
    assert (fst.ranges, fst.candidates) == (len(ranges), sum(cand)) and field_lst == [n for n, _ in lst]
    assert sum(sq) == O.process_field_niceonly_sq(a, e, 40, THREADS)[3] == st.square_ok
    assert (st.fast_ranges, st.generic_ranges, st.launches) == (len(ranges), 0, 1)


# --- the piece split -----------------------------------------------------------------------------------
def test_a_range_of_more_than_one_leaf_piece(ctx):
    """One b40 range of 4e9 numbers: > 2^28 candidates, so two leaves.  The
    oracle's figure is process_field_niceonly_sq's with the floor at the chunk
    size, where its recursion emits every chunk untested -- the count of
    (chunk = size, floor = size), summed over THREADS chunks instead of one so
    that the CPU side takes seconds, not a minute."""
    s, _ = O.base_range(40)
    size = 4 * 10 ** 9
    a = s + 3 * 10 ** 11
    assert not O.has_duplicate_msd_prefix(a, a + size, 40)
    total = C.count_candidates(a, a + size, 40)
    assert total > LEAF_PIECE
    chunk = -(-size // THREADS)
    _, cands, _, sq_want = O.process_field_niceonly_sq(a, a + size, 40, THREADS, chunk, chunk)
    assert cands == total
    cand, sq, lst = ctx.niceonly_ranges([(a, a + size)], 40)
    assert cand == [total] and sq == [sq_want] and lst == []


# --- list overflow ---------------------------------------------------------------------------------------
def test_list_overflow_keeps_the_results(ctx):
    a, size, _ = W.window(40, "fused")
    surv = all_survivors(a, size, 40)
    ranges = cut(a, size, 37, 5)
    want, sq = attribute(surv, ranges, 1)
    assert len(want) > 64
    L = _lib.lib()
    bounds, nr = api._pack_ranges(ranges)
    n = ctypes.c_size_t()
    cand = (ctypes.c_uint64 * nr)()
    sqb = (ctypes.c_uint32 * nr)()
    small, idx = (_lib.nice_number * 16)(), (ctypes.c_uint32 * 16)()
    with W.lowered(40, 1):
        assert L.nice_process_ranges_niceonly(ctx._h, 40, bounds, nr, 0, cand, sqb, small, idx, 16, n) == \
            _lib.NICE_ERR_CAPACITY
        assert n.value == len(want) and list(sqb) == sq
        before = ctx.ranges_niceonly_stats()
        assert before.launches == 1
        big, bidx = (_lib.nice_number * n.value)(), (ctypes.c_uint32 * n.value)()
        _lib.check(L.nice_process_ranges_niceonly(ctx._h, 40, bounds, nr, 0, cand, sqb, big, bidx, n.value, n))
    assert [(big[i].number_lo | big[i].number_hi << 64, bidx[i]) for i in range(n.value)] == want
    assert all(big[i].num_uniques == 40 for i in range(n.value))
    assert ctx.ranges_niceonly_stats() == before, "the kept results, not a second run"
    # a device list of 4096 entries at first: a longer list grows it and runs the share again
    c2 = N.GpuContext(0)
    try:
        whole = cut(a, size, 3, 9)
        want2, _ = attribute(surv, whole, 1)
        if len(want2) > 4096:
            with W.lowered(40, 1):
                assert c2.niceonly_ranges(whole, 40, cap=len(want2))[2] == want2
    finally:
        c2.close()


def test_leaf_staging_regrows_between_calls(ctx):
    """One context, three calls: 1 range, then 5000 ranges of 10^4 numbers --
    more leaf records than the leaf staging's first size (4096), so the pinned
    and device buffers are replaced -- then 1 range again, each against the CPU
    twin (all in range on the k = 2 table: square_ok counted on both sides)."""
    s, e = O.base_range(40)
    rng = random.Random(12)
    big = [(a, a + 10 ** 4) for a in sorted(rng.sample(range(s, e - 10 ** 5, 10 ** 5), 5000))]
    leaves = ctypes.c_size_t()
    _lib.check(_lib.lib().nice_debug_ranges_niceonly_plan(40, 0, api._pack_ranges(big)[0], len(big), 1, None, 0,
                                                          leaves))
    assert leaves.value > 4096
    for ranges in ([big[0]], big, [big[-1]]):
        assert ctx.niceonly_ranges(ranges, 40) == N.niceonly_ranges_cpu(ranges, 40, threads=THREADS)
        assert ctx.ranges_niceonly_stats().generic_ranges == 0


# --- beside fields in flight --------------------------------------------------------------------------
def test_independent_of_fields_in_flight(ctx):
    s, _ = O.base_range(40)
    fields = [(s + k * 10 ** 9, s + k * 10 ** 9 + 10 ** 8) for k in (1, 2, 3)]
    alone = [ctx.niceonly_raw(a, e, 40) for a, e in fields]
    ranges, cand, sq, lst, _ = gpu_expected(40)
    tickets = [ctx.niceonly_submit(a, e, 40) for a, e in fields]
    # every niceonly slot is taken: the batched call needs none
    assert ctx.niceonly_ranges(ranges, 40) == (cand, sq, lst)
    for t, (want_lst, want_st) in zip(tickets, alone):
        got_lst, got_st = ctx.niceonly_collect(t)
        assert got_lst == want_lst
        assert (got_st.ranges, got_st.candidates, got_st.square_ok) == \
            (want_st.ranges, want_st.candidates, want_st.square_ok)


# --- two devices ----------------------------------------------------------------------------------------
def test_two_devices_give_the_same_answers():
    two = N.GpuContext([0, 0])
    try:
        for base in (40, 97):
            ranges, cand, sq, lst, fast = gpu_expected(base)
            assert two.niceonly_ranges(ranges, base) == (cand, sq, lst)
            st = two.ranges_niceonly_stats()
            assert st.launches > (2 if base == 40 else 1), "both devices ran"
        a, size, _ = W.window(57, "fused")
        surv = all_survivors(a, size, 57)
        ranges = cut(a, size, 300, 57)
        want, sq = attribute(surv, ranges, 1)
        with W.lowered(57, 1):
            got = two.niceonly_ranges(ranges, 57)
        assert got[2] == want and got[1] == sq and len(want) >= W.MIN_SURVIVORS
        assert two.ranges_niceonly_stats().launches == 2
    finally:
        two.close()


# --- the survey ------------------------------------------------------------------------------------------
def test_survey_equals_the_cpu_twin(ctx):
    kw = dict(windows=64, seed=1, threads=THREADS)
    gpu = survey.survey_niceonly_base(ctx, 40, **kw)
    cpu = survey.survey_niceonly_base(None, 40, **kw)
    assert gpu == cpu
    assert gpu.sound.candidates > gpu.reference.candidates > 0 and gpu.reference.square_ok > 0
