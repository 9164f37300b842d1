"""The sound prefix test per caller range on the GPU
(nice_process_ranges_niceonly_ex with NICE_RANGES_PREFIX_ON: range_mask_kernel
and the prefix-testing variant of niceonly_ranges_kernel) against the Python
restatement of the rule (sound_restatement.py; per range:
ranges_prefix_cases.py), against the device-MSD sound field it composes to,
with non-empty lists under nice_debug_set_nice_min, across the leaf-piece
split, on two devices, and with the plain call left as it was.

Run on the MI355X box:  python -m pytest tests/test_gpu_ranges_prefix.py -m gpu -q
"""
import bisect
import ctypes

import pytest

import nice_amd as N
from nice_amd import _lib, api
from oracle import oracle as O

import nice_min_windows as W
import ranges_niceonly_cases as C
import ranges_prefix_cases as P
import sound_restatement as SR

pytestmark = pytest.mark.gpu

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


def launches(cand, fast):
    """Candidate launches of a one-device call: one per group that holds a candidate."""
    return sum(1 for g in (True, False) if sum(c for c, f in zip(cand, fast) if f == g))


def prefix_stats(c):
    st = c.ranges_niceonly_prefix_stats()
    return st.prefix_ranges, st.launches, st.rejected


# --- parity with the restatement ---------------------------------------------------------------------
@pytest.mark.parametrize("base", [40, 50, 57, 62, 65, 80])
def test_sound_leaves_of_a_window(ctx, base):
    """Two-word bases, 57 and 62 with n past 64 bits, 65 and 80 three-word."""
    leaves = P.window_leaves(base)
    cand, sq, rej = P.columns(leaves, base)
    got = ctx.niceonly_ranges_ex(leaves, base, prefix_test=True)
    print(base, len(leaves), sum(got[0]), sum(got[2]), sum(got[1]), (sum(cand), sum(rej), sum(sq)))
    assert got[0] == cand
    assert got[2] == rej
    assert got[1] == sq
    assert got[3] == []
    assert 0 < sum(rej) < sum(cand) and sum(sq) > 0
    if base in (57, 62):
        assert all(e >> 64 for _, e in leaves)
    assert prefix_stats(ctx) == (len(leaves), 1, sum(rej))
    st = ctx.ranges_niceonly_stats()
    assert (st.fast_ranges, st.generic_ranges, st.launches) == (len(leaves), 0, 1)
    assert (st.candidates, st.square_ok) == (sum(cand), sum(sq))
    assert 0 < ctx.ranges_niceonly_prefix_stats().mask_ms <= st.kernel_ms


@pytest.mark.parametrize("base", [40, 65])
def test_hand_made_ranges(ctx, base):
    ranges, kinds = P.hand_made(base)
    cand, sq, rej = P.check_kinds(base)
    assert ctx.niceonly_ranges_ex(ranges, base, prefix_test=True) == (cand, sq, rej, [])
    assert prefix_stats(ctx) == (len(ranges), 1, sum(rej))
    assert ctx.ranges_niceonly_stats().launches == 1


def test_fast_and_generic_ranges_in_one_call(ctx):
    """C.range_set(40) holds ranges inside, across and outside the valid range:
    the test runs on the first kind only, the others answer as the plain call."""
    ranges = C.range_set(40)
    cand, sq, lst = C.expected(40)
    fast = [C.in_range(r, 40) for r in ranges]
    inside = [r for r, f in zip(ranges, fast) if f]
    pc, psq, prej = P.columns(inside, 40)
    it = iter(zip(psq, prej))
    want_sq, want_rej = [], []
    for f in fast:
        q, r = next(it) if f else (0, 0)
        want_sq.append(q)
        want_rej.append(r)
    assert 0 < sum(fast) < len(fast) and sum(want_rej) > 0
    got = ctx.niceonly_ranges_ex(ranges, 40, prefix_test=True)
    assert got == (cand, want_sq, want_rej, lst)
    assert prefix_stats(ctx) == (sum(fast), 1, sum(want_rej))
    st = ctx.ranges_niceonly_stats()
    assert (st.fast_ranges, st.generic_ranges, st.launches) == (sum(fast), len(fast) - sum(fast), launches(cand, fast))


def test_where_the_test_does_not_run(ctx):
    for base in (10, 97):
        ranges = C.range_set(base)
        cand, _, lst = C.expected(base)
        assert ctx.niceonly_ranges_ex(ranges, base, prefix_test=True) == (cand, [0] * len(cand), [0] * len(cand), lst)
        assert prefix_stats(ctx) == (0, 0, 0)
    s, _ = O.base_range(40)
    r40 = [(s + 10 ** 9, s + 10 ** 9 + 50_000)]
    for k in (1, 3):
        cand, _, lst = C.expected_of(r40, 40, k)
        assert ctx.niceonly_ranges_ex(r40, 40, stride_k=k, prefix_test=True) == (cand, [0], [0], lst)
        assert prefix_stats(ctx) == (0, 0, 0) and ctx.ranges_niceonly_stats().fast_ranges == 0
    s, _ = O.base_range(43)
    assert ctx.niceonly_ranges_ex([(s, s + 10 ** 5)], 43, prefix_test=True) == ([0], [0], [0], [])
    assert ctx.ranges_niceonly_stats().launches == 0 and prefix_stats(ctx) == (0, 0, 0)
    with pytest.raises(_lib.NiceError) as err:
        ctx.niceonly_ranges_ex(r40, 40, prefix_test=2)
    assert err.value.code == _lib.NICE_ERR_INVALID


# --- the composed pipeline is the sound field ------------------------------------------------------
@pytest.mark.parametrize("base", [40, 57, 65])
def test_pipeline_identity_with_the_sound_field(ctx, base):
    a, size, chunk = W.window(base, "fused")
    bounds, _ = ctx.msd_ranges(api.chunk_roots(a, a + size, chunk), base, 250, "sound")
    cand, sq, rej, lst = ctx.niceonly_ranges_ex(bounds, base, prefix_test=True)
    composed = (len(bounds), sum(cand), sum(rej), sum(sq), [n for n, _ in lst])
    field_lst, st = ctx.niceonly_raw(a, a + size, base, chunk_size=chunk, msd_where="device", filter="sound")
    field = (st.ranges, st.candidates, st.prefix_rejected, st.square_ok, field_lst)
    want = SR.sound_field(a, size, base, chunk)
    print(base, composed[:4], field[:4], want[:4])
    assert composed == field
    assert composed == tuple(want)
    assert 0 < want[2] < want[1]
    # without the test the composition runs the square test on every candidate
    assert sum(ctx.niceonly_ranges(bounds, base)[1]) >= want[3]


# --- non-empty lists ----------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [40, 57, 65])
def test_lists_under_a_lowered_threshold(ctx, base):
    a, size, chunk = W.window(base, "fused")
    surv = W.sound_survivors(a, size, base, chunk)
    leaves = P.window_leaves(base)
    cand, sq, rej = P.columns(leaves, base)
    ts = W.thresholds(surv)
    picks = [ts[0], max(t for t in ts if len(W.listed(surv, t)) >= W.MIN_SURVIVORS)]
    assert picks[0] < picks[1]
    for t in picks:
        want = P.listed(leaves, base, t)
        assert [n for n, _ in want] == W.listed(surv, t) and len(want) >= W.MIN_SURVIVORS, "never [] against []"
        with W.lowered(base, t):
            got = ctx.niceonly_ranges_ex(leaves, base, prefix_test=True)
        assert got[3] == want, (base, t, len(got[3]), len(want))
        assert (got[0], got[1], got[2]) == (cand, sq, rej)
        starts = [s for s, _ in leaves]
        assert all(bisect.bisect_right(starts, n) - 1 == i for n, i in got[3])
    assert ctx.niceonly_ranges_ex(leaves, base, prefix_test=True)[3] == []


def test_capacity_retry_keeps_prefix_rejected(ctx):
    leaves = P.window_leaves(40)
    cand, sq, rej = P.columns(leaves, 40)
    want = P.listed(leaves, 40, 1)
    assert len(want) > 16
    L = _lib.lib()
    b, nr = api._pack_ranges(leaves)
    on = _lib.nice_ranges_niceonly_opts(0, _lib.NICE_RANGES_PREFIX_ON)
    n = ctypes.c_size_t()
    cb, sb, rb = (ctypes.c_uint64 * nr)(), (ctypes.c_uint32 * nr)(), (ctypes.c_uint64 * nr)()
    small, idx = (_lib.nice_number * 16)(), (ctypes.c_uint32 * 16)()
    with W.lowered(40, 1):
        assert L.nice_process_ranges_niceonly_ex(ctx._h, 40, b, nr, on, cb, sb, rb, small, idx, 16, n) == \
            _lib.NICE_ERR_CAPACITY
        assert n.value == len(want) and list(rb) == rej and list(sb) == sq
        before = (ctx.ranges_niceonly_stats(), ctx.ranges_niceonly_prefix_stats())
        rb2 = (ctypes.c_uint64 * nr)()
        big, bidx = (_lib.nice_number * n.value)(), (ctypes.c_uint32 * n.value)()
        _lib.check(L.nice_process_ranges_niceonly_ex(ctx._h, 40, b, nr, on, cb, sb, rb2, big, bidx, n.value, n))
    assert list(rb2) == rej and list(cb) == cand
    assert [(big[i].number_lo | big[i].number_hi << 64, bidx[i]) for i in range(n.value)] == want
    assert (ctx.ranges_niceonly_stats(), ctx.ranges_niceonly_prefix_stats()) == before, "the kept results"


# --- the piece split -----------------------------------------------------------------------------------
def test_a_range_of_more_than_one_leaf_piece(ctx):
    """The one b40 range of 4e9 numbers of test_gpu_ranges_niceonly.py: two leaf
    records, one mask.  prefix_rejected per residue class -- the range's P2 + P3
    against each residue's low digits, times the class's candidates in the
    range -- and square_ok against the CPU twin (Python cannot enumerate 2.9e8
    candidates), below the plain call's."""
    s, _ = O.base_range(40)
    size = 4 * 10 ** 9
    a = s + 3 * 10 ** 11
    total = C.count_candidates(a, a + size, 40)
    assert total > LEAF_PIECE
    M, res = C.table(40)
    assert len(res) == 4996
    pre = SR.leaf_prefix(a, a + size, 40)
    assert pre and not P.repeats(pre)
    want_rej = in_classes = 0
    for r in res:
        first = a + (r - a) % M  # the class's first member at or above a
        count = max(0, -(-(a + size - first) // M))
        in_classes += count
        if SR.rejected(pre, first, 40):
            want_rej += count
    assert in_classes == total and 0 < want_rej < total
    cand, sq, rej, lst = ctx.niceonly_ranges_ex([(a, a + size)], 40, prefix_test=True)
    print(total, want_rej, sq)
    assert (cand, rej, lst) == ([total], [want_rej], [])
    assert prefix_stats(ctx) == (1, 1, want_rej)
    cpu = api.niceonly_ranges_ex_cpu([(a, a + size)], 40, prefix_test=True, threads=16)
    assert cpu == (cand, sq, rej, lst)
    plain = ctx.niceonly_ranges([(a, a + size)], 40)
    assert 0 < sq[0] < plain[1][0]


# --- two devices ----------------------------------------------------------------------------------------
def test_two_devices_give_the_same_answers():
    two = N.GpuContext([0, 0])
    try:
        for base in (40, 65):
            ranges, _ = P.hand_made(base)
            cand, sq, rej = P.columns(ranges, base)
            assert two.niceonly_ranges_ex(ranges, base, prefix_test=True) == (cand, sq, rej, [])
            assert prefix_stats(two) == (len(ranges), 2, sum(rej)), "both devices made masks"
            assert two.ranges_niceonly_stats().launches == 2, "and both ran candidates"
        leaves = P.window_leaves(57)
        want = P.listed(leaves, 57, 1)
        with W.lowered(57, 1):
            got = two.niceonly_ranges_ex(leaves, 57, prefix_test=True)
        assert got[3] == want and len(want) >= W.MIN_SURVIVORS
        assert (got[0], got[1], got[2]) == P.columns(leaves, 57)
    finally:
        two.close()


# --- the plain call ---------------------------------------------------------------------------------
def test_existing_call_untouched_after_an_ex_call(ctx):
    ranges = C.range_set(40)
    cand, sq, lst = C.expected(40)
    fast = [C.in_range(r, 40) for r in ranges]
    want_sq = [q if f else 0 for q, f in zip(sq, fast)]
    assert sum(ctx.niceonly_ranges_ex(ranges, 40, prefix_test=True)[2]) > 0
    for call in (lambda: ctx.niceonly_ranges(ranges, 40), lambda: ctx.niceonly_ranges_ex(ranges, 40)[:2] +
                 ctx.niceonly_ranges_ex(ranges, 40)[3:]):
        assert call() == (cand, want_sq, lst)
        st = ctx.ranges_niceonly_stats()
        assert (st.fast_ranges, st.generic_ranges, st.launches) == (sum(fast), len(fast) - sum(fast), launches(cand, fast))
        assert (st.candidates, st.square_ok) == (sum(cand), sum(want_sq))
        assert prefix_stats(ctx) == (0, 0, 0) and ctx.ranges_niceonly_prefix_stats().mask_ms == 0
    assert ctx.niceonly_ranges_ex(ranges, 40)[2] == [0] * len(ranges)
