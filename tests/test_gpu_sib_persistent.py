"""The persistent grid of the b40 sibling-lane FD kernel (Cfg::SIBPERS).

One round of resident workgroups; workgroup g walks the strided 64-unit
batches g, g + G, ... of a launch's sibling and edge units, its waves pulling
them from an LDS counter and stopping after wave_cap batches.  Forced on with
nice_debug_force_sib_persistent(1, max_workgroups) so that small fields reach
it, with the near-miss cutoff lowered (nice_debug_set_near_miss_cutoff) so the
list -- whose n is rebuilt from the wave's batch index -- is not empty.

Run on the MI355X box:  python -m pytest tests/test_gpu_sib_persistent.py -m gpu -q -rA
"""
import contextlib
import functools

import pytest

import nice_amd as N
from nice_amd import _lib
from oracle import oracle as O

import near_miss_windows as W

pytestmark = pytest.mark.gpu

BASE, M = 40, 3
D = BASE ** 4          # B^2: one sibling's block
SB = M * D             # a super-block
# plan_sib_pers: a segment takes the persistent grid in production at or above
# this many wave batches per resident wave (PlanKnobs::sib_pers_min / 10)
PERS_MIN_TENTHS = 40
WAVES = 8              # per 512-thread workgroup


@pytest.fixture(scope="module")
def ctx():
    c = N.GpuContext(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def want(a, e, cutoff=None):
    return W.oracle(a, e, BASE, cutoff)


@contextlib.contextmanager
def forced(mode, max_wg=0, stride=0):
    lib = _lib.lib()
    assert lib.nice_debug_force_sib_persistent(mode, max_wg) == _lib.NICE_OK
    assert lib.nice_debug_force_sib_stride(stride) == _lib.NICE_OK
    try:
        yield
    finally:
        assert lib.nice_debug_force_sib_persistent(0, 0) == _lib.NICE_OK
        assert lib.nice_debug_force_sib_stride(0) == _lib.NICE_OK


def same(got, exp, cutoff, what, at_least=100):
    (h, lst), (hw, lw) = got, exp
    assert len(lw) >= at_least, f"{what}: the expected list has {len(lw)} entries"
    assert h == hw, f"{what}: histogram"
    assert lst == lw, f"{what}: list ({len(lst)} entries, expected {len(lw)})"
    assert len(lst) == sum(h[cutoff + 1:]), f"{what}: list length against the bins above the cutoff"
    print(f"near-miss entries, {what}: {len(lst)}")


def batches(q, L):
    """Wave batches of q super-blocks at lane stride L (plan_sib_launch)."""
    u = -(-D // L)
    upb = u - 1 if D % L else u
    return -(-q * upb // 64) + (-(-q // 64) if D % L else 0)


@functools.lru_cache(maxsize=None)
def field0():
    """4 super-blocks and a ragged remainder at the start of b40's range (the
    ND = 4 limb layout, the pipelined walk), placed so that a listed number
    sits 5 before the end of sibling 1's block of super-block 0: inside the
    edge unit of every lane stride L with B^2 mod L >= 5."""
    c = W.low_cutoff(BASE)
    x = O.base_range(BASE)[0] + 777 + 2 * D
    while True:  # the first listed number from there on
        lst = want(x, x + 500_000, c)[1]
        if lst:
            break
        x += 500_000
    return lst[0][0] - 2 * D + 5, 4 * SB + 1_234_567


def test_hook_rejects_other_modes():
    assert _lib.lib().nice_debug_force_sib_persistent(3, 0) == _lib.NICE_ERR_INVALID
    assert _lib.lib().nice_debug_force_sib_persistent(0, 0) == _lib.NICE_OK


# --- 1. small forced-persistent fields -------------------------------------------------------
@pytest.mark.parametrize("max_wg", [1, 3, 64])
def test_small_forced_persistent(ctx, max_wg):
    """Grids of 1, 3 and 64 workgroups, lane strides with (105, 143, 209) and
    without (125) edge units: histogram and list against the oracle, bit for bit."""
    s, n = field0()
    with W.lowered(BASE) as c:
        exp = want(s, s + n, c)
        inside = [x - s for x, _ in exp[1] if x - s < 4 * SB]
        assert any((o // D) % M >= 1 for o in inside), "no expected entry from a sibling j >= 1"
        for L in (105, 125, 143, 209):
            assert (D % L == 0) == (L == 125)
            if D % L:
                assert any(o % D >= D // L * L for o in inside), f"L {L}: no expected entry in an edge unit"
            with forced(1, max_wg, L):
                got = ctx.detailed_raw(s, s + n, BASE)
                st = ctx.kernel_stats()
            assert (st.sib_lanes, st.sib_stride, st.launches) == (M, L, 1), st
            assert 0 < st.sib_grid <= max_wg, st
            same(got, exp, c, f"persistent grid of {st.sib_grid}, L {L}")


# --- 2. the waves' caps do not cover the batches: the segment splits ---------------------------
def test_cap_overflow_splits_the_launch(ctx):
    """8 super-blocks at L = 143 on ONE workgroup: 2 239 batches, 280 per wave
    against wave_cap = 65535 / (3 * 143) = 152, so at least two launches; the
    result must equal the rounds kernel's."""
    L = 143
    assert batches(8, L) == 2239 and 65535 // (M * L) == 152
    s = O.base_range(BASE)[0] + 777
    n = 8 * SB + 54_321
    with W.lowered(BASE) as c:
        with forced(2, 0, L):
            exp = ctx.detailed_raw(s, s + n, BASE)
            assert ctx.kernel_stats().sib_grid == 0 and ctx.kernel_stats().sib_lanes == M
        with forced(1, 1, L):
            got = ctx.detailed_raw(s, s + n, BASE)
            st = ctx.kernel_stats()
        assert st.sib_grid == 1 and st.launches >= 2 and st.sib_stride == L, st
        assert sum(got[0]) == n
        same(got, exp, c, f"cap overflow, {st.launches} launches")


# --- 3. a field across the first limb-layout cut -----------------------------------------------
def test_layout_cut(ctx):
    """4 super-blocks and a remainder on the ND = 4 side of b40's first cut
    (persistent grid), 1.5e6 numbers beyond it (another kernel, which carries
    the field's finish): against the oracle."""
    cut = W.cuts_of(BASE)[0]
    s, e = cut - (4 * SB + 345_678), cut + 1_500_000
    assert s >= O.base_range(BASE)[0]
    with W.lowered(BASE) as c:
        exp = want(s, e, c)
        # (just beyond the cut nothing is listed: that side is pinned by the histogram)
        assert any(x < cut for x, _ in exp[1]) and sum(exp[0]) == e - s
        with forced(1, 64, 143):
            got = ctx.detailed_raw(s, e, BASE)
            st = ctx.kernel_stats()
        assert st.sib_grid > 0 and st.launches == 2, st
        same(got, exp, c, "across the first layout cut")


# --- 4. three fields in flight -----------------------------------------------------------------
def test_three_fields_in_flight(ctx):
    """Three forced-persistent fields submitted before the first is collected
    (state re-zero and arrival counting with the persistent grid): the field of
    test 1 at three grid sizes, each against the oracle."""
    s, n = field0()
    with W.lowered(BASE) as c:
        exp = want(s, s + n, c)
        tickets = []
        try:
            for max_wg in (3, 64, 0):
                assert _lib.lib().nice_debug_force_sib_persistent(1, max_wg) == _lib.NICE_OK
                tickets.append(ctx.detailed_submit(s, s + n, BASE))
            for t in tickets:
                same(ctx.detailed_collect(t, BASE), exp, c, "in flight")
                assert ctx.kernel_stats().sib_grid > 0
        finally:
            assert _lib.lib().nice_debug_force_sib_persistent(0, 0) == _lib.NICE_OK


# --- 5. what production picks ----------------------------------------------------------------------
def test_production_selection(ctx):
    """Mode 0 at a pinned stride, fields submitted while another is
    uncollected (the pipelined case; a lone field keeps rounds): the smallest
    field whose batches reach PERS_MIN_TENTHS / 10 per resident wave runs
    persistent, one super-block less runs rounds; the field above equals
    itself in rounds (mode 2, the kernel the existing tests pin)."""
    L = 143
    s = O.base_range(BASE)[0]

    def pipelined(n):
        """[s, s + n) submitted while another field is uncollected: its results and stats."""
        first = ctx.detailed_submit(s, s + 1_000_000, BASE)
        t = ctx.detailed_submit(s, s + n, BASE)
        ctx.detailed_collect(first, BASE)
        got = ctx.detailed_collect(t, BASE)
        return got, ctx.kernel_stats()

    with forced(0, 0, L):
        _, st = pipelined(10 ** 9)
        assert st.sib_grid > 0 and st.sib_stride == L, st
        resident_waves = WAVES * st.sib_grid  # one round of resident workgroups
        # a lone field keeps rounds of workgroups
        ctx.detailed_raw(s, s + 10 ** 9, BASE)
        lone = ctx.kernel_stats()
        assert lone.sib_grid == 0 and lone.sib_lanes == M, lone
        q = 4
        while 10 * batches(q, L) < PERS_MIN_TENTHS * resident_waves:
            q += 1
        assert q > 5
        above, sa = pipelined(q * SB + 99_999)
        below, sb = pipelined((q - 1) * SB + 99_999)
    assert sa.sib_grid == resident_waves // WAVES and sa.sib_lanes == M and sa.launches == 1, sa
    assert sb.sib_grid == 0 and sb.sib_lanes == M, sb
    assert sum(below[0]) == (q - 1) * SB + 99_999
    with forced(2, 0, L):
        rounds = ctx.detailed_raw(s, s + q * SB + 99_999, BASE)
        assert ctx.kernel_stats().sib_grid == 0
    assert above == rounds and sum(above[0]) == q * SB + 99_999
