"""The device MSD recursion's range list (nice_msd_ranges; msd_ranges_fused_kernel
and msd_ranges_level_kernel): range by range against the CPU twin under both
filters and against the oracle under the reference filter -- the split rule's
edges, every arithmetic path of classify_node, the depth cap in the level form,
empty answers, one mixed call of both forms, the round trip with the production
field path, the capacity retry, two devices and the survey's device placement.

Run on the MI355X box:  python -m pytest tests/test_gpu_msd_ranges.py -m gpu -q
"""
import ctypes
import functools

import pytest

import nice_amd as N
from nice_amd import _lib, api, survey
from oracle import oracle as O

pytestmark = pytest.mark.gpu

MASK = (1 << 64) - 1
THREADS = 16
A40 = 4_234_942_132_458
A50 = 94_760_515_586_064_977
EMPTY40 = 1_916_284_264_916  # the b40 range start: nothing survives near it
BIG = (1 << 23) + 3
FILTERS = ("reference", "sound")


@pytest.fixture(scope="module")
def ctx():
    c = N.GpuContext(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def twin(roots, base, floor, filt):
    """The CPU twin's (bounds, out_root, counts), computed once per case."""
    b, c = api.msd_ranges_cpu(list(roots), base, floor, filt, threads=THREADS)
    return b.tolist(), b.root_list(), c


@functools.lru_cache(maxsize=None)
def oracle_list(roots, base, floor):
    return [tuple(r) for s, e in roots for r in O.valid_ranges(s, e, base, floor)]


def check(ctx, roots, base, floor, want_ranges=None, want_numbers=None):
    """Device == CPU twin under both filters, == the oracle under the reference
    filter; the expected list is not empty."""
    roots = tuple(roots)
    for filt in FILTERS:
        want, want_root, want_counts = twin(roots, base, floor, filt)
        if filt == "reference":
            assert want == oracle_list(roots, base, floor)
            if want_ranges is not None:
                assert len(want) == want_ranges
            if want_numbers is not None:
                assert sum(e - s for s, e in want) == want_numbers
        assert want, "an empty expectation proves nothing"
        bounds, counts = ctx.msd_ranges(list(roots), base, floor, filt)
        assert len(bounds) == len(want)
        assert bounds.tolist() == want
        assert bounds.root_list() == want_root
        assert counts == want_counts
        st = ctx.msd_ranges_stats()
        assert st.ranges == len(want) and st.numbers == sum(e - s for s, e in want)
        assert st.fused_roots + st.level_roots == len(roots) and st.launches >= 1


# --- the split rule at its edges -------------------------------------------------------------------
@pytest.mark.parametrize("floor", [1, 7, 250])
@pytest.mark.parametrize("base,a", [(40, A40), (50, A50)])
def test_split_rule_edges(ctx, base, a, floor):
    sizes = [1, 2, floor - 1, floor, floor + 1, 2 * floor - 1, 2 * floor, 2 * floor + 1, 4 * floor + 3]
    check(ctx, [(a, a + z) for z in sizes if z > 0], base, floor)


# --- every arithmetic path -------------------------------------------------------------------------
PATHS = [
    (33, 5_780_673_250, 329, None),
    (40, A40, 336, 164_049),
    (45, 620_694_579_529_586, 262, None),
    (50, A50, 202, 98_628),
    (52, 243_304_715_894_231_440, 40, None),
    (57, 64_721_938_035_728_296_489, 139, None),
    (62, 7_997_740_455_941_656_547_328, 64, None),
    (64, 71_779_970_539_618_608_087_040, 117, None),
    (65, 119_730_384_190_360_286_819_380, 66, None),
    (68, 4_587_386_270_371_265_649_878_820, 110, None),
    (80, 2_589_277_757_751_866_062_101_796_092_655, 72, None),
    (97, 222_312_960_693_055_864_927_334_628_979_558_930_508, 48, None),
]


@pytest.mark.parametrize("base,a,ranges,numbers", PATHS, ids=[f"b{p[0]}" for p in PATHS])
def test_every_arithmetic_path(ctx, base, a, ranges, numbers):
    """One 1e6 root at floor 250: the run-time base (33, 97), the fast skip
    test with n in a u64 (40..52), past 64 bits (57..64), three words (65..80)."""
    check(ctx, [(a, a + 10 ** 6)], base, 250, ranges, numbers)
    assert ctx.msd_ranges_stats().fused_roots == 1


def test_b10_outside_the_fast_paths(ctx):
    check(ctx, [(47, 100)], 10, 4, 2, 13)


# --- the depth cap, in the level form --------------------------------------------------------------
@pytest.mark.parametrize("base,a,ranges", [(50, A50, 2_938), (40, A40, 4_162)])
def test_depth_cap_in_the_level_form(ctx, base, a, ranges):
    """2^23 + 3 numbers at floor 1: the recursion ends at depth 22 with ranges
    of 2 numbers, far past kFusedMaxCap floors, so the level form and the
    device ordering of its records run."""
    check(ctx, [(a, a + BIG)], base, 1, ranges)
    want, _, _ = twin(((a, a + BIG),), base, 1, "reference")
    assert {e - s for s, e in want} == {2}
    st = ctx.msd_ranges_stats()
    assert (st.fused_roots, st.level_roots) == (0, 1) and st.launches == 24  # level 0 set up, levels 0..22


# --- an empty answer -------------------------------------------------------------------------------
@pytest.mark.parametrize("size,floor", [(10 ** 6, 250), (BIG, 250), (BIG, 1)])
def test_an_empty_answer_between_two_others(ctx, size, floor):
    alone = ((EMPTY40, EMPTY40 + size),)
    assert twin(alone, 40, floor, "reference")[0] == [] == oracle_list(alone, 40, floor)
    for filt in FILTERS:
        bounds, counts = ctx.msd_ranges(list(alone), 40, floor, filt)
        assert len(bounds) == 0 and counts == [0] and bounds.tolist() == []
    roots = [(A40, A40 + 10 ** 5), alone[0], (A40 + 10 ** 6, A40 + 10 ** 6 + 10 ** 5)]
    check(ctx, roots, 40, floor)
    want, _, want_counts = twin(tuple(roots), 40, floor, "reference")
    assert want_counts[1] == 0 and want_counts[0] > 0 and want_counts[2] > 0
    assert want == sorted(want)


# --- one mixed call --------------------------------------------------------------------------------
@pytest.mark.parametrize("base,a", [(40, A40), (50, A50)])
def test_one_mixed_call_of_both_forms(ctx, base, a):
    """About 300 roots at floor 16: sizes from 1 to 2.6e5 + a few of 4e5 and
    1e6 lie on both sides of the form boundary ((2^14 - 2) * 16 = 262 112
    numbers), some repeated, some overlapping, one across the base range's end
    (its nodes outside the range take the run-time skip test)."""
    floor = 16
    edge = ((1 << 14) - 2) * floor
    _, e = O.base_range(base)
    roots = []
    for i in range(290):
        size = 1 + (i * 7919) % 3000 if i % 3 else 1 + (i * 104_729) % 20_000
        roots.append((a + i * 1500, a + i * 1500 + size))  # overlapping neighbours
    roots += [(a, a + edge), (a, a + edge + floor - 1), (a, a + edge + floor), (a + 5, a + 400_000),
              (a + 10 ** 6, a + 2 * 10 ** 6), roots[3], roots[3], (a, a + edge + floor), (e - 10 ** 5, e + 3000)]
    plan = api.msd_ranges_plan(roots, base, floor)
    assert 0 < sum(p[1] for p in plan) < len(plan)
    check(ctx, roots, base, floor)
    st = ctx.msd_ranges_stats()
    assert st.fused_roots == sum(p[1] for p in plan) and st.level_roots == len(plan) - st.fused_roots
    assert st.fused_roots > 0 and st.level_roots > 0


# --- the round trip with the production field path -------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("base,a,size,chunk,floor", [(40, A40, 3 * 10 ** 6 + 1, 999_983, 250),
                                                     (50, A50, 10 ** 7, 0, 1000)])
def test_round_trip_with_the_field_path(ctx, base, a, size, chunk, floor, filt):
    """msd_ranges of a field's chunk grid is the list that field's niceonly run
    tests: as many ranges and numbers as its statistics say, and handed to
    niceonly_ranges the same candidates and the same nice list."""
    nice, st = ctx.niceonly_raw(a, a + size, base, msd_floor=floor, chunk_size=chunk, msd_where="device", filter=filt)
    roots = api.chunk_roots(a, a + size, chunk)
    bounds, counts = ctx.msd_ranges(roots, base, floor, filt)
    assert len(bounds) == st.ranges > 0 and sum(counts) == st.ranges
    assert bounds.numbers() == st.range_numbers
    cand, _, lst = ctx.niceonly_ranges(bounds, base)
    assert sum(cand) == st.candidates > 0
    assert [n for n, _ in lst] == nice


# --- the remaining cases ---------------------------------------------------------------------------
def test_capacity_retry_returns_the_kept_list(ctx):
    roots = [(A40, A40 + 10 ** 6), (A40 + 10 ** 6, A40 + 2 * 10 ** 6)]
    want, want_root, want_counts = twin(tuple(roots), 40, 250, "reference")
    L = _lib.lib()
    rb, n_roots = api._pack_ranges(roots)
    cap = len(want) - 1
    out = (ctypes.c_uint64 * (4 * len(want)))()
    idx = (ctypes.c_uint32 * len(want))()
    counts = (ctypes.c_uint64 * 2)()
    n = ctypes.c_size_t()
    rc = L.nice_msd_ranges(ctx._h, 40, rb, n_roots, 250, 0, out, idx, counts, cap, n)
    assert rc == _lib.NICE_ERR_CAPACITY and n.value == len(want) and list(counts) == want_counts
    assert not any(out), "nothing is written without room"
    first = ctx.msd_ranges_stats()
    assert first.launches >= 1 and first.ranges == len(want)
    rc = L.nice_msd_ranges(ctx._h, 40, rb, n_roots, 250, 0, out, idx, counts, len(want), n)
    assert rc == _lib.NICE_OK and n.value == len(want)
    assert [(out[4 * i] | out[4 * i + 1] << 64, out[4 * i + 2] | out[4 * i + 3] << 64) for i in range(len(want))] == want
    assert list(idx) == want_root
    assert ctx.msd_ranges_stats() == first, "the retry returns the kept results without running again"
    # another floor is another call
    rc = L.nice_msd_ranges(ctx._h, 40, rb, n_roots, 1000, 0, out, idx, counts, len(want), n)
    assert rc == _lib.NICE_OK and n.value == len(twin(tuple(roots), 40, 1000, "reference")[0]) != len(want)


def test_argument_errors_on_the_device_call(ctx):
    L = _lib.lib()
    rb, _ = api._pack_ranges([(47, 100), (5, 5)])
    out = (ctypes.c_uint64 * 64)()
    n = ctypes.c_size_t()
    assert L.nice_msd_ranges(ctx._h, 10, rb, 1, 4, 0, out, None, None, 16, n) == _lib.NICE_OK and n.value == 2
    assert L.nice_msd_ranges(ctx._h, 10, rb, 2, 4, 0, out, None, None, 16, n) == _lib.NICE_ERR_INVALID
    assert b"root 1" in L.nice_last_error()
    assert L.nice_msd_ranges(ctx._h, 10, rb, 0, 4, 0, out, None, None, 16, n) == _lib.NICE_ERR_INVALID
    assert L.nice_msd_ranges(ctx._h, 10, rb, 1, 0, 0, out, None, None, 16, n) == _lib.NICE_ERR_INVALID
    assert L.nice_msd_ranges(ctx._h, 10, rb, 1, 4, 2, out, None, None, 16, n) == _lib.NICE_ERR_INVALID
    assert L.nice_msd_ranges(ctx._h, 129, rb, 1, 4, 0, out, None, None, 16, n) == _lib.NICE_ERR_INVALID
    rb, _ = api._pack_ranges([(47, 48 + (1 << 40))])
    assert L.nice_msd_ranges(ctx._h, 10, rb, 1, 4, 0, out, None, None, 16, n) == _lib.NICE_ERR_INVALID


def test_two_devices_give_the_single_device_answer(ctx):
    roots = [(A50, A50 + 2 * 10 ** 6)] + [(A50 + i * 10 ** 5, A50 + (i + 1) * 10 ** 5) for i in range(9)]
    assert len({p[2] for p in api.msd_ranges_plan(roots, 50, 100, 2)}) == 2
    two = N.GpuContext([0, 0])
    try:
        for filt in FILTERS:
            want, want_root, want_counts = twin(tuple(roots), 50, 100, filt)
            assert want
            bounds, counts = two.msd_ranges(roots, 50, 100, filt)
            assert (bounds.tolist(), bounds.root_list(), counts) == (want, want_root, want_counts)
            one, one_counts = ctx.msd_ranges(roots, 50, 100, filt)
            assert (one.tolist(), one_counts) == (want, want_counts)
        st = two.msd_ranges_stats()
        assert (st.fused_roots, st.level_roots) == (9, 1)
    finally:
        two.close()


def test_survey_device_placement_equals_host(ctx):
    host = survey.survey_niceonly_base(ctx, 50, windows=64, threads=THREADS)
    dev = survey.survey_niceonly_base(ctx, 50, windows=64, threads=THREADS, msd_where="device")
    assert host == dev
    assert host.reference.msd_ranges > 0 and host.sound.msd_ranges >= host.reference.msd_ranges
