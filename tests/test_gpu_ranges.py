"""Batched detailed ranges on the GPU (nice_process_ranges_detailed, the
fd2_batch_kernel): every row against the oracle or the per-field call (which
tests/test_gpu_parity.py pins to the oracle), the launch count, near-misses,
fallbacks, list overflow, two devices and the base survey.

Run on the MI355X box:  python -m pytest tests/test_gpu_ranges.py -m gpu -q
"""
import ctypes
import random

import pytest

import nice_amd as N
from nice_amd import _lib, api, survey
from oracle import oracle as O

pytestmark = pytest.mark.gpu
MASK = (1 << 64) - 1


@pytest.fixture(scope="module")
def ctx():
    c = N.GpuContext(0)
    yield c
    c.close()


def oracle_row(a, b, base):
    r = O.process_range_detailed(a, b, base, cap=b - a)
    return [0] + [c for _, c in r.distribution], r.nice_numbers


def cuts_of(base):
    buf = (ctypes.c_uint64 * 16)()
    n = ctypes.c_size_t()
    assert _lib.lib().nice_fd_segment_cuts(base, buf, 8, n) == 0
    return [buf[2 * i] | (buf[2 * i + 1] << 64) for i in range(n.value)]


def shape_of(base):
    """(WG, chunk) of the base's batch plan (tests/test_ranges.py pins both):
    the lanes of a full workgroup and the target chunk."""
    s, _ = O.base_range(base)
    b = (ctypes.c_uint64 * 4)(s & MASK, s >> 64, (s + 10 ** 6) & MASK, (s + 10 ** 6) >> 64)
    buf = (ctypes.c_uint64 * 6)()
    n = ctypes.c_size_t()
    assert _lib.lib().nice_debug_ranges_plan(base, b, 1, buf, 1, n) == 0
    return buf[2], (80 if base <= 45 else 160 if base <= 58 else 240) + 1


def check_rows(ctx, ranges, base):
    rows, lst = ctx.detailed_ranges(ranges, base)
    assert len(rows) == len(ranges)
    want_list = []
    for i, (a, b) in enumerate(ranges):
        row, near = oracle_row(a, b, base)
        assert rows[i] == row, (base, i, a, b - a)
        want_list += [(n, u, i) for n, u in near]
    assert lst == want_list
    return rows, lst


# --- 1. edge sizes against the oracle ----------------------------------------------
FD_BASES = [b for b in range(2, 129) if _lib.lib().nice_fd_kernel_base(b) == 1]


def test_the_old_bases_are_fd_bases():
    assert {40, 52, 62, 80} <= set(FD_BASES) and len(FD_BASES) == 24


@pytest.mark.parametrize("base", FD_BASES)
def test_edge_sizes_match_oracle(ctx, base):
    """Every base with an FD kernel (one / two / three mask words; low-digit
    table, LSDX, no low-digit table; TIGHT entry; limbs decoded by VALU; 512 and
    1024 threads): every size at which the plan changes shape, at the range's
    first and last n, a full workgroup and one number from the first n of every
    limb layout and up to its last -- so every fd2_batch_kernel instantiation
    of the base runs -- across every cut and at seeded interior points, in ONE
    call of one launch per layout."""
    s, e = O.base_range(base)
    cuts = cuts_of(base)
    wg, chunk = shape_of(base)
    assert wg in (512, 1024)
    sizes = (1, 2, 63, 64, 65, chunk - 1, chunk, chunk + 1, wg - 1, wg, wg + 1, wg * chunk, wg * chunk + 1)
    rng = random.Random(100 + base)
    ranges = []
    at_s, at_e = s, e
    for size in sizes:
        a = rng.randrange(s, e - size)
        ranges.append((a, a + size))          # seeded interior point
        if size <= wg + 1:                    # packed from the first n up and from the last n down
            ranges.append((at_s, at_s + size))
            ranges.append((at_e - size, at_e))
            at_s, at_e = at_s + size, at_e - size
    ranges += [(s, s + 1), (e - 1, e), (s, s + wg * chunk + 1), (e - wg * chunk - 1, e)]
    ranges += [(c - 1000, c + 1000) for c in cuts]
    # the same two at the inner ends of every limb layout (the cut is the next layout's first n)
    ranges += [r for c in cuts for r in ((c - wg * chunk - 1, c), (c, c + wg * chunk + 1))]
    check_rows(ctx, ranges, base)
    st = ctx.ranges_stats()
    assert st.launches == len(cuts) + 1 and st.fallback_ranges == 0
    assert st.numbers == sum(b - a for a, b in ranges)


# --- 2. many ranges -------------------------------------------------------------------
def survivor_ranges(n=3000, seed=2):
    """Seeded disjoint b40 ranges of 100-400 numbers: the shape of MSD survivors."""
    s, e = O.base_range(40)
    rng = random.Random(seed)
    starts = sorted(rng.sample(range(s, e - 1000, 1000), n))
    return [(a, a + rng.randrange(100, 401)) for a in starts]


@pytest.fixture(scope="module")
def many(ctx):
    ranges = survivor_ranges()
    rows, lst = ctx.detailed_ranges(ranges, 40)
    return ranges, rows, lst, ctx.ranges_stats()


def test_many_small_ranges(ctx, many):
    ranges, rows, lst, st = many
    assert st.launches <= 3 and st.fallback_ranges == 0
    want = []
    for i, (a, b) in enumerate(ranges):
        row, near = oracle_row(a, b, 40)
        assert rows[i] == row, i
        want += [(n, u, i) for n, u in near]
    assert lst == want
    srow, slst = ctx.detailed_ranges(ranges, 40, sum=True)
    assert srow == [[sum(col) for col in zip(*rows)]] and slst == lst
    assert ctx.ranges_stats().launches <= 3


def test_msd_survivors_pass_straight_in(ctx):
    """nice_msd_valid_ranges' own output on a 1e6 b40 window, handed over as it
    was written (four u64 per range)."""
    L = _lib.lib()
    s, e = O.base_range(40)
    a = s + (e - s) // 2  # (the MSD filter keeps nothing of a 1e6 window in the range's first third)
    n = ctypes.c_size_t()
    rc = L.nice_msd_valid_ranges(a & MASK, a >> 64, (a + 10 ** 6) & MASK, (a + 10 ** 6) >> 64, 40, 250, None, 0, n)
    assert rc in (_lib.NICE_OK, _lib.NICE_ERR_CAPACITY) and n.value > 100
    nr = n.value
    bounds = (ctypes.c_uint64 * (4 * nr))()
    assert L.nice_msd_valid_ranges(a & MASK, a >> 64, (a + 10 ** 6) & MASK, (a + 10 ** 6) >> 64, 40, 250,
                                   bounds, nr, n) == _lib.NICE_OK
    hist = (ctypes.c_uint64 * (41 * nr))()
    out = (_lib.nice_number * 64)()
    cnt = ctypes.c_size_t()
    assert L.nice_process_ranges_detailed(ctx._h, 40, bounds, nr, _lib.NICE_RANGES_PER_RANGE, hist, out, None,
                                          64, cnt) == _lib.NICE_OK
    for i in range(nr):
        x, y = bounds[4 * i] | (bounds[4 * i + 1] << 64), bounds[4 * i + 2] | (bounds[4 * i + 3] << 64)
        assert list(hist[41 * i:41 * (i + 1)]) == oracle_row(x, y, 40)[0], i
    st = ctx.ranges_stats()
    assert st.launches <= 3 and st.fallback_ranges == 0


# --- 3. against the single-field path at size -------------------------------------------
@pytest.mark.parametrize("base", [40, 80])
def test_default_field_three_ways(ctx, base):
    if base == 40:
        f = N.get_benchmark_field(N.BenchmarkMode.DEFAULT)
        a, b = f.range_start, f.range_end
    else:
        f = N.get_benchmark_field(N.BenchmarkMode.HI_BASE, 10 ** 6)
        a, b = f.range_start, f.range_start + 10 ** 6
    assert b - a == 10 ** 6
    hist, lst = ctx.detailed_raw(a, b, base)
    rows, l1 = ctx.detailed_ranges([(a, b)], base)
    assert rows == [hist] and [(n, u) for n, u, _ in l1] == lst
    tens = [(a + 10 ** 5 * k, a + 10 ** 5 * (k + 1)) for k in range(10)]
    rows, l10 = ctx.detailed_ranges(tens, base)
    assert [sum(col) for col in zip(*rows)] == hist and [(n, u) for n, u, _ in l10] == lst
    for k in (0, 9):
        assert rows[k] == ctx.detailed_raw(*tens[k], base)[0]
    thousand = [(a + 1000 * k, a + 1000 * (k + 1)) for k in range(1000)]
    srow, ls = ctx.detailed_ranges(thousand, base, sum=True)
    assert srow == [hist] and [(n, u) for n, u, _ in ls] == lst
    st = ctx.ranges_stats()
    assert st.launches <= 3 and st.fallback_ranges == 0 and st.numbers == 10 ** 6


# --- 4. near-misses through the batch kernel ----------------------------------------------
# A b40 window whose near-miss list is not empty (in-range near-misses are rare:
# the committed 1e9 fixtures have none), found with detailed_raw on the MI355X.
NEAR_WINDOW = (2_016_284_264_916, 2_036_284_264_916)
NEAR_COUNT = 10


@pytest.fixture(scope="module")
def near(ctx):
    a, b = NEAR_WINDOW
    assert 0 < b - a <= 10 ** 11
    _, lst = ctx.detailed_raw(a, b, 40)
    return lst


def test_near_misses_in_a_batch(ctx, near):
    a, b = NEAR_WINDOW
    assert len(near) == NEAR_COUNT
    cutoff = O.near_miss_cutoff(40)
    for n, u in near:
        assert a <= n < b and u == O.num_unique_digits(n, 40) and u > cutoff
    quiet = survivor_ranges(200, seed=9)
    around = [(n - 500, n + 500) for n, _ in near]
    # the two closest entries (9.2e7 apart): one range over both of their ranges
    k = min(range(len(near) - 1), key=lambda i: near[i + 1][0] - near[i][0])
    both = (near[k][0] - 100, near[k + 1][0] + 100)
    assert both[1] - both[0] < 1 << 27
    ranges = quiet[:100] + around + [around[0], both] + quiet[100:]
    random.Random(4).shuffle(ranges)
    rows, lst = ctx.detailed_ranges(ranges, 40)
    st = ctx.ranges_stats()
    assert st.launches <= 3 and st.fallback_ranges == 0
    want = []
    for i, (x, y) in enumerate(ranges):
        mine = [(n, u, i) for n, u in near if x <= n < y]      # ascending, as `near` is
        if (x, y) in quiet:
            row, onear = oracle_row(x, y, 40)
            assert rows[i] == row and not onear and not mine
        elif (x, y) == both:
            assert len(mine) == 2 and rows[i] == ctx.detailed_raw(x, y, 40)[0]
        else:
            assert len(mine) == 1 and rows[i] == oracle_row(x, y, 40)[0]
        want += mine
    assert lst == want
    assert len(lst) == NEAR_COUNT + 1 + 2 and len({i for _, _, i in lst}) == NEAR_COUNT + 2


# --- 5. fallbacks in the same call ---------------------------------------------------------
def test_fallback_ranges_in_the_same_call(ctx):
    s, e = O.base_range(40)
    ranges = [(s + 5000, s + 5400), (e - 300, e + 100), (s - 100, s + 300), (s + 10 ** 6, s + 10 ** 6 + 77),
              (e - 900, e + 100), (s - 100, s + 900), (e + 5, e + 50), (s, s + 64)]
    rows, lst = ctx.detailed_ranges(ranges, 40)
    st = ctx.ranges_stats()
    assert st.fallback_ranges == 5 and 1 <= st.launches <= 3
    want = []
    for i, (a, b) in enumerate(ranges):
        hist, near = ctx.detailed_raw(a, b, 40)
        assert rows[i] == hist, i
        assert rows[i] == oracle_row(a, b, 40)[0], i
        want += [(n, u, i) for n, u in near]
    assert lst == want
    srow, _ = ctx.detailed_ranges(ranges, 40, sum=True)
    assert srow == [[sum(col) for col in zip(*rows)]]


def test_non_fd_base_and_base_ten(ctx):
    s, _ = O.base_range(70)
    r70 = [(s + 1000, s + 1300), (s + 1100, s + 1500)]
    rows, lst = ctx.detailed_ranges(r70, 70)
    assert rows == [ctx.detailed_raw(a, b, 70)[0] for a, b in r70]
    st = ctx.ranges_stats()
    assert (st.fallback_ranges, st.launches) == (2, 0)
    rows, lst = ctx.detailed_ranges([(47, 100), (60, 80)], 10)
    assert rows[0] == ctx.detailed_raw(47, 100, 10)[0] and rows[0] == oracle_row(47, 100, 10)[0]
    assert lst == [(69, 10, 0), (69, 10, 1)]
    assert ctx.ranges_stats().fallback_ranges == 2


# --- 6. list overflow ------------------------------------------------------------------------
def test_short_list_reports_the_needed_length(ctx):
    L = _lib.lib()
    ranges = [(1_000_000, 1_005_000), (1_005_000, 1_010_000)]
    want = ctx.detailed_raw(1_000_000, 1_010_000, 10)[1]
    assert len(want) == 5395
    flat = []
    for a, b in ranges:
        flat += [a, 0, b, 0]
    bounds = (ctypes.c_uint64 * 8)(*flat)
    hist = (ctypes.c_uint64 * 22)()
    out = (_lib.nice_number * 5395)()
    idx = (ctypes.c_uint32 * 5395)()
    n = ctypes.c_size_t()
    rc = L.nice_process_ranges_detailed(ctx._h, 10, bounds, 2, 0, hist, out, idx, 16, n)
    assert (rc, n.value) == (_lib.NICE_ERR_CAPACITY, 5395)
    rc = L.nice_process_ranges_detailed(ctx._h, 10, bounds, 2, 0, hist, out, idx, n.value, n)
    assert (rc, n.value) == (_lib.NICE_OK, 5395)
    assert [(out[i].number_lo, out[i].num_uniques) for i in range(5395)] == want
    assert [idx[i] for i in range(5395)] == [0 if nn < 1_005_000 else 1 for nn, _ in want]
    assert [hist[i] + hist[11 + i] for i in range(11)] == ctx.detailed_raw(1_000_000, 1_010_000, 10)[0]


def test_device_list_overflow_reruns_the_batch(near):
    """More entries in one batch than the device list's first size (4096): the
    list is grown and the batch run again.  In-range near-misses are rare, so
    the entries are one near-miss in 5000 copies of a three-number range -- every
    copy records it, and every copy gets it back."""
    n, u = near[0]
    ranges = [(n - 1, n + 2)] * 5000
    c = N.GpuContext(0)  # a fresh context: its list has its first size
    try:
        rows, lst = c.detailed_ranges(ranges, 40)
        assert lst == [(n, u, i) for i in range(5000)]
        assert rows == [oracle_row(n - 1, n + 2, 40)[0]] * 5000
        assert c.ranges_stats().launches == 1 and c.ranges_stats().fallback_ranges == 0
        srow, slst = c.detailed_ranges(ranges, 40, sum=True)
        assert srow == [[5000 * v for v in rows[0]]] and slst == lst
    finally:
        c.close()


def test_descriptor_staging_regrows_between_calls(ctx):
    """One context, three calls: 1 range, then 5000 ranges of 100 numbers --
    more workgroups than the descriptor staging's first size (4096), so the
    pinned and device buffers are replaced -- then 1 range again, each against
    the CPU twin."""
    s, e = O.base_range(40)
    rng = random.Random(11)
    big = [(a, a + 100) for a in sorted(rng.sample(range(s, e - 1000, 1000), 5000))]
    units = ctypes.c_size_t()
    _lib.check(_lib.lib().nice_debug_ranges_plan(40, api._pack_ranges(big)[0], len(big), None, 0, units))
    assert units.value > 4096
    for ranges in ([big[0]], big, [big[-1]]):
        assert ctx.detailed_ranges(ranges, 40) == api.detailed_ranges_cpu(ranges, 40, threads=16)
        assert ctx.ranges_stats().fallback_ranges == 0


# --- 7. two devices ------------------------------------------------------------------------------
def test_two_device_context_gives_the_same(many):
    ranges, rows, lst, _ = many
    c2 = N.GpuContext([0, 0])
    try:
        r2, l2 = c2.detailed_ranges(ranges, 40)
        assert r2 == rows and l2 == lst
        s2, _ = c2.detailed_ranges(ranges, 40, sum=True)
        assert s2 == [[sum(col) for col in zip(*rows)]]
        assert c2.ranges_stats().launches <= 6 and c2.ranges_stats().fallback_ranges == 0
    finally:
        c2.close()


# --- 8. survey ------------------------------------------------------------------------------------
def test_survey_matches_the_cpu_twin(ctx):
    g = survey.survey_base(ctx, 50, windows=256, window_size=2000, seed=3)
    c = survey.survey_base(None, 50, windows=256, window_size=2000, seed=3, threads=8)
    assert g == c and g.numbers == 256 * 2000
    assert ctx.ranges_stats().fallback_ranges == 0 and ctx.ranges_stats().launches <= 3
