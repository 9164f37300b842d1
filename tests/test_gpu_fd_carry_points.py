"""Every FD kernel stepped across the deep carries of tests/fd_carry_points.py.

A carry out of the top stepped limb of n^2 or n^3 goes to rare() and ripples
through the cached limbs (carry_plain), and 2n+1 / 3n+1 carry into their upper
limbs (carry_scaled, carry_n3) -- at numbers far rarer than any window the
rest of the suite compares with the oracle.  Here each such number n* sits in
the middle of one lane's run and every kernel family walks across it: the map
kernel (one byte per n: a wrong step shows at its own position), the batch
kernel, the small-field kernels, the big-field and persistent kernels and the
sibling-lane kernels (rare_sib).  A wrong ripple corrupts every later number
of the lane's run, so each comparison is exact and with the oracle.

Run on the MI355X box:  python -m pytest tests/test_gpu_fd_carry_points.py -m gpu -q -rA
"""
import functools

import numpy as np
import pytest

import nice_amd as N
from oracle import oracle as O

import fd_carry_points as F
import near_miss_windows as W
from test_ranges import plan

pytestmark = pytest.mark.gpu
BASES = W.fd_bases()


@pytest.fixture(scope="module")
def ctx():
    c = N.GpuContext(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def per_number(a, b, base):
    """The oracle's count of every n in [a, b): process_range_detailed listing
    everything (cutoff 0), computed once per range."""
    r = O.process_range_detailed(a, b, base, cap=b - a, cutoff=0)
    assert [n for n, _ in r.nice_numbers] == list(range(a, b))
    m = np.array([u for _, u in r.nice_numbers], dtype=np.uint8)
    m.setflags(write=False)
    return m


def row_and_list(m, a, base):
    """(histogram with base + 1 bins, production near-miss list) of the
    numbers whose counts are m, the first of them a."""
    pos = np.nonzero(m > O.near_miss_cutoff(base))[0]
    return np.bincount(m, minlength=base + 1).tolist(), [(a + int(i), int(m[i])) for i in pos]


def same(got, want, what):
    """Byte for byte; on a mismatch the first differing positions."""
    assert got.dtype == np.uint8 and got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, bad.size, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


def chunk_of(base):
    """The chunk of a WINDOW-number map or batch tile: 41 at 512 threads, 21 at
    1024 (test_fd_carry_points.py pins it, and where n* then falls, against
    both plans)."""
    rs, _ = O.base_range(base)
    wg = plan(base, [(rs, rs + 10 ** 6)])[0][1]
    assert wg in (512, 1024)
    return 41 if wg == 512 else 21


def shifted(want, a, size, base):
    """The (hist, list) of [a - 1, a - 1 + size) from that of [a, a + size)."""
    hist, lst = list(want[0]), list(want[1])
    cutoff = O.near_miss_cutoff(base)
    u_in, u_out = O.num_unique_digits(a - 1, base), O.num_unique_digits(a + size - 1, base)
    hist[u_in] += 1
    hist[u_out] -= 1
    if lst and lst[-1][0] == a + size - 1:
        lst.pop()
    if u_in > cutoff:
        lst.insert(0, (a - 1, u_in))
    return hist, lst


# --- 1. the map kernel, number by number ----------------------------------------------------
@pytest.mark.parametrize("base", BASES)
def test_map_across_every_point(ctx, base):
    """fd2_map_kernel: n* is number chunk // 2 of lane 100's run in a window of
    20 001 numbers (one main workgroup and a tail)."""
    chunk = chunk_of(base)
    for _, q, k, n in F.points(base):
        a = F.window_for(n, chunk)
        same(ctx.unique_map(a, a + F.WINDOW, base), per_number(a - 1, a + F.WINDOW, base)[1:],
             f"b{base} {q} level {k} n* {n} at position {n - a}")
        st = ctx.map_stats()
        assert (st.fd_segments, st.fd_numbers, st.generic_segments, st.generic_numbers) == (1, F.WINDOW, 0, 0)


# --- 2. the batch kernel ------------------------------------------------------------------------
@pytest.mark.parametrize("base", BASES)
def test_batch_across_every_point(ctx, base):
    """fd2_batch_kernel: all windows of the base in one call, each twice, the
    second copy one number lower; one launch per limb layout."""
    chunk = chunk_of(base)
    ranges, want_rows, want_list = [], [], []
    for _, q, k, n in F.points(base):
        a = F.window_for(n, chunk)
        m = per_number(a - 1, a + F.WINDOW, base)
        for x, part in ((a, m[1:]), (a - 1, m[:-1])):
            row, near = row_and_list(part, x, base)
            want_list += [(nn, u, len(ranges)) for nn, u in near]
            ranges.append((x, x + F.WINDOW))
            want_rows.append(row)
    rows, lst = ctx.detailed_ranges(ranges, base)
    st = ctx.ranges_stats()
    assert st.fallback_ranges == 0 and st.launches == len(F.intervals(base))
    bad = [i for i in range(len(ranges)) if rows[i] != want_rows[i]]
    assert not bad, (base, [(F.points(base)[i // 2][1:], i % 2) for i in bad[:6]])
    assert lst == want_list


# --- 3. the small-field kernels -----------------------------------------------------------------
def _layouts():
    return [(b, i) for b in BASES for i in range(len(F.intervals(b)))]


@pytest.mark.parametrize("base,layout", _layouts())
def test_small_field_across_every_point(ctx, base, layout):
    """The < 1e7 kernels (512 threads; they include the table-free
    configurations that neither the map nor the batch kernel instantiates):
    [n* - 20 000, n* + 45 537) and the same window one number lower, histogram
    and production near-miss list (mostly empty: the histogram is the
    comparison) against the oracle.

    No plan hook says where a lane's run starts here, so the shift is the
    placement guarantee: plan_regular tiles a segment from its first number
    with ONE chunk >= min_chunk = 4, so the chunk boundaries of the two runs
    differ by one number, and in at least one of them n* - 1 and n* are walked
    by the same lane.  n* lies in the first third of the window, away from the
    one-number-per-lane tail."""
    iv = F.intervals(base)[layout]
    for _, q, k, n in (p for p in F.points(base) if p[0] == iv):
        a, size = n - 20_000, 65_537
        m = per_number(a - 1, a + size, base)
        for x, part in ((a, m[1:]), (a - 1, m[:-1])):
            got = ctx.detailed_raw(x, x + size, base)
            assert ctx.kernel_stats().fd_kernel
            assert got == row_and_list(part, x, base), (base, q, k, n, x)


# --- 4. the big-field and persistent kernels ----------------------------------------------------
@pytest.mark.parametrize("q", ["S", "C"])
@pytest.mark.parametrize("base", [40, 53, 60, 65, 80])
def test_big_field_across_the_deepest_points(ctx, base, q):
    """Fields of >= 1e7 numbers (1024 threads, valu_limbs_big), one base per
    class: 1.2e7 numbers from n* - 4 000 000 and from n* - 4 000 001, n* the
    deepest point of n^2 / n^3 in the base's first limb layout."""
    _, _, k, n = F.deepest(base, q)
    a, size = n - 4_000_000, 12_000_000
    want = W.oracle(a, a + size, base)
    for x, exp in ((a, want), (a - 1, shifted(want, a, size, base))):
        got = ctx.detailed_raw(x, x + size, base)
        assert ctx.kernel_stats().fd_kernel
        assert got[0] == exp[0], (base, q, k, n, x)
        assert got[1] == exp[1], (base, q, k, n, x)


# --- 5. the sibling-lane kernels ---------------------------------------------------------------------
@pytest.mark.parametrize("q", ["S", "C"])
@pytest.mark.parametrize("base,layout,stride", [(40, 0, 143), (40, -1, 81), (47, 0, 161)])
def test_sibling_lanes_across_the_deepest_points(ctx, base, layout, stride, q):
    """rare_sib (cached S limbs in K form, cached C limbs in LDS): b40 in its
    first limb layout (pipelined walk) and its last (lookup-group walk), b47
    (two lanes, short low-digit table).  The field has the shape of
    test_gpu_near_miss_list.sib_field -- 4 super-blocks of M b^4 numbers and a
    ragged remainder, inside one layout -- placed so that n* is the middle
    number of sibling j = 1's b^4 block in super-block 1, and runs from two
    starts one apart.

    A lone field this short leaves the sibling kernel for the regular one
    (plan_sib: below 1.5 rounds of the resident lanes), which part 4 covers; as
    in test_sibling_lane_kernels the lane stride is set through
    nice_debug_force_sib_stride, which keeps the sibling kernel on a field of
    >= 4 super-blocks: the pipelined walk's pick on a 1e9 field (143), TCHUNK +
    1 (81, 161) elsewhere -- all leave an edge unit.  A lane's unit is stride
    numbers from a multiple of the stride inside the b^4 block, so n* - 1 and
    n* are walked by one lane, with numbers to follow, at both starts.
    Nothing forces the persistent grid; the printed line says which ran."""
    iv = F.intervals(base)[layout]
    _, _, k, n = F.deepest(base, q, iv)
    m = 3 if base <= 45 else 2
    d = base ** 4
    size = 4 * m * d + 1_234_567
    a = n - (m * d + d + d // 2)
    assert iv[0] < a - 1 and a + size <= iv[1]
    want = W.oracle(a, a + size, base)
    lib = N._lib.lib()
    try:
        assert lib.nice_debug_force_sib_stride(stride) == 0
        for x, exp in ((a, want), (a - 1, shifted(want, a, size, base))):
            o = n - x
            assert o // (m * d) == 1 and (o // d) % m == 1 and 1 <= (o % d) % stride <= stride - 3
            assert (o % d) // stride < d // stride  # a full unit, not the edge unit
            got = ctx.detailed_raw(x, x + size, base)
            st = ctx.kernel_stats()
            assert st.sib_lanes == m and st.sib_stride == stride and st.fd_kernel, st
            print(f"sibling b{base} layout {layout} {q} level {k}, start n* - {o}: stride {st.sib_stride}, "
                  f"{'persistent grid of ' + str(st.sib_grid) if st.sib_grid else 'rounds of workgroups'}")
            assert got[0] == exp[0], (base, q, k, n, x)
            assert got[1] == exp[1], (base, q, k, n, x)
    finally:
        lib.nice_debug_force_sib_stride(0)
