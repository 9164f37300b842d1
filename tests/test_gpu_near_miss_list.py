"""The FD kernels' near-miss list, with something in it.

The production FD kernels record a listed number only on their out-of-window
branch when u > cutoff = floor(0.9 b): about once in 1e8 numbers at b40 and
never, in this suite, at b >= 57 where n passes 64 bits.  Every other list
comparison on an in-range FD field compares [] with [].  Here
nice_debug_set_near_miss_cutoff lowers the cutoff to the top of the base's
histogram window (W0 + W - 1), so every number on the high out-of-window
branch is listed -- tens to thousands per 1e6 -- and each way the device and
the host rebuild and carry an entry is compared with the oracle at the same
cutoff: walk_chunk (small-field, big-field, persistent grid, batch kernel),
sib_record and the per-sibling lookup-group walk, the tagged count word, the
list growth with the shard re-run, the order across shards.

Every comparison checks, through `same`: a non-empty expected list; the
histogram; the list exactly (n with its high word, u, the range index for
ranges); ascending n; length == the histogram's bins above the lowered cutoff.

Run on the MI355X box:  python -m pytest tests/test_gpu_near_miss_list.py -m gpu -q -rA
(-rA shows the entries each kernel path saw).
"""
import functools
import random

import pytest

import nice_amd as N
from nice_amd import _lib
from oracle import oracle as O

import near_miss_windows as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = N.GpuContext(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def want(a, e, base, cutoff=None):
    """The oracle's (hist, list) of [a, e), computed once per module."""
    return W.oracle(a, e, base, cutoff)


def same(got, exp, cutoff, what, at_least=1):
    """The checks every comparison of this file makes (see the module text)."""
    (h, lst), (hw, lw) = got, exp
    assert len(lw) >= at_least, f"{what}: the expected list has {len(lw)} entries; nothing would be compared"
    assert h == hw, f"{what}: histogram"
    assert lst == lw, f"{what}: list ({len(lst)} entries, expected {len(lw)})"
    assert all(x[0] < y[0] for x, y in zip(lst, lst[1:])), f"{what}: not ascending in n"
    assert len(lst) == sum(h[cutoff + 1:]), f"{what}: list length against the bins above the cutoff"
    print(f"near-miss entries, {what}: {len(lst)}")
    return len(lst)


def pieces(ctx, a, e, base, piece):
    """Sum of the histograms and concatenation of the lists of [a, e) run in
    consecutive pieces (each below 1e7 numbers: the small-field kernel, which
    test_small_field_kernel pins to the oracle)."""
    hs, ls = [0] * (base + 1), []
    while a < e:
        b = min(e, a + piece)
        hk, lk = ctx.detailed_raw(a, b, base)
        hs = [x + y for x, y in zip(hs, hk)]
        ls += lk
        a = b
    return hs, ls


# --- a. the small-field kernel, every FD base ------------------------------------------
@pytest.mark.parametrize("base", sorted(W.WINDOW_FRAC))
def test_small_field_kernel(ctx, base):
    """walk_chunk's n0 + (r8 - r80) / ES, the tagged count word and, at
    b >= 57, number_hi: the table's 1e6 window, a ragged start and size inside
    it, and a 1e6 window across each limb-count cut of the base's range."""
    a, e = W.window(base)
    s, r1 = O.base_range(base)
    empty_cuts = []
    with W.lowered(base) as c:
        exp = want(a, e, base, c)
        assert len(exp[1]) >= W.MIN_ENTRIES
        same(ctx.detailed_raw(a, e, base), exp, c, f"walk_chunk small b{base} 1e6")
        assert ctx.kernel_stats().fd_kernel
        if base >= 57:
            assert all(n >> 64 for n, _ in exp[1]), "b >= 57: every n of the window is wider than 64 bits"
        x, y = a + 11, a + 11 + 65_537
        ragged = want(x, y, base, c)
        if ragged[1]:
            same(ctx.detailed_raw(x, y, base), ragged, c, f"walk_chunk small b{base} ragged")
        else:  # (rates below 15 per 1e6: the 65 537 numbers may hold none)
            assert ctx.detailed_raw(x, y, base) == ragged
        for cut in W.cuts_of(base):
            x, y = max(s, cut - 500_000), min(r1, cut + 500_000)
            across = want(x, y, base, c)
            if not across[1]:
                empty_cuts.append(cut)
                continue
            same(ctx.detailed_raw(x, y, base), across, c, f"walk_chunk small b{base} across cut {cut}")
    if empty_cuts:
        print(f"b{base}: no number above the window within 5e5 of the cut(s) {empty_cuts}; sub-case skipped")


# --- b. the big-field kernel ---------------------------------------------------------------
@pytest.mark.parametrize("base", [40, 45, 50, 53, 58, 60, 64, 65, 68, 80])
def test_big_field_kernel(ctx, base):
    """Fields of >= 1e7 and < 2e7 numbers leave the small-field kernel: the
    1024-thread kernel with its valu_limbs_big choice at b58 and above, and at
    b40..53 the sibling configuration's regular-kernel fallback (the field is
    shorter than 4 super-blocks); their result words are still tagged.  1.2e7
    at the table's fraction, one base per class, against the oracle."""
    a, _ = W.window(base)
    e = a + 12_000_000
    with W.lowered(base) as c:
        same(ctx.detailed_raw(a, e, base), want(a, e, base, c), c, f"walk_chunk big b{base} 1.2e7", W.MIN_ENTRIES)
        assert ctx.kernel_stats().fd_kernel


# --- c. the persistent grid ------------------------------------------------------------------
@pytest.mark.parametrize("base", [42, 49, 58, 59, 65, 68, 80])
def test_persistent_grid(ctx, base):
    """One field of 1.5 x the two-round threshold of the base's TCHUNK class
    must equal its consecutive 9 000 001-number pieces, which run on the
    small-field kernel (pinned to the oracle above).  No oracle on the whole
    field.  b58, b65, b68 and b80 hold one 1024-thread workgroup per CU and run
    such a field on the persistent grid (waves pull strided 64-unit batches,
    each with its own n0); b59 holds two and runs rounds of workgroups; b42 and
    b49 go through the sibling-lane dispatch at this size (its regular-kernel
    fallback or the sibling kernel: the printed line says which)."""
    size = {80: 63_000_000, 160: 130_000_000, 240: 190_000_000}[80 if base <= 45 else 160 if base <= 58 else 240]
    a, _ = W.window(base)
    with W.lowered(base) as c:
        got = ctx.detailed_raw(a, a + size, base)
        st = ctx.kernel_stats()
        exp = pieces(ctx, a, a + size, base, 9_000_001)
        same(got, exp, c, f"persistent b{base} {size:.1e} (sibling lanes {st.sib_lanes})", 100)
        assert sum(got[0]) == size and st.fd_kernel


# --- d. the sibling-lane kernels ---------------------------------------------------------------
def sib_field(base, frac):
    """_stride_field's shape (4 super-blocks of M B^2 numbers -- B = base^2 --
    plus a ragged remainder, inside one limb layout), moved so that a listed
    number sits 5 before the end of the B^2 block of sibling j = 1 in
    super-block 0: the last numbers of a block are the edge unit of every lane
    stride L with B^2 mod L >= 5."""
    m = 3 if base <= 45 else 2
    d = base ** 4
    n = 4 * m * d + 1_234_567
    c = W.low_cutoff(base)
    x = W.at(base, frac) + 777 + 2 * d
    while True:  # the first listed number from there on
        lst = want(x, x + 500_000, base, c)[1]
        if lst:
            break
        x += 500_000
    s = lst[0][0] - 2 * d + 5
    r0, r1 = O.base_range(base)
    assert r0 <= s and s + n <= r1 and not any(s < cut < s + n for cut in W.cuts_of(base))
    return m, d, s, n


@pytest.mark.parametrize("base,frac,strides", [
    (40, 0.0, (125, 105, 209)),   # pipelined walk (sib_record), picker range [105, 210]; oracle
    (40, 0.5, (125, 61, 119)),    # per-sibling lookup-group walk, [60, 120]; oracle
    (44, 0.3, (121, 61, 119)),    # M = 3, lookup groups; 4.6e7 numbers: pieces
    (52, 0.2, (169, 121, 239)),   # M = 2, short low-digit table, [120, 240]; 6.0e7: pieces
    (55, 0.8, (125, 123, 239)),   # the same; 7.4e7: pieces
])
def test_sibling_lane_kernels(ctx, base, frac, strides):
    """sib_record's su.lo + j B^2 + i and the lookup-group walk's su + j B^2 +
    (r8 - r80) / ES, at three forced lane strides: the first divides B^2 (no
    edge units), the others leave edge units and sit at the two ends of the
    picker's range.  Fields of up to 3.5e7 numbers (b40) are compared with the
    oracle, longer ones (b44, b52, b55) with their sub-1e7 pieces.  The
    expected list must hold entries of a sibling j >= 1 and of an edge unit."""
    lib = _lib.lib()
    m, d, s, n = sib_field(base, frac)
    with W.lowered(base) as c:
        if n <= 35_000_000:
            exp, how = want(s, s + n, base, c), "oracle"
        else:
            exp, how = pieces(ctx, s, s + n, base, 9_000_001), "pieces"
        inside = [x - s for x, _ in exp[1] if x - s < 4 * m * d]
        assert any((o // d) % m >= 1 for o in inside), "no expected entry from a sibling j >= 1"
        try:
            for k, L in enumerate(strides):
                assert (d % L == 0) == (k == 0)
                if k:
                    assert d % L >= 5 and any(o % d >= d // L * L for o in inside), f"L {L}: no expected entry in an edge unit"
                assert lib.nice_debug_force_sib_stride(L) == 0
                got = ctx.detailed_raw(s, s + n, base)
                st = ctx.kernel_stats()
                assert (st.sib_lanes, st.sib_stride) == (m, L), st
                same(got, exp, c, f"sibling b{base} at {frac} L {L} ({how})", 100)
        finally:
            lib.nice_debug_force_sib_stride(0)


# --- e. the batch kernel ---------------------------------------------------------------------------
@pytest.mark.parametrize("base", [40, 52, 62, 80])
def test_batch_kernel(ctx, base):
    """fd2_batch_kernel's n0 per range descriptor and the range index of an
    entry: 300 seeded disjoint ranges of 100-400 numbers, 3000-number ranges
    around 20 listed numbers of the 1e6 window, two overlapping ranges that
    share one, shuffled; rows and (n, u, range index) against one oracle call
    per range at the lowered cutoff."""
    s, r1 = O.base_range(base)
    a, e = W.window(base)
    rng = random.Random(500 + base)
    with W.lowered(base) as c:
        listed = want(a, e, base, c)[1]
        assert len(listed) >= 20
        starts = sorted(rng.sample(range(1000), 300))
        ranges = [(s + (r1 - s - 1000) * k // 1000, 0) for k in starts]
        ranges = [(x, x + rng.randrange(100, 401)) for x, _ in ranges]
        # (offsets vary so the entries fall on different steps of their lanes' chunks)
        ranges += [(n - 1400 - 37 * k, n + 1600 - 37 * k) for k, (n, _) in enumerate(listed[::len(listed) // 20][:20])]
        shared = listed[len(listed) // 2][0]
        ranges += [(shared - 1000, shared + 200), (shared - 100, shared + 1500)]
        rng.shuffle(ranges)
        rows_w, list_w = [], []
        for i, (x, y) in enumerate(ranges):
            r = O.process_range_detailed(x, y, base, cutoff=c)
            rows_w.append([0] + [k for _, k in r.distribution])
            list_w += [(n, u, i) for n, u in r.nice_numbers]
        assert len({i for n, _, i in list_w if n == shared}) >= 2, "the shared entry must be listed for both ranges"
        assert len(list_w) >= 22
        rows, lst = ctx.detailed_ranges(ranges, base)
        st = ctx.ranges_stats()
        assert st.fallback_ranges == 0 and st.launches >= 1
        assert rows == rows_w
        assert lst == list_w
        by_range = {}
        for n, u, i in lst:
            assert ranges[i][0] <= n < ranges[i][1]
            by_range.setdefault(i, []).append(n)
        assert all(v == sorted(v) for v in by_range.values()) and [i for _, _, i in lst] == sorted(i for _, _, i in lst)
        assert all(len(by_range.get(i, [])) == sum(rows[i][c + 1:]) for i in range(len(ranges)))
        srow, slst = ctx.detailed_ranges(ranges, base, sum=True)
        assert ctx.ranges_stats().fallback_ranges == 0
        assert srow == [[sum(col) for col in zip(*rows_w)]] and slst == list_w
        assert len(slst) == sum(srow[0][c + 1:])
        print(f"near-miss entries, batch b{base}: {len(lst)} (and again with sum=True)")


# --- f. list growth on an FD field with the in-kernel finish --------------------------------------------
# 1 358 653 numbers above b50's window (1.30 x 2^20, by the oracle) from 0.5 of the range on; the
# rate falls from 1837 per 1e6 at the start of the field to about 1300
GROW_SIZE = 1_075_000_000


def test_list_growth_reruns_the_shard():
    """A fresh context's list holds 2^20 entries.  One b50 field with more
    listed numbers than that overflows it: the host reads the count word, grows
    the list and runs the shard again.  The result must equal its 2.5e7 pieces
    (each far below the capacity), and a second run on the grown list must
    return the same."""
    base = 50
    a = W.at(base, W.WINDOW_FRAC[base])
    c = N.GpuContext(0)
    try:
        with W.lowered(base) as cut:
            first = c.detailed_raw(a, a + GROW_SIZE, base)
            assert len(first[1]) > 2 ** 20
            assert len(first[1]) >= 1.25 * 2 ** 20
            again = c.detailed_raw(a, a + GROW_SIZE, base)
            exp = pieces(c, a, a + GROW_SIZE, base, 25_000_000)
            same(first, exp, cut, "overflow re-run b50 1.075e9", 2 ** 20 + 1)
            same(again, exp, cut, "grown list b50 1.075e9", 2 ** 20 + 1)
    finally:
        c.close()


# --- g. two shards ---------------------------------------------------------------------------------------------
def test_two_shards_keep_the_order():
    """GpuContext([0, 0]): the b57 window, 4e6 numbers, as two shards whose
    lists the host concatenates and orders; with kernel timing on and off."""
    base = 57
    a, _ = W.window(base)
    e = a + 4_000_000
    two = N.GpuContext([0, 0])
    try:
        with W.lowered(base) as c:
            exp = want(a, e, base, c)
            mid = a + (e - a) // 2
            assert any(n < mid for n, _ in exp[1]) and any(n >= mid for n, _ in exp[1])
            same(two.detailed_raw(a, e, base), exp, c, "two shards b57 4e6", W.MIN_ENTRIES)
            two.set_kernel_timing(False)
            same(two.detailed_raw(a, e, base), exp, c, "two shards b57 4e6, untimed", W.MIN_ENTRIES)
    finally:
        two.close()


# --- h. restore, and a field across the range end ------------------------------------------------------------------
def test_restore_and_range_end(ctx):
    """After cutoff = 0 the b40 and b57 windows return the production result;
    under the lowered cutoff a field across the start of b40's range (generic
    and FD launches of one field) lists by the same cutoff in both parts, and
    one across its end equals the oracle too."""
    for base in (40, 57):
        a, e = W.window(base)
        with W.lowered(base) as c:
            assert len(ctx.detailed_raw(a, e, base)[1]) >= W.MIN_ENTRIES
        prod = want(a, e, base)
        assert ctx.detailed_raw(a, e, base) == prod
        assert prod[0] == want(a, e, base, c)[0]
        assert len(prod[1]) == sum(prod[0][O.near_miss_cutoff(base) + 1:])
    r0, r1 = O.base_range(40)
    for x, y, edge in ((r0 - 2_000_000, r0 + 200_000, r0), (r1 - 5000, r1 + 5000, r1)):
        with W.lowered(40) as c:
            exp = want(x, y, 40, c)
            got = ctx.detailed_raw(x, y, 40)
            if edge == r0:
                # listed numbers on both sides of the range start: the generic and the FD part
                assert any(n < edge for n, _ in exp[1]) and any(n >= edge for n, _ in exp[1])
                same(got, exp, c, "b40 range start, generic + FD")
            else:
                # (near the range end n^3 starts 39 39 39 ...: nothing within 5e5 of it has more than
                # 32 unique digits, so this part pins the histogram of the two launches only)
                assert got == exp and sum(got[0]) == y - x
        assert ctx.detailed_raw(x, y, 40) == want(x, y, 40)
