"""GPU tests of the niceonly fast path on the twelve bases that joined
40/50/52/53/54/80 on the list (csrc/niceonly_bases.h): each base's digit path,
its fields through both device paths with the square-survivor count pinned,
the wide (n past 64 bits) lane walk across shards and dealt chunks, and a base
that stays on the run-time-base kernels.

Run on the MI355X box:  python -m pytest tests/test_gpu_niceonly_bases.py -m gpu -q
"""
import functools
import random

import pytest

import nice_amd as N
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NEW = [42, 44, 45, 48, 49, 57, 58, 60, 62, 64, 65, 68]
# window start a = s + K[b] (e - s) // 256: windows with square survivors
# (found on the CPU oracle); b64 has none anywhere, see its test
K = {42: 27, 44: 2, 45: 2, 48: 1, 49: 10, 57: 31, 58: 7, 60: 8, 62: 24, 65: 21, 68: 23, 64: 128}
# (window size, chunk size): 3e6 / 1e6 is the fused per-chunk MSD plus
# niceonly_kernel; 4e7 / 1e7 has chunk / floor = 40 000 > 16 384, so the level
# BFS plus msd_wave_kernel (lane walk, or packed groups on b65 / b68)
WINDOWS = [(3 * 10 ** 6, 10 ** 6), (4 * 10 ** 7, 10 ** 7)]


@pytest.fixture(scope="module")
def ctx():
    c = N.GpuContext(0)
    yield c
    c.close()


def _start(base):
    s, e = O.base_range(base)
    return s + K[base] * (e - s) // 256


@functools.lru_cache(maxsize=None)
def _oracle(a, size, base, chunk):
    res, cands, ranges, sq = O.process_field_niceonly_sq(a, a + size, base, 16, chunk)
    return [n for n, _ in res.nice_numbers], cands, ranges, sq


@pytest.mark.parametrize("base", NEW)
def test_debug_unique_fast_new_bases(ctx, base):
    """unique_fast_kernel<b>: the range ends and 2000 seeded random in-range n
    against the oracle's get_num_unique_digits."""
    rng = random.Random(31 * base)
    s, e = O.base_range(base)
    ns = [s, s + 1, e - 2, e - 1] + [rng.randrange(s, e) for _ in range(2000)]
    assert ctx.debug_unique_fast(ns, base) == [O.num_unique_digits(n, base) for n in ns]


@pytest.mark.parametrize("base", [b for b in NEW if b != 64])
def test_fields_with_square_survivors(ctx, base):
    """Candidates, MSD ranges, square survivors (> 0) and the nice list equal
    the oracle's on a window through each device path."""
    assert N.niceonly_fast_base(base)
    a = _start(base)
    for size, chunk in WINDOWS:
        want, cands, ranges, sq = _oracle(a, size, base, chunk)
        lst, st = ctx.niceonly_raw(a, a + size, base, chunk_size=chunk, msd_where="device")
        print(base, size, (st.candidates, st.ranges, st.square_ok), (cands, ranges, sq))
        assert (st.candidates, st.ranges, st.square_ok) == (cands, ranges, sq), (base, size)
        assert sq > 0
        assert lst == want


def test_b64_field_without_candidates(ctx):
    """Base 64 is the one exception: on a 1/4096 grid of 1e10 windows its MSD
    filter leaves no candidate anywhere, so no window has a square survivor.
    This pins candidates, ranges and the list of a mid-range window through
    both device paths; b64's digit path rests on
    test_debug_unique_fast_new_bases and the CPU hook tests
    (test_niceonly_bases.py)."""
    a = _start(64)
    for size, chunk in WINDOWS:
        want, cands, ranges, sq = _oracle(a, size, 64, chunk)
        lst, st = ctx.niceonly_raw(a, a + size, 64, chunk_size=chunk, msd_where="device")
        assert (st.candidates, st.ranges, st.square_ok) == (cands, ranges, sq), size
        assert lst == want


def test_wide_walk_across_shards_and_deals(ctx):
    """The b57 wave-path window (n past 64 bits: the wide lane walk) beyond a
    single batch: sharded over two contexts' worth of device 0, and dealt two
    ways; candidates, ranges and square survivors sum to the single run's."""
    size, chunk = WINDOWS[1]
    a = _start(57)
    want, cands, ranges, sq = _oracle(a, size, 57, chunk)
    lst, st = ctx.niceonly_raw(a, a + size, 57, chunk_size=chunk, msd_where="device")
    assert (lst, st.candidates, st.ranges, st.square_ok) == (want, cands, ranges, sq)
    two = N.GpuContext([0, 0])
    try:
        l2, s2 = two.niceonly_raw(a, a + size, 57, chunk_size=chunk, msd_where="device")
    finally:
        two.close()
    assert (sorted(l2), s2.candidates, s2.ranges, s2.square_ok) == (want, cands, ranges, sq)
    got, tot = [], [0, 0, 0]
    for r in range(2):
        l3, s3 = ctx.niceonly_raw(a, a + size, 57, chunk_size=chunk, msd_where="device",
                                  deal_stride=2, deal_offset=r)
        got += l3
        tot = [tot[0] + s3.candidates, tot[1] + s3.ranges, tot[2] + s3.square_ok]
    assert (sorted(got), tot) == (want, [cands, ranges, sq])


def test_generic_path_guard(ctx):
    """Base 70 has no FD kernel and stays on the run-time-base kernels (the
    generic wave path that b45 / b62 used to exercise): candidates, ranges and
    the list equal the oracle's, and no square survivors are counted there
    (the oracle has 117)."""
    assert not N.niceonly_fast_base(70)
    s, e = O.base_range(70)
    a = s + 2 * (e - s) // 256
    size, chunk = WINDOWS[1]
    want, cands, ranges, sq = _oracle(a, size, 70, chunk)
    assert (cands, ranges, sq) == (29650, 1967, 117)
    lst, st = ctx.niceonly_raw(a, a + size, 70, chunk_size=chunk, msd_where="device")
    assert (st.candidates, st.ranges) == (cands, ranges)
    assert lst == want
    assert st.square_ok == 0
