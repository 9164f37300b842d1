"""GPU tests of the sound niceonly filter (filter="sound"): every fast base
through the fused per-chunk path, the three candidate walks of the wave path,
floor 64, the paths that run without the prefix test, the plumbing (two
devices, dealt chunks, submit / collect beside a reference-mode field), and
the default mode left as it was.

Ranges, candidates and the nice list are the oracle's with Filter C off; the
prefix-rejected and square-survivor counts come from the Python restatement of
the test's definition (sound_restatement.py).

Run on the MI355X box:  python -m pytest tests/test_gpu_sound_filter.py -m gpu -q
"""
import ctypes

import pytest

import nice_amd as N
from nice_amd import _lib
from oracle import oracle as O

import sound_restatement as SR
from test_sound_filter import FAST, start

pytestmark = pytest.mark.gpu

FUSED = (3 * 10 ** 6, 10 ** 6)   # msd_fused_kernel + niceonly_kernel
WAVE = (4 * 10 ** 7, 10 ** 7)    # level BFS + msd_wave_kernel
B40_CHUNK = 1_917_123_264_916


@pytest.fixture(scope="module")
def ctx():
    c = N.GpuContext(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _restore_filter_c():
    """The oracle's Filter C switch is process-global: later tests rely on 1."""
    yield
    O.lib().oracle_set_filter_c(1)


def totals(st):
    return st.ranges, st.candidates, st.prefix_rejected, st.square_ok


def check_field(ctx, a, size, base, chunk, floor=250):
    ranges, cands, rej, sq, want = SR.sound_field(a, size, base, chunk, floor)
    lst, st = ctx.niceonly_raw(a, a + size, base, chunk_size=chunk, msd_floor=floor, msd_where="device",
                               filter="sound")
    print(base, size, floor, totals(st), (ranges, cands, rej, sq))
    assert (st.ranges, st.candidates) == (ranges, cands)
    assert (st.prefix_rejected, st.square_ok) == (rej, sq)
    assert lst == want
    return ranges, cands, rej, sq


@pytest.mark.parametrize("base", FAST)
def test_fused_path_every_fast_base(ctx, base):
    ranges, cands, rej, sq = check_field(ctx, start(base), FUSED[0], base, FUSED[1])
    if base != 64:  # b64 has no candidate anywhere
        assert 0 < rej < cands and sq > 0


@pytest.mark.parametrize("base", [45, 57, 65])
def test_wave_path_each_walk(ctx, base):
    """b45: the narrow lane walk, b57: the wide one, b65: packed groups."""
    ranges, cands, rej, sq = check_field(ctx, start(base), WAVE[0], base, WAVE[1])
    assert 0 < rej < cands and sq > 0


def test_floor_64(ctx):
    got = check_field(ctx, B40_CHUNK, 10 ** 6, 40, 10 ** 6, floor=64)
    assert got == (2630, 25717, 21989, 242)


def test_default_mode_unchanged(ctx):
    lst, st = ctx.niceonly_raw(B40_CHUNK, B40_CHUNK + 10 ** 6, 40, chunk_size=10 ** 6, msd_where="device")
    res, cands, ranges, sq = O.process_field_niceonly_sq(B40_CHUNK, B40_CHUNK + 10 ** 6, 40, 16, 10 ** 6)
    assert (st.ranges, st.candidates) == (281, 11111) == (ranges, cands)
    assert (st.square_ok, st.prefix_rejected) == (sq, 0)
    assert lst == [n for n, _ in res.nice_numbers]
    l2, s2 = ctx.niceonly_raw(B40_CHUNK, B40_CHUNK + 10 ** 6, 40, chunk_size=10 ** 6, msd_where="device",
                              filter="reference")
    assert (l2, totals(s2)) == (lst, totals(st))


def oracle_sound(a, size, base, chunk):
    O.lib().oracle_set_filter_c(0)
    res, cands, ranges, _ = O.process_field_niceonly_sq(a, a + size, base, 16, chunk)
    return ranges, cands, [n for n, _ in res.nice_numbers]


def test_generic_base_runs_without_the_prefix_test(ctx):
    """Base 70 (run-time-base kernels), the window of test_generic_path_guard."""
    s, e = O.base_range(70)
    a = s + 2 * (e - s) // 256
    ranges, cands, want = oracle_sound(a, WAVE[0], 70, WAVE[1])
    lst, st = ctx.niceonly_raw(a, a + WAVE[0], 70, chunk_size=WAVE[1], msd_where="device", filter="sound")
    assert (st.ranges, st.candidates, lst) == (ranges, cands, want)
    assert ranges > 1967  # more than with Filter C
    assert (st.prefix_rejected, st.square_ok) == (0, 0)
    # and through the fused path
    ranges, cands, want = oracle_sound(a, FUSED[0], 70, FUSED[1])
    lst, st = ctx.niceonly_raw(a, a + FUSED[0], 70, chunk_size=FUSED[1], msd_where="device", filter="sound")
    assert (st.ranges, st.candidates, lst, st.prefix_rejected) == (ranges, cands, want, 0)


def test_host_msd_runs_without_the_prefix_test(ctx):
    a = start(45)
    ranges, cands, _, _, want = SR.sound_field(a, FUSED[0], 45, FUSED[1])
    lst, st = ctx.niceonly_raw(a, a + FUSED[0], 45, chunk_size=FUSED[1], msd_where="host", filter="sound")
    assert (st.ranges, st.candidates, lst) == (ranges, cands, want)
    assert st.prefix_rejected == 0


def test_out_of_range_and_small_bases(ctx):
    """b10 [47, 100) still returns 69; a fast base's field that leaves its
    range runs without the prefix test."""
    lst, st = ctx.niceonly_raw(47, 100, 10, filter="sound")
    assert lst == [69] and st.prefix_rejected == 0
    s, e = O.base_range(40)
    a = e - 10 ** 6
    ranges, cands, want = oracle_sound(a, 2 * 10 ** 6, 40, 10 ** 6)
    lst, st = ctx.niceonly_raw(a, a + 2 * 10 ** 6, 40, chunk_size=10 ** 6, msd_where="device", filter="sound")
    assert (st.ranges, st.candidates, lst, st.prefix_rejected) == (ranges, cands, want, 0)


def test_two_devices_and_dealt_chunks(ctx):
    """The b57 wave window over two contexts' worth of device 0 and dealt two
    ways: totals, prefix_rejected included, equal the single run's."""
    a = start(57)
    ranges, cands, rej, sq, want = SR.sound_field(a, WAVE[0], 57, WAVE[1])
    two = N.GpuContext([0, 0])
    try:
        l2, s2 = two.niceonly_raw(a, a + WAVE[0], 57, chunk_size=WAVE[1], msd_where="device", filter="sound")
    finally:
        two.close()
    assert (sorted(l2), totals(s2)) == (want, (ranges, cands, rej, sq))
    got, tot = [], (0, 0, 0, 0)
    for r in range(2):
        l3, s3 = ctx.niceonly_raw(a, a + WAVE[0], 57, chunk_size=WAVE[1], msd_where="device", filter="sound",
                                  deal_stride=2, deal_offset=r)
        got += l3
        tot = tuple(x + y for x, y in zip(tot, totals(s3)))
    assert (sorted(got), tot) == (want, (ranges, cands, rej, sq))


def test_submit_collect_beside_a_reference_field(ctx):
    a = start(45)
    ranges, cands, rej, sq, want = SR.sound_field(a, FUSED[0], 45, FUSED[1])
    opts = dict(chunk_size=FUSED[1], msd_where="device")
    ref_l, ref_s = ctx.niceonly_raw(a, a + FUSED[0], 45, **opts)
    t_sound = ctx.niceonly_submit(a, a + FUSED[0], 45, filter="sound", **opts)
    t_ref = ctx.niceonly_submit(a, a + FUSED[0], 45, **opts)
    l1, s1 = ctx.niceonly_collect(t_ref)
    l0, s0 = ctx.niceonly_collect(t_sound)
    assert (l1, totals(s1)) == (ref_l, totals(ref_s)) and s1.prefix_rejected == 0
    assert (l0, totals(s0)) == (want, (ranges, cands, rej, sq))
    r = N.process_range_niceonly_gpu(ctx, N.FieldSize(a, a + FUSED[0]), 45, filter="sound", **opts)
    assert [x.number for x in r.nice_numbers] == want


def test_bad_filter_is_refused_at_submit(ctx):
    opts = _lib.nice_niceonly_opts(0, 0, 0, 0, 0, 0, 0, 2)
    t = ctypes.c_int()
    rc = _lib.lib().nice_niceonly_submit(ctx._h, 47, 0, 100, 0, 10, opts, t)
    assert rc == _lib.NICE_ERR_INVALID
    st = _lib.nice_niceonly_stats()
    n = ctypes.c_size_t()
    out = (_lib.nice_number * 4)()
    rc = _lib.lib().nice_process_range_niceonly_ex(ctx._h, 47, 0, 100, 0, 10, opts, out, 4, n, st)
    assert rc == _lib.NICE_ERR_INVALID
