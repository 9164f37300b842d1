"""Batched detailed ranges, the parts that need no GPU: the batch planner
(nice_debug_ranges_plan), the CPU twin (nice_cpu_process_ranges_detailed), the
error codes of both entry points, the Python layer and the base survey.
Expectations come from the oracle or from the per-field CPU call (which
tests/test_cpu_path.py pins to the oracle).
"""
import ctypes
import random

import pytest

import nice_amd as N
from nice_amd import _lib, api, survey
from oracle import oracle as O

MASK = (1 << 64) - 1


def _bounds(ranges):
    flat = []
    for s, e in ranges:
        flat += [s & MASK, s >> 64, e & MASK, e >> 64]
    return (ctypes.c_uint64 * max(4, len(flat)))(*flat)


def plan(base, ranges):
    """[(start, lanes, chunk, range index, combo index)] per workgroup."""
    L = _lib.lib()
    n = ctypes.c_size_t()
    b = _bounds(ranges)
    assert L.nice_debug_ranges_plan(base, b, len(ranges), None, 0, n) == _lib.NICE_OK
    buf = (ctypes.c_uint64 * (6 * max(1, n.value)))()
    cap = n.value
    assert L.nice_debug_ranges_plan(base, b, len(ranges), buf, cap, n) == _lib.NICE_OK and n.value == cap
    return [(buf[6 * i] | (buf[6 * i + 1] << 64), buf[6 * i + 2], buf[6 * i + 3], buf[6 * i + 4], buf[6 * i + 5])
            for i in range(cap)]


def cuts_of(base):
    buf = (ctypes.c_uint64 * 16)()
    n = ctypes.c_size_t()
    assert _lib.lib().nice_fd_segment_cuts(base, buf, 8, n) == 0
    return [buf[2 * i] | (buf[2 * i + 1] << 64) for i in range(n.value)]


def shape_of(base):
    """(WG, chunk) of the base's batch plan: the kernel's workgroup size (the
    lanes of a full workgroup) and its target chunk -- the FD kernel's TCHUNK
    (80 numbers up to b45, 160 up to b58, 240 above) made odd.  A range of
    exactly WG x chunk numbers is one full workgroup of such chunks."""
    s, _ = O.base_range(base)
    wg = plan(base, [(s, s + 10 ** 6)])[0][1]
    chunk = (80 if base <= 45 else 160 if base <= 58 else 240) + 1
    assert plan(base, [(s + 7, s + 7 + wg * chunk)]) == [(s + 7, wg, chunk, 0, 0)]
    return wg, chunk


@pytest.mark.parametrize("base", [40, 50, 62, 80])
def test_plan_tiles_every_range_exactly(base):
    s, e = O.base_range(base)
    cuts = cuts_of(base)
    wg, chunk = shape_of(base)
    assert wg in (512, 1024) and 1 < chunk <= base * base
    rng = random.Random(base)
    ranges = []
    for size in (1, chunk - 1, chunk, chunk + 1, wg - 1, wg, wg + 1, wg * chunk, wg * chunk + 1, 10 ** 6):
        a = rng.randrange(s, e - size)
        ranges.append((a, a + size))
    ranges += [(s, s + 1), (e - 1, e), (s, s + chunk + 1), (e - wg * chunk - 1, e)]
    # the span from the range start to its end, in pieces: 3e5 numbers at the
    # start, at the end and around every cut -- the points where a plan can go
    # wrong.  (The stretches between them are 1e8 workgroups at b40 and do not
    # fit u64 counts at b80: every piece there plans like the seeded ranges.)
    edges = sorted({s, e, *cuts})
    for x in edges:
        lo, hi = max(s, x - 150_000), min(e, x + 150_000)
        ranges.append((lo, hi))
    for c in cuts:
        ranges.append((c - 1000, c + 1000))
    units = plan(base, ranges)
    per = {}
    for u in units:
        per.setdefault(u[3], []).append(u)
    assert sorted(per) == list(range(len(ranges)))
    for ri, (a, b) in enumerate(ranges):
        at = a
        tails = {}
        for n0, lanes, ch, _, combo in per[ri]:
            assert n0 == at, (base, ri)                  # in order, no gap, no overlap
            assert 1 <= lanes <= wg and 1 <= ch <= chunk <= base * base
            end = n0 + lanes * ch
            # no unit crosses a cut; its combo is the cut interval of its last n + 1
            assert not any(n0 < c < end for c in cuts), (base, ri, n0, end)
            assert combo == sum(1 for c in cuts if c < end), (base, ri, n0, end)
            if ch == 1:
                tails[combo] = tails.get(combo, 0) + 1
            at = end
        assert at == b, (base, ri)
        # at most one one-number-per-lane (tail) unit per cut piece
        assert all(v == 1 for v in tails.values()), (base, ri, tails)


def test_plan_rejects_out_of_range_and_non_fd():
    L = _lib.lib()
    n = ctypes.c_size_t()
    s, e = O.base_range(40)
    assert L.nice_debug_ranges_plan(40, _bounds([(s - 1, s + 5)]), 1, None, 0, n) == _lib.NICE_ERR_INVALID
    assert L.nice_debug_ranges_plan(40, _bounds([(e - 1, e + 1)]), 1, None, 0, n) == _lib.NICE_ERR_INVALID
    assert L.nice_debug_ranges_plan(70, _bounds([O.base_range(70)]), 1, None, 0, n) == _lib.NICE_ERR_INVALID
    assert L.nice_debug_ranges_plan(40, _bounds([(s + 5, s + 5)]), 1, None, 0, n) == _lib.NICE_ERR_INVALID


# --- CPU twin ------------------------------------------------------------------
def _one(s, e, base):
    r = N.process_range_detailed_cpu(N.FieldSize(s, e), base)
    return [0] + [d.count for d in r.distribution], [(x.number, x.num_uniques) for x in r.nice_numbers]


@pytest.mark.parametrize("base", [10, 40])
def test_cpu_twin_matches_per_range_calls(base):
    s, e = O.base_range(base)
    rng = random.Random(5 + base)
    if base == 10:
        ranges = [(47, 100), (60, 80), (47, 100), (69, 70), (1_000_000, 1_002_000), (10, 300), (50, 75)]
    else:
        ranges = [(s, s + 300), (e - 200, e), (s - 50, s + 50)]
        a = rng.randrange(s, e - 10 ** 4)
        ranges += [(a, a + 700), (a + 100, a + 900), (a, a + 700)]  # overlapping, repeated
    want = [_one(a, b, base) for a, b in ranges]
    rows, lst = api.detailed_ranges_cpu(ranges, base)
    assert rows == [w[0] for w in want]
    assert all(r[0] == 0 for r in rows)
    assert lst == [(n, u, i) for i, w in enumerate(want) for n, u in w[1]]
    srow, slst = api.detailed_ranges_cpu(ranges, base, sum=True, threads=2)
    assert srow == [[sum(col) for col in zip(*rows)]]
    assert slst == lst
    if base == 10:
        assert (69, 10, 0) in lst and (69, 10, 2) in lst and (69, 10, 3) in lst
        assert [i for n, u, i in lst if n == 69] == [0, 1, 2, 3, 5, 6]
    # the oracle itself, on one range
    o = O.process_range_detailed(*ranges[0], base, cap=ranges[0][1] - ranges[0][0])
    assert [(i, c) for i, c in enumerate(rows[0]) if i] == o.distribution
    assert [(n, u) for n, u, i in lst if i == 0] == o.nice_numbers


def _call_cpu(base, ranges, n_ranges=None, flags=0, cap=64):
    hist = (ctypes.c_uint64 * (129 * max(1, len(ranges))))()
    out = (_lib.nice_number * max(1, cap))()
    idx = (ctypes.c_uint32 * max(1, cap))()
    n = ctypes.c_size_t()
    rc = _lib.lib().nice_cpu_process_ranges_detailed(base, _bounds(ranges), len(ranges) if n_ranges is None else
                                                     n_ranges, flags, 1, hist, out, idx, cap, n)
    return rc, n.value


def _call_gpu_null_ctx(base, ranges, n_ranges=None, flags=0):
    hist = (ctypes.c_uint64 * 129)()
    n = ctypes.c_size_t()
    return _lib.lib().nice_process_ranges_detailed(None, base, _bounds(ranges), len(ranges) if n_ranges is None else
                                                   n_ranges, flags, hist, None, None, 0, n)


def test_error_codes():
    ok = [(47, 100)]
    assert _call_cpu(10, ok) == (_lib.NICE_OK, 1)
    assert _call_cpu(10, ok, n_ranges=0)[0] == _lib.NICE_ERR_INVALID
    assert _call_cpu(10, ok, n_ranges=(1 << 20) + 1)[0] == _lib.NICE_ERR_INVALID
    assert _call_cpu(1, ok)[0] == _lib.NICE_ERR_INVALID
    assert _call_cpu(129, ok)[0] == _lib.NICE_ERR_INVALID
    assert _call_cpu(10, ok, flags=2)[0] == _lib.NICE_ERR_INVALID
    for bad in ((60, 60), (80, 60)):  # empty, inverted: the message names the index
        assert _call_cpu(10, [(47, 100), (50, 60), bad])[0] == _lib.NICE_ERR_INVALID
        assert b"range 2 " in _lib.lib().nice_last_error()
    # a short list: the needed length, then success at that length
    rc, need = _call_cpu(10, [(1_000_000, 1_010_000)], cap=16)
    assert (rc, need) == (_lib.NICE_ERR_CAPACITY, 5395)
    assert _call_cpu(10, [(1_000_000, 1_010_000)], cap=need) == (_lib.NICE_OK, need)
    # the GPU entry point sees bad arguments before it needs a context
    assert _call_gpu_null_ctx(10, ok) == _lib.NICE_ERR_INVALID
    st = _lib.nice_ranges_stats()
    assert _lib.lib().nice_last_ranges_stats(None, st) == _lib.NICE_ERR_INVALID


def test_python_layer_returns_field_results():
    s, _ = O.base_range(40)
    ranges = [N.FieldSize(47, 100), N.FieldSize(60, 80)]
    got = N.process_ranges_detailed_cpu(ranges, 10, threads=2)
    assert got == [N.process_range_detailed_cpu(r, 10) for r in ranges]
    assert N.NiceNumberSimple(69, 10) in got[0].nice_numbers
    r40 = [(s + 10, s + 400), (s + 200, s + 900)]
    got = N.process_ranges_detailed_cpu(r40, 40)
    assert got == [N.process_range_detailed_cpu(N.FieldSize(*r), 40) for r in r40]
    with pytest.raises(N.NiceError):
        N.process_ranges_detailed_cpu([], 40)


# --- survey ----------------------------------------------------------------------
def test_survey_is_stratified_and_deterministic():
    a = survey.survey_base(None, 40, windows=8, window_size=500, seed=1)
    b = survey.survey_base(None, 40, windows=8, window_size=500, seed=1)
    c = survey.survey_base(None, 40, windows=8, window_size=500, seed=2)
    assert a == b and a.windows != c.windows
    s, e = O.base_range(40)
    assert len(a.windows) == 8
    for j, (x, y) in enumerate(a.windows):  # one window per stratum, inside the range
        assert s + (e - s) * j // 8 <= x < s + (e - s) * (j + 1) // 8
        assert s <= x < y <= e and y - x == 500
    assert sum(a.distribution) == 4000 and a.numbers == 4000 and a.distribution[0] == 0
    want = [0] * 41
    for x, y in a.windows:
        for u, cnt in O.process_range_detailed(x, y, 40, cap=y - x).distribution:
            want[u] += cnt
    assert a.distribution == want
    mean = sum(u / 40 * cnt for u, cnt in enumerate(want)) / 4000
    var = sum((u / 40) ** 2 * cnt for u, cnt in enumerate(want)) / 4000 - mean ** 2
    assert a.mean == pytest.approx(mean, rel=1e-12) and a.stdev == pytest.approx(var ** 0.5, rel=1e-9)
    # a window that reaches past the range end is clipped
    w = survey.survey_windows(10, 4, 1000, seed=0)
    assert all(47 <= x < y <= 100 for x, y in w)


def test_survey_cli(capsys):
    import json
    from nice_amd import client
    assert client.main(["--survey", "--base", "40", "--windows", "4", "--window-size", "50", "--seed", "3",
                        "--log-level", "off"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    r = survey.survey_base(None, 40, windows=4, window_size=50, seed=3)
    assert out["distribution"] == r.distribution and out["numbers"] == 200 and out["mean"] == r.mean
