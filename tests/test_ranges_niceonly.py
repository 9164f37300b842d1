"""Batched niceonly ranges, the parts that need no GPU: the CPU twin
(nice_cpu_process_ranges_niceonly) against the oracle's primitives, the leaf
plan (nice_debug_ranges_niceonly_plan), the error codes and empty answers, the
Python layer and the niceonly survey's arithmetic.  The range sets and their
expectations are ranges_niceonly_cases.py's, shared with the GPU tests.
"""
import bisect
import ctypes
import json
import os
import shutil
import subprocess

import pytest

import nice_amd as N
from nice_amd import _lib, api, client, survey
from oracle import oracle as O

import ranges_niceonly_cases as C

MASK = (1 << 64) - 1
LEAF_PIECE = 1 << 28  # kLeafPiece (layout.h)
BASES = [10, 12, 25, 40, 45, 50, 60, 62, 80, 97]


def _bounds(ranges):
    flat = []
    for s, e in ranges:
        flat += [s & MASK, s >> 64, e & MASK, e >> 64]
    return (ctypes.c_uint64 * max(4, len(flat)))(*flat)


def plan(base, ranges, n_devices=1, k=0):
    """[(b0, g0, count, range index, group, device)] per leaf."""
    L = _lib.lib()
    n = ctypes.c_size_t()
    b = _bounds(ranges)
    assert L.nice_debug_ranges_niceonly_plan(base, k, b, len(ranges), n_devices, None, 0, n) == _lib.NICE_OK
    cap = n.value
    buf = (ctypes.c_uint64 * (7 * max(1, cap)))()
    assert L.nice_debug_ranges_niceonly_plan(base, k, b, len(ranges), n_devices, buf, cap, n) == _lib.NICE_OK
    assert n.value == cap
    return [(buf[7 * i] | (buf[7 * i + 1] << 64), *buf[7 * i + 2:7 * i + 7]) for i in range(cap)]


# --- the CPU twin against the oracle's primitives ------------------------------------------------
@pytest.mark.parametrize("base", BASES)
def test_cpu_twin_matches_the_oracle(base):
    ranges = C.range_set(base)
    cand, sq, lst = C.expected(base)
    assert sum(cand) > 1000 and 0 in cand and 1 in cand and len(ranges) % 8
    assert cand == [C.count_candidates(s, e, base) for s, e in ranges]
    if base >= 60 and base <= 64:
        assert any(e >> 64 for _, e in ranges), "n passes 64 bits"
    got = api.niceonly_ranges_cpu(ranges, base, threads=3)
    assert got[0] == cand and got[1] == sq and got[2] == lst
    assert api.niceonly_ranges_cpu(ranges, base, threads=1) == got
    # repeated ranges answer alike, each completely
    assert ranges[-1] == ranges[-2] and cand[-1] == cand[-2] and sq[-1] == sq[-2]


def test_set_has_the_g0_equals_R_case():
    """A start whose residue lies above the table's last: on the bases whose
    last residue is not M - 1."""
    with_case = []
    for base in BASES:
        M, res = C.table(base)
        if any(s % M > res[-1] for s, _ in C.range_set(base)):
            with_case.append(base)
    assert len(with_case) >= 3, with_case
    for base in with_case:
        M, res = C.table(base)
        s, e = next(r for r in C.range_set(base) if r[0] % M == res[-1] + 1)
        (leaf,) = plan(base, [(s, e)])
        assert leaf[1] == len(res) and leaf[0] == s - s % M and leaf[2] == C.count_candidates(s, e, base) > 0


def test_b10_lists_69():
    cand, sq, lst = api.niceonly_ranges_cpu([(47, 100)], 10)
    assert lst == [(69, 0)] and cand == [len(C.candidates(47, 100, 10))]
    (r,) = N.process_ranges_niceonly_cpu([N.FieldSize(47, 100)], 10)
    assert [(x.number, x.num_uniques) for x in r.nice_numbers] == [(69, 10)] and r.distribution == []
    # a number inside two ranges is listed twice; out_range names each
    cand, sq, lst = api.niceonly_ranges_cpu([(47, 100), (1000, 2000), (60, 70)], 10)
    assert lst == [(69, 0), (69, 2)] and cand[1] == len(C.candidates(1000, 2000, 10))


@pytest.mark.parametrize("k", [1, 3])
def test_other_stride_depths(k):
    base = 12
    s, e = O.base_range(base)
    ranges = [(1, 3000), (s, e), (10 ** 5, 10 ** 5 + 40_000), (7, 8)]
    want = C.expected_of(ranges, base, k)
    assert sum(want[0]) > 100 and want[2]
    assert api.niceonly_ranges_cpu(ranges, base, stride_k=k) == want
    assert want[0] != C.expected_of(ranges, base, 2)[0], "another table, another candidate set"


# --- the leaf plan ---------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [10, 40, 62, 80, 97])
def test_plan_leaves_sum_to_the_candidates(base):
    ranges = C.range_set(base)
    M, res = C.table(base)
    leaves = plan(base, ranges)
    per = [0] * len(ranges)
    for b0, g0, count, ri, group, dev in leaves:
        assert 0 < count <= LEAF_PIECE and b0 % M == 0 and g0 <= len(res) and dev == 0
        per[ri] += count
        s, e = ranges[ri]
        assert group == (1 if N.niceonly_fast_base(base) and C.in_range((s, e), base) else 0)
        # a one-leaf range: the cycle base and stride index of its start
        if count == C.count_candidates(s, e, base):
            assert (b0, g0) == (s - s % M, bisect.bisect_left(res, s % M))
    assert per == [C.count_candidates(s, e, base) for s, e in ranges]
    groups = [l[4] for l in leaves]
    assert groups == sorted(groups, reverse=True), "the fast group first"
    if N.niceonly_fast_base(base):
        assert 0 < sum(groups) < len(groups), "both groups in one call"
    for g in (0, 1):
        idx = [l[3] for l in leaves if l[4] == g]
        assert idx == sorted(idx), "range order inside a group"


def test_plan_splits_long_ranges_into_pieces():
    """b40, 4e9 numbers: more than 2^28 candidates, so the range is several
    leaves, each continuing where the one before ended."""
    base = 40
    M, res = C.table(base)
    R = len(res)
    s, _ = O.base_range(base)
    a, e = s + 12345, s + 12345 + 4 * 10 ** 9
    total = C.count_candidates(a, e, base)
    assert total > LEAF_PIECE
    leaves = plan(base, [(a, a + 1000), (a, e), (e, e + 1000)])
    mine = [l for l in leaves if l[3] == 1]
    assert len(mine) == -(-total // LEAF_PIECE) >= 2
    assert [l[2] for l in mine] == [LEAF_PIECE] * (len(mine) - 1) + [total - LEAF_PIECE * (len(mine) - 1)]
    g = a // M * R + bisect.bisect_left(res, a % M)  # global stride index of the first candidate
    for b0, g0, count, *_ in mine:
        assert (b0, g0) == (g // R * M, g % R)
        g += count
    assert all(l[4] == 1 for l in leaves)


@pytest.mark.parametrize("nd", [1, 2, 8])
def test_plan_deals_each_group_in_balanced_contiguous_runs(nd):
    base = 40
    ranges = C.range_set(base)
    leaves = plan(base, ranges, nd)
    assert len(ranges) % 8 and [l[:5] for l in leaves] == [l[:5] for l in plan(base, ranges, 1)]
    for g in (0, 1):
        mine = [l for l in leaves if l[4] == g]
        devs = [l[5] for l in mine]
        assert devs == sorted(devs) and max(devs) < nd, "contiguous runs"
        total = sum(l[2] for l in mine)
        biggest = max(l[2] for l in mine)
        for d in range(nd):
            load = sum(l[2] for l in mine if l[5] == d)
            assert abs(load - total / nd) <= biggest, (g, d, load, total / nd, biggest)


# --- errors and empty answers ------------------------------------------------------------------------
def _call(base, ranges, k=0, cap=64, n_ranges=None, gpu_ctx=None):
    L = _lib.lib()
    nr = len(ranges) if n_ranges is None else n_ranges
    cand = (ctypes.c_uint64 * max(1, nr))()
    sq = (ctypes.c_uint32 * max(1, nr))()
    out, idx, n = (_lib.nice_number * max(1, cap))(), (ctypes.c_uint32 * max(1, cap))(), ctypes.c_size_t()
    rc = L.nice_cpu_process_ranges_niceonly(base, _bounds(ranges), nr, k, 1, cand, sq, out, idx, cap, n)
    return rc, list(cand), list(sq), [(out[i].number_lo | out[i].number_hi << 64, idx[i]) for i in
                                       range(min(n.value, cap))], n.value


def _plan_rc(base, ranges, k=0, n_ranges=None):
    n = ctypes.c_size_t()
    return _lib.lib().nice_debug_ranges_niceonly_plan(base, k, _bounds(ranges), len(ranges) if n_ranges is None
                                                      else n_ranges, 1, None, 0, n)


@pytest.mark.parametrize("call", [lambda *a, **kw: _call(*a, **kw)[0], _plan_rc], ids=["cpu", "plan"])
def test_invalid_arguments(call):
    INV = _lib.NICE_ERR_INVALID
    ok = [(47, 100)]
    assert call(10, ok) == _lib.NICE_OK
    assert call(10, ok, n_ranges=0) == INV
    assert call(10, ok, n_ranges=(1 << 20) + 1) == INV and b"n_ranges" in _lib.lib().nice_last_error()
    for bad in ((100, 100), (100, 47)):
        assert call(10, ok + [bad]) == INV
        assert b"range 1 is empty or inverted" in _lib.lib().nice_last_error()
    # more than 2^40 candidates in one range: that is a field
    assert call(10, ok + ok + [(1, 1 << 60)]) == INV
    msg = _lib.lib().nice_last_error()
    assert b"range 2" in msg and b"2^40" in msg
    # the stride modulus must fit a u32: b97 k = 4 is 96 * 97^4 > 2^32
    assert call(97, [(1, 1000)], k=4) == INV and b"modulus" in _lib.lib().nice_last_error()
    assert call(97, [(1, 1000)], k=40) == INV
    for base in (0, 1, 129, 1000):
        assert call(base, ok) == INV and b"base" in _lib.lib().nice_last_error()


def test_capacity_and_retry():
    ranges = [(1, 600), (47, 100)]
    rc, cand, sq, lst, n = _call(10, ranges, cap=4096)
    assert rc == _lib.NICE_OK and n == len(lst) > 4
    rc2, cand2, sq2, part, n2 = _call(10, ranges, cap=3)
    assert rc2 == _lib.NICE_ERR_CAPACITY and n2 == n and (cand2, sq2) == (cand, sq)
    assert _call(10, ranges, cap=n) == (rc, cand, sq, lst, n)
    # the Python layer retries with room on its own
    assert api.niceonly_ranges_cpu(ranges, 10, cap=1)[2] == lst


def test_residue_empty_base_answers_zeros():
    s, _ = O.base_range(43)
    assert O.residue_filter(43) == []
    ranges = [(s, s + 10 ** 5), (1, 1000)]
    rc, cand, sq, lst, n = _call(43, ranges)
    assert (rc, cand, sq, lst, n) == (_lib.NICE_OK, [0, 0], [0, 0], [], 0)
    assert plan(43, ranges) == []
    assert N.process_ranges_niceonly_cpu(ranges, 43) == [N.FieldResults([], []), N.FieldResults([], [])]


# --- the survey's arithmetic ----------------------------------------------------------------------
def whole_range(base):
    s, e = O.base_range(base)
    ns = C.candidates(s, e, base)
    return e - s, len(ns), sum(1 for n in ns if C.square_free(n, base)), [n for n in ns if O.is_nice(n, base)]


@pytest.mark.parametrize("base", [10, 25])
def test_survey_of_the_whole_range_equals_the_unsampled_counts(base):
    """One window per number of the range (every stratum holds one number, so
    the windows are the range, each number once): the MSD filter has nothing
    to split, both filters see every candidate, and the scaled figures are the
    counts themselves."""
    size, cands, sq, nice = whole_range(base)
    r = survey.survey_niceonly_base(None, base, windows=size, window_size=1, threads=4)
    assert r.sampled == r.range_size == size and len(r.windows) == size
    for f in (r.reference, r.sound):
        assert f.counts() == {"msd_ranges": size, "msd_numbers": size, "candidates": cands, "square_ok": sq,
                              "found": len(nice)}
        assert f.found == nice
    assert r.scaled("reference") == dict({k: float(v) for k, v in r.reference.counts().items()}, sampled=float(size))
    if base == 10:
        assert nice == [69]


def test_survey_samples_and_scales():
    """Sampled windows: each filter's figures are the sums over its own MSD
    ranges, the sound filter keeps at least the reference's, and scaling is
    count * range / sampled."""
    base = 40
    r = survey.survey_niceonly_base(None, base, windows=6, window_size=50_000, seed=3, threads=4)
    assert r.windows == survey.survey_windows(base, 6, 50_000, 3) and r.sampled == 300_000
    for which in ("reference", "sound"):
        f = getattr(r, which)
        ranges = [(x.range_start, x.range_end) for s, e in r.windows
                  for x in api.get_valid_ranges(N.FieldSize(s, e), base, 250, which)]
        cand, sq, lst = api.niceonly_ranges_cpu(ranges, base)
        assert (f.msd_ranges, f.msd_numbers) == (len(ranges), sum(e - s for s, e in ranges))
        assert (f.candidates, f.square_ok, f.found) == (sum(cand), sum(sq), [n for n, _ in lst])
        assert f.candidates == sum(C.count_candidates(s, e, base) for s, e in ranges)
        sc = r.scaled(which)
        assert sc["candidates"] == f.candidates * r.range_size / r.sampled and sc["sampled"] == r.range_size
    assert r.sound.msd_numbers >= r.reference.msd_numbers > 0 and r.sound.candidates >= r.reference.candidates


def test_cli_survey_niceonly(capsys):
    assert client.main(["--survey-niceonly", "--base", "10", "--windows", "53", "--window-size", "1",
                        "--log-level", "off"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["base"] == 10 and out["sampled"] == 53 and out["reference"]["numbers_found"] == ["69"]
    assert out["sound"]["candidates"] == out["reference"]["candidates"] == len(C.candidates(47, 100, 10))
    # --survey keeps its own default window, whatever the positional mode
    a = client.parse_args(["niceonly", "--survey", "--base", "10"])
    assert a.survey and not a.survey_niceonly and a.window_size == 100_000
    assert client.parse_args(["--survey-niceonly", "--base", "10"]).window_size == 1_000_000


# --- the host code under the sanitizers ------------------------------------------------------------
def test_host_code_runs_clean_under_asan_and_ubsan(tmp_path):
    """tests/ranges_niceonly_san.cpp: the plan header and the CPU twin
    (cpu_path.cpp) in a program of their own, built with ASan + UBSan (as
    scripts/sanitize.sh builds it) and run as it is: no Python, no preload."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "nice_amd", "csrc")
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "ranges_niceonly_san")
    r = subprocess.run([cxx, "-std=c++17", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", csrc, os.path.join(root, "tests", "ranges_niceonly_san.cpp"),
                        os.path.join(csrc, "cpu_path.cpp"), "-o", exe, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
                                UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0 and "ranges_niceonly_san ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
