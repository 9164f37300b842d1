"""The sound prefix test per caller range (nice_process_ranges_niceonly_ex), the
parts that need no GPU: the CPU twin against the Python restatement of the rule
(sound_restatement.py, per range: ranges_prefix_cases.py), the domain the test
runs on (the leaf plan's fast group), the options' plumbing and the niceonly
survey's prefix column.
"""
import ctypes
import os
import shutil
import subprocess

import pytest

import nice_amd as N
from nice_amd import _lib, api, survey
from oracle import oracle as O

import nice_min_windows as W
import ranges_niceonly_cases as C
import ranges_prefix_cases as P
import sound_restatement as SR

THREADS = W.THREADS
INV = _lib.NICE_ERR_INVALID


@pytest.fixture(autouse=True)
def _restore_filter_c():
    """The oracle's Filter C switch is process-global: later tests rely on 1."""
    yield
    O.lib().oracle_set_filter_c(1)


def groups(base, ranges, k=0):
    """Per range: whether the leaf plan puts it in the fast group (ranges
    without a candidate have no leaf: None)."""
    L = _lib.lib()
    b, nr = api._pack_ranges(ranges)
    n = ctypes.c_size_t()
    assert L.nice_debug_ranges_niceonly_plan(base, k, b, nr, 1, None, 0, n) == _lib.NICE_OK
    buf = (ctypes.c_uint64 * (7 * max(1, n.value)))()
    assert L.nice_debug_ranges_niceonly_plan(base, k, b, nr, 1, buf, n.value, n) == _lib.NICE_OK
    out = [None] * nr
    for i in range(n.value):
        out[buf[7 * i + 4]] = bool(buf[7 * i + 5])
    return out


# --- the sound recursion's leaves -------------------------------------------------------------------
@pytest.mark.parametrize("base", P.BASES)
def test_sound_leaves_of_a_window(base):
    a, size, chunk = W.window(base, "fused")
    leaves = P.window_leaves(base)
    cand, sq, rej = P.columns(leaves, base)
    got = api.niceonly_ranges_ex_cpu(leaves, base, prefix_test=True, threads=THREADS)
    assert got[0] == cand
    assert got[2] == rej
    assert got[1] == sq
    assert got[3] == []
    ranges, cands, n_rej, n_sq, nice = SR.sound_field(a, size, base, chunk)
    assert (len(leaves), sum(got[0]), sum(got[2]), sum(got[1]), got[3]) == (ranges, cands, n_rej, n_sq, nice)
    assert 0 < n_rej < cands and n_sq > 0
    assert all(g in (True, None) for g in groups(base, leaves)), "the test ran on every leaf"
    # off: the plain call, which tests the rejected candidates' squares too
    off = api.niceonly_ranges_ex_cpu(leaves, base, threads=THREADS)
    assert (off[0], off[2], off[3]) == (cand, [0] * len(leaves), [])
    assert all(o >= q for o, q in zip(off[1], sq)) and sum(off[1]) >= n_sq


# --- ranges no recursion hands over ------------------------------------------------------------------
@pytest.mark.parametrize("base", [40, 65])
def test_hand_made_ranges(base):
    ranges, kinds = P.hand_made(base)
    cand, sq, rej = P.check_kinds(base)
    # MSD leaves hold none of these: no one-number leaf, no leaf whose own prefix repeats
    leaves = P.window_leaves(base)
    assert all(e - s > 1 and not P.repeats(SR.leaf_prefix(s, e, base)) for s, e in leaves)
    got = api.niceonly_ranges_ex_cpu(ranges, base, prefix_test=True, threads=THREADS)
    assert got == (cand, sq, rej, [])
    assert api.niceonly_ranges_ex_cpu(ranges, base, prefix_test=True, threads=1) == got
    assert all(g in (True, None) for g in groups(base, ranges))


# --- where the test does not run ---------------------------------------------------------------------
def plain_as_ex(ranges, base, k=0):
    cand, sq, lst = api.niceonly_ranges_cpu(ranges, base, stride_k=k, threads=THREADS)
    return cand, sq, [0] * len(cand), lst


@pytest.mark.parametrize("base", [10, 70, 97])
def test_not_on_a_base_without_a_compile_time_kernel(base):
    ranges = C.range_set(base)
    assert not N.niceonly_fast_base(base) and not any(groups(base, ranges))
    got = api.niceonly_ranges_ex_cpu(ranges, base, prefix_test=True, threads=THREADS)
    assert got == plain_as_ex(ranges, base) and sum(got[0]) > 0


def test_not_on_other_stride_depths_or_outside_the_valid_range():
    s, e = O.base_range(40)
    inside = [(s + 10 ** 9, s + 10 ** 9 + 50_000), (s + 10 ** 9 + 7, s + 10 ** 9 + 9)]
    for k in (1, 3):
        assert not any(groups(40, inside, k))
        got = api.niceonly_ranges_ex_cpu(inside, 40, stride_k=k, prefix_test=True)
        assert got == plain_as_ex(inside, 40, k) and got[0][0] > 0
    # across the valid range's end: the run-time-base test, nothing rejected -- beside a
    # range inside, on which the test runs
    mixed = [(e - 20_000, e + 20_000), (e - 20_000, e)]
    assert groups(40, mixed) == [False, True]
    got = api.niceonly_ranges_ex_cpu(mixed, 40, prefix_test=True)
    plain = plain_as_ex(mixed, 40)
    cand, sq, rej = P.columns([mixed[1]], 40)
    assert (got[0], got[3]) == (plain[0], plain[3])
    assert got[2] == [0, rej[0]] and rej[0] > 0
    assert got[1] == [plain[1][0], sq[0]]


def test_residue_empty_base():
    s, _ = O.base_range(43)
    ranges = [(s, s + 10 ** 5), (1, 1000)]
    assert api.niceonly_ranges_ex_cpu(ranges, 43, prefix_test=True) == ([0, 0], [0, 0], [0, 0], [])


# --- plumbing -------------------------------------------------------------------------------------------
def raw_cpu(base, ranges, opts, cap=64):
    """(rc, candidates, square_ok, prefix_rejected, [(n, range)]) of the C call."""
    L = _lib.lib()
    b, nr = api._pack_ranges(ranges)
    cand, sq, rej = (ctypes.c_uint64 * nr)(), (ctypes.c_uint32 * nr)(), (ctypes.c_uint64 * nr)()
    for i in range(nr):
        rej[i] = 77  # the call overwrites it
    out, idx, n = (_lib.nice_number * max(cap, 1))(), (ctypes.c_uint32 * max(cap, 1))(), ctypes.c_size_t()
    rc = L.nice_cpu_process_ranges_niceonly_ex(base, b, nr, opts, THREADS, cand, sq, rej, out if cap else None,
                                               idx if cap else None, cap, n)
    lst = [(out[i].number_lo | out[i].number_hi << 64, idx[i]) for i in range(min(n.value, cap))]
    return rc, list(cand), list(sq), list(rej), lst, n.value


def test_off_and_null_options_are_the_plain_call():
    for base in (10, 40):
        ranges = C.range_set(base)
        cand, sq, lst = api.niceonly_ranges_cpu(ranges, base, threads=THREADS)
        want = (_lib.NICE_OK, cand, sq, [0] * len(ranges), lst, len(lst))
        assert raw_cpu(base, ranges, None) == want
        assert raw_cpu(base, ranges, _lib.nice_ranges_niceonly_opts(0, _lib.NICE_RANGES_PREFIX_OFF)) == want
        assert raw_cpu(base, ranges, _lib.nice_ranges_niceonly_opts(2, 0)) == want
        assert api.niceonly_ranges_ex_cpu(ranges, base, threads=THREADS) == (cand, sq, [0] * len(ranges), lst)
    assert raw_cpu(10, [(47, 100)], None)[4] == [(69, 0)]
    # the arrays may be null
    L = _lib.lib()
    b, nr = api._pack_ranges([(47, 100)])
    n = ctypes.c_size_t()
    on = _lib.nice_ranges_niceonly_opts(0, 1)
    assert L.nice_cpu_process_ranges_niceonly_ex(10, b, nr, on, 1, None, None, None, None, None, 0, n) == \
        _lib.NICE_ERR_CAPACITY and n.value == 1


def test_invalid_options():
    L = _lib.lib()
    r = [(47, 100)]
    assert raw_cpu(10, r, _lib.nice_ranges_niceonly_opts(0, 2))[0] == INV and b"prefix_test" in L.nice_last_error()
    assert raw_cpu(10, r, _lib.nice_ranges_niceonly_opts(0, 0xffffffff))[0] == INV
    o = _lib.nice_ranges_niceonly_opts(0, 1)
    o.reserved[1] = 5
    assert raw_cpu(10, r, o)[0] == INV and b"reserved" in L.nice_last_error()
    assert raw_cpu(97, [(1, 1000)], _lib.nice_ranges_niceonly_opts(4, 1))[0] == INV
    with pytest.raises(_lib.NiceError):
        api.niceonly_ranges_ex_cpu(r, 10, prefix_test=2)


def test_capacity_error_keeps_prefix_rejected():
    """The CPU twin lists only nice numbers, so its list is b10's 69 -- beside a
    b40 call whose counts must come back with NICE_ERR_CAPACITY too."""
    on = _lib.nice_ranges_niceonly_opts(0, 1)
    rc, cand, sq, rej, lst, n = raw_cpu(10, [(47, 100), (60, 70)], on, cap=1)
    assert (rc, n, rej) == (_lib.NICE_ERR_CAPACITY, 2, [0, 0]) and cand[0] > 0
    assert raw_cpu(10, [(47, 100), (60, 70)], on, cap=2)[4] == [(69, 0), (69, 1)]
    leaves = P.window_leaves(40)[:50]
    want = P.columns(leaves, 40)
    rc, cand, sq, rej, lst, n = raw_cpu(40, leaves, on, cap=0)
    assert (rc, cand, sq, rej, n) == (_lib.NICE_OK, *want, 0) and sum(rej) > 0


# --- the survey ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [40, 65])
def test_survey_prefix_column(base):
    kw = dict(windows=5, window_size=10 ** 5, seed=3, threads=THREADS)
    plain = survey.survey_niceonly_base(None, base, **kw)
    pre = survey.survey_niceonly_base(None, base, prefix_test=True, **kw)
    keys = ["msd_ranges", "msd_numbers", "candidates", "square_ok", "found"]
    assert list(plain.sound.counts()) == keys == list(plain.reference.counts())
    assert plain.sound.prefix_rejected == 0
    assert list(pre.sound.counts()) == keys + ["prefix_rejected"] == list(pre.reference.counts())
    assert pre.reference.counts() == dict(plain.reference.counts(), prefix_rejected=0)
    # the restatement, window by window (a window is one chunk of the recursion)
    want = [SR.sound_field(a, e - a, base, e - a) for a, e in pre.windows]
    ranges, cands, rej, sq = (sum(x[i] for x in want) for i in range(4))
    assert pre.sound.counts() == {"msd_ranges": ranges, "msd_numbers": plain.sound.msd_numbers, "candidates": cands,
                                  "square_ok": sq, "found": 0, "prefix_rejected": rej}
    assert 0 < rej < cands
    # the kept and the rejected make up the plain column's candidates; the plain
    # square_ok also counts rejected candidates whose square happens to be repeat-free
    assert plain.sound.candidates == cands and plain.sound.square_ok >= sq
    assert "prefix_rejected" in pre.scaled("sound") and "prefix_rejected" not in plain.scaled("sound")


# --- the host code under the sanitizers ------------------------------------------------------------
def test_host_code_runs_clean_under_asan_and_ubsan(tmp_path):
    """tests/ranges_prefix_san.cpp: the CPU twin with the test on and off
    (cpu_path.cpp) in a program of its own, built with ASan + UBSan and run as
    it is: no Python, no preload."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "nice_amd", "csrc")
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "ranges_prefix_san")
    r = subprocess.run([cxx, "-std=c++17", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", csrc, os.path.join(root, "tests", "ranges_prefix_san.cpp"),
                        os.path.join(csrc, "cpu_path.cpp"), "-o", exe, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
                                UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0 and "ranges_prefix_san ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
