"""The per-number unique-count map, the parts that need no GPU: the CPU twin
(nice_cpu_unique_map) against the oracle number by number, the launch plan
(nice_debug_map_plan), the argument errors, the Python layer and the host code
under the sanitizers (tests/map_san.cpp).
"""
import ctypes
import functools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from nice_amd import _lib, api, client, survey
from oracle import oracle as O

MASK = (1 << 64) - 1
FD, GENERIC = 0, 1


@functools.lru_cache(maxsize=None)
def oracle_map(a, b, base):
    """The oracle's count of every n in [a, b), computed once per range."""
    return bytes(O.num_unique_digits(n, base) for n in range(a, b))


def cuts_of(base):
    buf = (ctypes.c_uint64 * 16)()
    n = ctypes.c_size_t()
    assert _lib.lib().nice_fd_segment_cuts(base, buf, 8, n) == 0
    return [buf[2 * i] | (buf[2 * i + 1] << 64) for i in range(n.value)]


def plan(base, s, e):
    """[(kind, first n, offset, lanes, chunk, combo, count)] per record."""
    L = _lib.lib()
    n = ctypes.c_size_t()
    args = (base, s & MASK, s >> 64, e & MASK, e >> 64)
    assert L.nice_debug_map_plan(*args, None, 0, n) == _lib.NICE_OK
    cap = n.value
    buf = (ctypes.c_uint64 * (8 * max(1, cap)))()
    assert L.nice_debug_map_plan(*args, buf, cap, n) == _lib.NICE_OK and n.value == cap
    return [(buf[8 * i], buf[8 * i + 1] | (buf[8 * i + 2] << 64), *buf[8 * i + 3:8 * i + 8]) for i in range(cap)]


# --- the CPU twin against the oracle ----------------------------------------------------
def _cpu_cases():
    s40, e40 = O.base_range(40)
    s50, _ = O.base_range(50)
    s70, _ = O.base_range(70)
    s80, _ = O.base_range(80)
    return [(10, 47, 100), (40, s40, s40 + 2000), (80, s80, s80 + 2000), (70, s70 + 12345, s70 + 12345 + 2000),
            (40, e40 - 150, e40 + 150), (50, s50 - 150, s50 + 150)]


@pytest.mark.parametrize("base,a,b", _cpu_cases())
def test_cpu_map_equals_oracle(base, a, b):
    want = oracle_map(a, b, base)
    for threads in (1, 3):
        got = api.unique_map_cpu(a, b, base, threads)
        assert got.dtype == np.uint8 and got.tobytes() == want, (base, threads)
    if base == 10:
        assert got[69 - 47] == 10 and got.max() == 10


# --- the plan ---------------------------------------------------------------------------
def check_plan(base, s, e, wg_max):
    """The records tile [s, e) exactly once, in order, each at offset first n - s;
    an FD record lies inside the valid range and inside one cut interval, whose
    index it carries; everything outside the valid range is generic."""
    rs, re = O.base_range(base)
    cuts = cuts_of(base)
    recs = plan(base, s, e)
    at = s
    for kind, lo, off, lanes, chunk, combo, count in recs:
        assert lo == at and off == lo - s and count >= 1, (base, s, e, lo)
        if kind == FD:
            assert 1 <= lanes <= wg_max and 1 <= chunk <= base * base and count == lanes * chunk
            assert rs <= lo and lo + count <= re
            # the limb layout of a segment is that of its END: cut interval i holds ends in (cuts[i-1], cuts[i]]
            assert combo == sum(1 for c in cuts if c < lo + count), (base, lo, count)
            assert all(not (lo < c < lo + count) for c in cuts)
        else:
            assert kind == GENERIC and (lanes, chunk) == (0, 0)
            assert lo + count <= rs or lo >= re or not _lib.lib().nice_fd_kernel_base(base)
        at = lo + count
    assert at == e
    starts = {r[1] for r in recs}
    for c in cuts + [rs, re]:
        if s < c < e:
            assert c in starts, (base, c)
    return recs


FD_BASES = [b for b in range(2, 129) if _lib.lib().nice_fd_kernel_base(b) == 1]


@pytest.mark.parametrize("base", FD_BASES)
def test_plan_tiles_the_range(base):
    """Every base with an FD kernel; among them one per shape: b40 and b50
    (low-digit table, 512 threads), b64 (side carry table, 1024 threads), b80
    (three mask words, n above 64 bits: the descriptors' digits feed init_at).
    The workgroup size is the plan's own: the lanes of a full workgroup."""
    assert {40, 50, 64, 80} <= set(FD_BASES) and len(FD_BASES) == 24
    rs, re = O.base_range(base)
    cuts = cuts_of(base)
    assert len(cuts) <= 2 and (cuts or base not in (40, 50, 80))  # (b64, for one, has one limb layout and no cut)
    wg = max(r[3] for r in plan(base, rs, rs + 10 ** 6))
    assert wg in (512, 1024)
    if base in (40, 50, 64, 80):
        assert wg == (1024 if base == 64 else 512)
    sizes = (1, 63, 64 * 80 + 1, 100_003)
    for size in sizes:
        recs = check_plan(base, rs, rs + size, wg)
        assert all(r[0] == FD for r in recs)
        check_plan(base, rs + (re - rs) // 3 + 5, rs + (re - rs) // 3 + 5 + size, wg)
        check_plan(base, re - size, re, wg)
    # a range of several full workgroups uses all their lanes, and at most one tail workgroup
    recs = check_plan(base, rs, rs + 3 * wg * 241 + 17, wg)
    assert max(r[3] for r in recs) == wg and sum(1 for r in recs if r[4] == 1) <= 1
    for c in cuts:
        recs = check_plan(base, c - 300, c + 300, wg)
        assert {r[5] for r in recs} == {cuts.index(c), cuts.index(c) + 1}
    # FD -> generic and generic -> FD inside one call
    recs = check_plan(base, re - 150, re + 150, wg)
    assert recs[-1][0] == GENERIC and recs[-1][1:3] == (re, 150) and recs[-1][6] == 150 and recs[0][0] == FD
    recs = check_plan(base, rs - 150, rs + 150, wg)
    assert recs[0][0] == GENERIC and recs[0][6] == 150 and recs[1][0] == FD
    assert [r[0] for r in check_plan(base, re + 7, re + 5000, wg)] == [GENERIC]


def test_plan_of_a_base_without_fd_kernel():
    s, e = O.base_range(70)
    assert plan(70, s + 5, s + 10_012) == [(GENERIC, s + 5, 0, 0, 0, 0, 10_007)]
    assert plan(10, 47, 100) == [(GENERIC, 47, 0, 0, 0, 0, 53)]


# --- argument errors --------------------------------------------------------------------
def _invalid_cases():
    s, _ = O.base_range(40)
    return [(40, s + 5, s + 5), (40, s + 9, s + 5), (1, 47, 100), (129, 47, 100), (40, s, s + (1 << 32) + 1)]


def test_cpu_map_argument_errors():
    L = _lib.lib()
    buf = np.full(64, 0xEE, dtype=np.uint8)
    for base, a, b in _invalid_cases():
        rc = L.nice_cpu_unique_map(a & MASK, a >> 64, b & MASK, b >> 64, base, 1, buf.ctypes.data, buf.size)
        assert rc == _lib.NICE_ERR_INVALID, (base, a, b)
    assert L.nice_cpu_unique_map(47, 0, 100, 0, 10, 1, None, 64) == _lib.NICE_ERR_INVALID
    # too short: nothing is written
    assert L.nice_cpu_unique_map(47, 0, 100, 0, 10, 1, buf.ctypes.data, 52) == _lib.NICE_ERR_CAPACITY
    assert (buf == 0xEE).all()
    assert L.nice_cpu_unique_map(47, 0, 100, 0, 10, 1, buf.ctypes.data, 53) == _lib.NICE_OK
    assert buf[:53].tobytes() == oracle_map(47, 100, 10) and (buf[53:] == 0xEE).all()
    with pytest.raises(_lib.NiceError):
        api.unique_map_cpu(100, 47, 10)


def test_plan_and_gpu_entry_argument_errors():
    L = _lib.lib()
    n = ctypes.c_size_t()
    for base, a, b in _invalid_cases():
        assert L.nice_debug_map_plan(base, a & MASK, a >> 64, b & MASK, b >> 64, None, 0, n) == _lib.NICE_ERR_INVALID
    assert L.nice_debug_map_plan(10, 47, 0, 100, 0, None, 0, None) == _lib.NICE_ERR_INVALID
    assert L.nice_debug_map_plan(10, 47, 0, 100, 0, None, 4, n) == _lib.NICE_ERR_INVALID
    # exactly 2^32 numbers are allowed
    s, _ = O.base_range(40)
    e = s + (1 << 32)
    assert L.nice_debug_map_plan(40, s & MASK, s >> 64, e & MASK, e >> 64, None, 0, n) == _lib.NICE_OK
    # no context
    buf = np.full(64, 0xEE, dtype=np.uint8)
    assert L.nice_unique_map(None, 47, 0, 100, 0, 10, buf.ctypes.data, 64, 0, 0) == _lib.NICE_ERR_INVALID
    assert L.nice_last_map_stats(None, _lib.nice_map_stats()) == _lib.NICE_ERR_INVALID
    assert (buf == 0xEE).all()


# --- the Python layer -------------------------------------------------------------------
def test_class_distribution_cpu():
    """b10 over its whole range, one window per number: the table by n mod 9
    sums over the classes to survey_base's distribution and holds each number
    in its own class."""
    table = survey.class_distribution(None, 10, 9, windows=53, window_size=1, seed=3)
    assert len(table) == 9 and all(len(row) == 11 for row in table)
    want = [[0] * 11 for _ in range(9)]
    for n in range(47, 100):
        want[n % 9][O.num_unique_digits(n, 10)] += 1
    assert table == want
    r = survey.survey_base(None, 10, windows=53, window_size=1, seed=3)
    assert [sum(row[u] for row in table) for u in range(11)] == r.distribution
    # windows longer than one number, a base with an FD kernel
    s, _ = O.base_range(40)
    table = survey.class_distribution(None, 40, 39, windows=5, window_size=400, seed=1)
    w = survey.survey_windows(40, 5, 400, 1)
    want = [[0] * 41 for _ in range(39)]
    for a, b in w:
        for n, u in zip(range(a, b), oracle_map(a, b, 40)):
            want[n % 39][u] += 1
    assert table == want
    with pytest.raises(ValueError):
        survey.class_distribution(None, 10, 0)


def test_cli_survey_classes_and_map(capsys, tmp_path):
    assert client.main(["--survey-classes", "9", "--base", "10", "--windows", "53", "--window-size", "1",
                        "--log-level", "off"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["base"] == 10 and out["modulus"] == 9 and out["numbers"] == 53
    assert out["table"][69 % 9][10] == 1 and sum(row[10] for row in out["table"]) == 1
    path = str(tmp_path / "m.npy")
    assert client.main(["--map", path, "--base", "10", "--range", "47", "100", "--log-level", "off"]) == 0
    m = np.load(path)
    assert m.dtype == np.uint8 and m.tobytes() == oracle_map(47, 100, 10)
    assert client.main(["--map", path, "--base", "10", "--log-level", "off"]) == 2


# --- the host code under the sanitizers -------------------------------------------------
def test_host_code_runs_clean_under_asan_and_ubsan(tmp_path):
    """tests/map_san.cpp: the plan header and the CPU twin (cpu_path.cpp) in a
    program of their own, built with ASan + UBSan (as scripts/sanitize.sh builds
    it) and run as it is: no Python, no preload."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "nice_amd", "csrc")
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "map_san")
    r = subprocess.run([cxx, "-std=c++17", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", csrc, os.path.join(root, "tests", "map_san.cpp"),
                        os.path.join(csrc, "cpu_path.cpp"), "-o", exe, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
                                UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0 and "map_san ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
