"""The MSD recursion's range list, the parts that need no GPU: the CPU twin
(nice_cpu_msd_ranges) against the oracle root by root, out_root and counts, the
capacity retry, the argument errors, the plan hook (nice_debug_msd_ranges_plan),
the Python layer (chunk_roots, RangeBounds) and the host code under the
sanitizers (tests/msd_ranges_san.cpp).
"""
import ctypes
import os
import shutil
import subprocess

import pytest

from nice_amd import _lib, api, client, survey
from oracle import oracle as O

import sound_restatement as S

MASK = (1 << 64) - 1
FUSED_MAX = 1 << 14  # layout.h kFusedMaxCap
BATCH_NODES = 1 << 27  # msd_ranges_plan.hpp kMsdRangesBatchNodes
A40 = 4_234_942_132_458
A50 = 94_760_515_586_064_977


@pytest.fixture(autouse=True)
def _restore():
    """The oracle's Filter C switch is process-global."""
    yield
    O.lib().oracle_set_filter_c(1)


def pack(roots):
    flat = [x for s, e in roots for x in (s & MASK, s >> 64, e & MASK, e >> 64)]
    return (ctypes.c_uint64 * max(len(flat), 4))(*flat)


def cpu_call(base, roots, floor, filt, cap, threads=2, n_roots=None, with_idx=True):
    """(rc, n_out, bounds, out_root, counts) of one nice_cpu_msd_ranges call."""
    n_roots = len(roots) if n_roots is None else n_roots
    out = (ctypes.c_uint64 * (4 * max(cap, 1)))()
    idx = (ctypes.c_uint32 * max(cap, 1))()
    counts = (ctypes.c_uint64 * max(n_roots, 1))()
    n = ctypes.c_size_t(12345)
    rc = _lib.lib().nice_cpu_msd_ranges(base, pack(roots), n_roots, floor, filt, threads, out if cap else None,
                                        idx if with_idx else None, counts if with_idx else None, cap, n)
    m = min(n.value, cap)
    return (rc, n.value, [(out[4 * i] | out[4 * i + 1] << 64, out[4 * i + 2] | out[4 * i + 3] << 64) for i in range(m)],
            list(idx[:m]), list(counts[:n_roots]))


def roots_of(base):
    """Roots around the split rule's edges, across the base range's end,
    repeated and overlapping."""
    s, e = O.base_range(base)
    a = {40: A40, 50: A50}.get(base, s + (e - s) // 3)
    sizes = [1, 2, 249, 250, 251, 499, 500, 501, 1003, 30_000]
    roots = [(a + 7 * i, a + 7 * i + z) for i, z in enumerate(sizes)]
    return roots + [(e - 2_000, e + 2_000), (a, a + 30_000), (a + 15_000, a + 45_000), (s - 100, s + 900)]


# --- the CPU twin against the oracle ----------------------------------------------------
@pytest.mark.parametrize("base", [10, 33, 40, 50, 57, 65, 80, 97])
@pytest.mark.parametrize("filt", ["reference", "sound"])
def test_cpu_twin_equals_the_oracle_root_by_root(base, filt):
    """Reference filter: oracle.valid_ranges.  Sound filter: the same recursion
    with the oracle's Filter C off (sound_restatement.oracle_ranges)."""
    roots = [(47, 100), (1, 60), (47, 100)] if base == 10 else roots_of(base)
    floor = 4 if base == 10 else 250
    want = [[tuple(r) for r in S.oracle_ranges(s, e, base, floor, filt == "reference")] for s, e in roots]
    assert any(want)
    bounds, counts = api.msd_ranges_cpu(roots, base, floor, filt, threads=3)
    assert counts == [len(w) for w in want]
    assert bounds.tolist() == [r for w in want for r in w]
    assert bounds.root_list() == [i for i, w in enumerate(want) for _ in w]
    assert bounds.numbers() == sum(e - s for w in want for s, e in w)
    # ... and nice_msd_valid_ranges_ex, which it loops
    for (s, e), w in zip(roots[:4], want):
        assert [(r.range_start, r.range_end) for r in api.get_valid_ranges(api.FieldSize(s, e), base, floor, filt)] == w


def test_b10_counts():
    bounds, counts = api.msd_ranges_cpu([(47, 100)], 10, 4)
    assert counts == [2] and bounds.numbers() == 13


@pytest.mark.parametrize("floor", [1, 7, 250])
def test_split_rule_edges(floor):
    sizes = [1, 2, floor - 1, floor, floor + 1, 2 * floor - 1, 2 * floor, 2 * floor + 1, 4 * floor + 3]
    for base, a in ((40, A40), (50, A50)):
        roots = [(a, a + z) for z in sizes if z > 0]
        want = [[tuple(r) for r in O.valid_ranges(s, e, base, floor)] for s, e in roots]
        bounds, counts = api.msd_ranges_cpu(roots, base, floor)
        assert bounds.tolist() == [r for w in want for r in w] and counts == [len(w) for w in want]


def test_capacity_and_null_outputs():
    roots = roots_of(40)
    rc, n, full, idx, counts = cpu_call(40, roots, 250, 0, 4096)
    assert rc == _lib.NICE_OK and n == len(full) > len(roots)
    rc, n2, part, _, counts2 = cpu_call(40, roots, 250, 0, n - 1)
    assert rc == _lib.NICE_ERR_CAPACITY and n2 == n and counts2 == counts
    rc, n3, _, _, _ = cpu_call(40, roots, 250, 0, 0)
    assert rc == _lib.NICE_ERR_CAPACITY and n3 == n
    rc, n4, again, _, _ = cpu_call(40, roots, 250, 0, n, with_idx=False)
    assert rc == _lib.NICE_OK and again == full
    assert sum(counts) == n and idx == sorted(idx)


def test_argument_errors():
    ok = [(47, 100)]

    def rc(base=10, roots=ok, floor=4, filt=0, n_roots=None):
        r = cpu_call(base, roots, floor, filt, 64, n_roots=n_roots)[0]
        return r, (_lib.lib().nice_last_error() or b"").decode()

    assert rc()[0] == _lib.NICE_OK
    assert rc(n_roots=0)[0] == _lib.NICE_ERR_INVALID
    assert rc(n_roots=(1 << 20) + 1)[0] == _lib.NICE_ERR_INVALID
    for bad in ((100, 100), (100, 47)):
        code, msg = rc(roots=[(47, 100), (1, 5), bad])
        assert code == _lib.NICE_ERR_INVALID and "root 2" in msg
    code, msg = rc(roots=[(47, 100), (47, 48 + (1 << 40))])
    assert code == _lib.NICE_ERR_INVALID and "root 1" in msg and "2^40" in msg
    assert rc(floor=0)[0] == _lib.NICE_ERR_INVALID
    assert rc(filt=2)[0] == _lib.NICE_ERR_INVALID
    assert rc(base=1)[0] == _lib.NICE_ERR_INVALID and rc(base=129)[0] == _lib.NICE_ERR_INVALID
    n = ctypes.c_size_t()
    L = _lib.lib()
    assert L.nice_cpu_msd_ranges(10, None, 1, 4, 0, 1, None, None, None, 0, n) == _lib.NICE_ERR_INVALID
    assert L.nice_cpu_msd_ranges(10, pack(ok), 1, 4, 0, 1, None, None, None, 8, n) == _lib.NICE_ERR_INVALID
    # the plan hook refuses the same
    buf = (ctypes.c_uint64 * 64)()
    assert L.nice_debug_msd_ranges_plan(10, pack(ok), 1, 4, 1, buf, 16, n) == _lib.NICE_OK and n.value == 1
    assert L.nice_debug_msd_ranges_plan(10, pack(ok), 1, 0, 1, buf, 16, n) == _lib.NICE_ERR_INVALID
    assert L.nice_debug_msd_ranges_plan(10, pack(ok), 0, 4, 1, buf, 16, n) == _lib.NICE_ERR_INVALID
    assert L.nice_debug_msd_ranges_plan(10, pack([(5, 5)]), 1, 4, 1, buf, 16, n) == _lib.NICE_ERR_INVALID
    assert L.nice_debug_msd_ranges_plan(10, pack(ok), 1, 4, 0, buf, 16, n) == _lib.NICE_ERR_INVALID
    assert L.nice_debug_msd_ranges_plan(10, pack(ok), 1, 4, 65, buf, 16, n) == _lib.NICE_ERR_INVALID
    assert L.nice_debug_msd_ranges_plan(130, pack(ok), 1, 4, 1, buf, 16, n) == _lib.NICE_ERR_INVALID


def test_a_root_of_two_to_the_forty_numbers_is_taken():
    """The limit is 2^40 inclusive: with a floor as large the root is one leaf."""
    bounds, counts = api.msd_ranges_cpu([(A40, A40 + (1 << 40))], 40, 1 << 40)
    assert bounds.tolist() == [(A40, A40 + (1 << 40))] and counts == [1]


# --- the plan hook -----------------------------------------------------------------------
def test_plan_group_on_both_sides_of_the_fused_cap():
    for floor in (1, 250, 1000):
        edge = floor * (FUSED_MAX - 2)  # the largest size with size / floor + 2 <= kFusedMaxCap ...
        sizes = [1, floor, edge, edge + floor - 1, edge + floor, edge + floor + 1, 10 * edge]
        plan = api.msd_ranges_plan([(A40, A40 + z) for z in sizes], 40, floor)
        assert [p[0] for p in plan] == list(range(len(sizes)))
        assert [p[1] for p in plan] == [1 if z // floor + 2 <= FUSED_MAX else 0 for z in sizes]
        assert [p[1] for p in plan] == [1, 1, 1, 1, 0, 0, 0]
    # a root of 2^32 numbers or more never fits a workgroup's 32-bit nodes
    plan = api.msd_ranges_plan([(A40, A40 + (1 << 32) - 1), (A40, A40 + (1 << 32))], 40, 1 << 20)
    assert [p[1] for p in plan] == [1, 0]


@pytest.mark.parametrize("nd", [1, 2, 3, 8])
def test_plan_devices_are_contiguous_runs_balanced_by_numbers(nd):
    sizes = [10 ** 6] * 40 + [1, 5, 10 ** 7, 3 * 10 ** 6] + [10 ** 5] * 100
    plan = api.msd_ranges_plan([(A50 + i, A50 + i + z) for i, z in enumerate(sizes)], 50, 250, nd)
    dev = [p[2] for p in plan]
    assert dev == sorted(dev) and dev[0] == 0 and set(dev) <= set(range(nd))
    total = sum(sizes)
    before = 0
    for z, d in zip(sizes, dev):  # a root runs where the numbers before it fall
        assert d == before * nd // total
        before += z
    if nd > 1:
        per = [sum(z for z, d in zip(sizes, dev) if d == q) for q in range(nd)]
        # each cut lies at most one root past its ideal place, k * total / nd
        assert all(abs(x - total / nd) <= max(sizes) for x in per)


def test_plan_batches_cover_every_root_once():
    """Bounds of min(size / floor + 1, 2^22) nodes per root, 2^27 per batch:
    at floor 1 thirty-two roots of 2^23 numbers fill a batch."""
    roots = [(A40 + i, A40 + i + (1 << 23)) for i in range(80)] + [(A40, A40 + 10)]
    for nd in (1, 2):
        plan = api.msd_ranges_plan(roots, 40, 1, nd)
        assert [p[0] for p in plan] == list(range(len(roots)))
        for d in range(nd):
            mine = [(p[3], min((roots[p[0]][1] - roots[p[0]][0]) // 1 + 1, 1 << 22)) for p in plan if p[2] == d]
            batches = [b for b, _ in mine]
            assert batches == sorted(batches) and batches[0] == 0 and set(batches) == set(range(batches[-1] + 1))
            for b in set(batches):
                assert sum(z for q, z in mine if q == b) <= BATCH_NODES
        if nd == 1:
            assert [p[3] for p in plan] == [0] * 32 + [1] * 32 + [2] * 17
    # at floor 250 the same roots fit one batch
    assert {p[3] for p in api.msd_ranges_plan(roots, 40, 250)} == {0}


# --- the Python layer --------------------------------------------------------------------
def test_chunk_roots_is_the_field_chunk_grid():
    r = api.chunk_roots(A40, A40 + 3 * 10 ** 6 + 1, 999_983)
    assert r.tolist() == [(A40 + i * 999_983, min(A40 + (i + 1) * 999_983, A40 + 3 * 10 ** 6 + 1)) for i in range(4)]
    assert api.chunk_roots(47, 100, 53).tolist() == [(47, 100)]
    assert api.chunk_roots(47, 100, 52).tolist() == [(47, 99), (99, 100)]
    # 0: the reference client's rule, 1e6 * clamp(ceil(size / 1e11), 1, 1000)
    assert api.chunk_roots(A40, A40 + 10 ** 7).tolist() == [(A40 + i * 10 ** 6, A40 + (i + 1) * 10 ** 6) for i in range(10)]
    assert api.chunk_roots(A40, A40 + 3 * 10 ** 11)[0] == (A40, A40 + 3 * 10 ** 6)
    big = 1 << 70
    assert api.chunk_roots(big, big + 25, 10).tolist() == [(big, big + 10), (big + 10, big + 20), (big + 20, big + 25)]
    assert api.chunk_roots((1 << 64) - 5, (1 << 64) + 5, 4).tolist()[1] == ((1 << 64) - 1, (1 << 64) + 3)
    with pytest.raises(ValueError):
        api.chunk_roots(100, 100)


def test_range_bounds_pass_through_unchanged():
    """msd_ranges' bounds are what niceonly_ranges and detailed_ranges take:
    the CPU twins of both accept the object as it is."""
    roots = api.chunk_roots(A40, A40 + 2 * 10 ** 5, 10 ** 5)
    bounds, counts = api.msd_ranges_cpu(roots, 40)
    assert len(bounds) == sum(counts) > 2 and bounds[0] == bounds.tolist()[0] and bounds[-1] == bounds.tolist()[-1]
    buf, n = api._pack_ranges(bounds)
    assert buf is bounds.buf and n == len(bounds)
    assert api.niceonly_ranges_cpu(bounds, 40) == api.niceonly_ranges_cpu(bounds.tolist(), 40)
    part = bounds.part(1, 3)
    assert part.tolist() == bounds.tolist()[1:3] and part.root_list() == bounds.root_list()[1:3]
    assert api.detailed_ranges_cpu(part, 40) == api.detailed_ranges_cpu(part.tolist(), 40)


def test_survey_and_cli_know_the_device_placement():
    with pytest.raises(ValueError):
        survey.survey_niceonly_base(None, 10, 4, 10, msd_where="device")  # needs a context
    with pytest.raises(ValueError):
        survey.survey_niceonly_base(None, 10, 4, 10, msd_where="gpu")
    a = client.parse_args(["--survey-niceonly", "--base", "50", "--survey-msd", "device"])
    assert a.survey_msd == "device"
    assert client.parse_args(["--survey-niceonly", "--base", "50"]).survey_msd == "host"
    assert client.main(["--survey-niceonly", "--base", "10", "--survey-msd", "device", "--log-level", "off"]) == 2


# --- the host code under the sanitizers ---------------------------------------------------
def test_host_code_runs_clean_under_asan_and_ubsan(tmp_path):
    """tests/msd_ranges_san.cpp: the plan header and the CPU twin (cpu_path.cpp)
    in a program of their own, built with ASan + UBSan and run as it is: no
    Python, no preload."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "nice_amd", "csrc")
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "msd_ranges_san")
    r = subprocess.run([cxx, "-std=c++17", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", csrc, os.path.join(root, "tests", "msd_ranges_san.cpp"),
                        os.path.join(csrc, "cpu_path.cpp"), "-o", exe, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
                                UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0 and "msd_ranges_san ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
