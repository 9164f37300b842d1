"""The niceonly threshold hook (nice_debug_set_nice_min), without a GPU: the
oracle's nice_min variant against brute force, the hook's argument checks, the
host paths it must leave alone, and the window table the GPU tests
(test_gpu_nice_list.py) rely on -- every window must give the oracle square
survivors with several distinct union counts, or those tests would compare []
with [] as every in-range niceonly comparison did before.
"""
import ctypes

import pytest

import nice_amd as N
from nice_amd import _lib
from oracle import oracle as O

import nice_min_windows as W
import sound_restatement as SR
from test_sound_filter import K, cpu_niceonly


@pytest.fixture(autouse=True)
def _restore_filter_c():
    """The oracle's Filter C switch is process-global: later tests rely on 1."""
    yield
    O.lib().oracle_set_filter_c(1)


# --- the oracle variant ----------------------------------------------------------------------
def test_oracle_default_nice_min_equals_old_entry_points(golden):
    for case in golden["reference"]["niceonly"]:
        b = case["base"]
        s, e = O.base_range(b)
        if case["range"] != "base_range":
            e = s + case["size"]
        old, cands = O.process_field_niceonly_mt(s, e, b, 4)
        assert old.nice_numbers == [tuple(x) for x in case["nice_numbers"]], case["source"]
        ex = O.process_field_niceonly_ex(s, e, b, 4)
        sq = O.process_field_niceonly_sq(s, e, b, 4)
        sq0 = O.process_field_niceonly_sq(s, e, b, 4, nice_min=0)
        assert (ex[0], ex[1]) == (old, cands) and sq[:3] == ex and sq0 == sq, case["source"]
        # the C entry point itself at nice_min 0, with the count array
        buf, ubuf = (ctypes.c_uint64 * 64)(), (ctypes.c_uint32 * 32)()
        c, r, q = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        n = O.lib().oracle_process_field_niceonly_min(*O._split(s), *O._split(e), b, 4, 0, 0, 0, buf, ubuf, 32,
                                                      c, r, q)
        assert [(buf[2 * i] | (buf[2 * i + 1] << 64), ubuf[i]) for i in range(n)] == old.nice_numbers
        assert (c.value, r.value, q.value) == sq[1:]


@pytest.mark.parametrize("base,offset", [(40, 0), (57, 2 * 10 ** 6), (80, 0)])
def test_oracle_nice_min_is_the_brute_force_list(base, offset):
    """5e5 numbers of the base's fused window (the part of it that holds
    survivors) on 1e5 chunks: the valid ranges from the oracle, the stride
    candidates and their digits in Python integers."""
    a = W.start(base, "fused") + offset
    size, chunk = 500_000, 100_000
    surv, n_cand = [], 0
    leaves = SR.oracle_ranges(a, a + size, base, 250, True, chunk)
    for s, e in leaves:
        for n in SR.candidates(s, e, base):
            n_cand += 1
            if SR.square_repeat_free(n, base):
                surv.append((n, SR.union_count(n, base)))
    assert len(surv) >= 4, "an empty list proves nothing"
    old = O.process_field_niceonly_sq(a, a + size, base, 4, chunk)
    assert old[1:] == (n_cand, len(leaves), len(surv))
    assert old[0].nice_numbers == [(n, base) for n, u in surv if u == base]
    counts = sorted({u for _, u in surv})
    for t in [1, counts[0], counts[len(counts) // 2], counts[-1], counts[-1] + 1, base]:
        got = O.process_field_niceonly_sq(a, a + size, base, 4, chunk, nice_min=t)
        assert got[0].nice_numbers == [(n, u) for n, u in surv if u >= t], t
        assert got[1:] == old[1:]
        # a list longer than the caller's room is re-read, not cut
        assert O.process_field_niceonly_sq(a, a + size, base, 4, chunk, cap=1, nice_min=t) == got


# --- the hook's arguments ----------------------------------------------------------------------
def test_set_nice_min_checks_its_arguments():
    L = _lib.lib()
    try:
        for b in range(0, 131):
            if L.nice_niceonly_fast_base(b) == 1:
                assert b in W.FAST
                assert L.nice_debug_set_nice_min(b, b + 1) == _lib.NICE_ERR_INVALID
                assert b"nice_min must be" in L.nice_last_error()
                assert L.nice_debug_set_nice_min(b, 0xffffffff) == _lib.NICE_ERR_INVALID
                assert L.nice_debug_set_nice_min(b, 1) == _lib.NICE_OK
                assert L.nice_debug_set_nice_min(b, b) == _lib.NICE_OK
                assert L.nice_debug_set_nice_min(b, 0) == _lib.NICE_OK
            else:
                assert b not in W.FAST
                for v in (0, 1, b):
                    assert L.nice_debug_set_nice_min(b, v) == _lib.NICE_ERR_INVALID
        assert L.nice_debug_set_nice_min(70, 60) == _lib.NICE_ERR_INVALID  # an FD-less, residue-carrying base
        assert b"niceonly fast path" in L.nice_last_error()
    finally:
        for b in W.FAST:
            L.nice_debug_set_nice_min(b, 0)


def test_hook_leaves_the_host_paths_alone():
    """nice_cpu_process_range_niceonly and nice_check_is_nice_inrange keep
    production semantics while the hook lists every square survivor on the
    GPU paths: the window's survivors stay unlisted and not nice."""
    L = _lib.lib()
    for base in (40, 57, 80):
        a, size, chunk = W.window(base, "fused")
        surv = W.reference_field(a, size, base, chunk)[3]
        assert len(surv) >= W.MIN_SURVIVORS and all(u < base for _, u in surv)
        want = [n for n, _ in O.process_range_niceonly(a, a + 10 ** 6, base)[0].nice_numbers]
        before = cpu_niceonly(a, a + 10 ** 6, base)
        with W.lowered(base, 1):
            assert cpu_niceonly(a, a + 10 ** 6, base) == before == want == []
            assert cpu_niceonly(a, a + 10 ** 6, base, 1) == cpu_niceonly(a, a + 10 ** 6, base, 0) == []
            r = N.api.process_range_niceonly_cpu(N.FieldSize(a, a + 10 ** 6), base)
            assert [x.number for x in r.nice_numbers] == []
            for n, u in surv[:50]:
                assert L.nice_check_is_nice_inrange(base, *O._split(n)) == 0
                assert L.nice_check_unique_inrange(base, *O._split(n)) == u


# --- the window table ----------------------------------------------------------------------------
def enough(surv, what):
    counts = {u for _, u in surv}
    assert len(surv) >= W.MIN_SURVIVORS, (what, len(surv))
    assert len(counts) >= W.MIN_COUNTS, (what, sorted(counts))
    assert [n for n, _ in surv] == sorted({n for n, _ in surv}), what


@pytest.mark.parametrize("base", W.BASES)
def test_window_table_gives_the_oracle_survivors(base):
    """What keeps the GPU tests from comparing empty lists: >= 8 square
    survivors with >= 3 distinct union counts in the base's fused and wave
    window under the reference filter, in its fused window under the sound
    filter and, for the three walks, in its wave window under the sound
    filter -- by the oracle and the restatement alone.  The windows lie in the
    base's valid range; for b >= 57 every survivor is wider than 64 bits."""
    r0, r1 = O.base_range(base)
    for kind in ("fused", "wave"):
        a, size, chunk = W.window(base, kind)
        assert r0 <= a and a + size <= r1
        ranges, cands, sq, surv = W.reference_field(a, size, base, chunk)
        enough(surv, (base, kind, "reference"))
        assert sq == len(surv) <= cands and ranges > 0
        if base >= 57:
            assert all(n >> 64 for n, _ in surv)
        # the thresholds the GPU tests run: the oracle at each equals the filtered survivors
        ts = W.thresholds(surv)
        for t in (ts[0], ts[len(ts) // 2], ts[-1]):
            got = O.process_field_niceonly_sq(a, a + size, base, W.THREADS, chunk, nice_min=t)
            assert [n for n, _ in got[0].nice_numbers] == W.listed(surv, t)
            assert got[1:] == (cands, ranges, sq)
        assert W.listed(surv, ts[0]) == [n for n, _ in surv] and W.listed(surv, ts[-1]) == []
        # production: the same statistics, nothing listed
        prod = O.process_field_niceonly_sq(a, a + size, base, W.THREADS, chunk)
        assert prod[0].nice_numbers == [] and prod[1:] == (cands, ranges, sq)
        if kind == "fused" or base in W.WAVE_WALKS:
            ssurv = W.sound_survivors(a, size, base, chunk)
            enough(ssurv, (base, kind, "sound"))
            st = SR.sound_field(a, size, base, chunk)
            assert st[3] == len(ssurv) and st[4] == [] and 0 < st[2] < st[1]
            if base >= 57:
                assert all(n >> 64 for n, _ in ssurv)


def test_b64_windows_hold_no_candidate():
    """Why b64 is not in the table (nice_debug_cube_count reaches it): the MSD
    filter leaves its windows no candidate to list."""
    assert 64 in W.FAST and 64 not in W.BASES
    s, e = O.base_range(64)
    a = s + K[64] * (e - s) // 256
    for size, chunk in (W.FUSED, W.WAVE):
        assert O.process_field_niceonly_sq(a, a + size, 64, W.THREADS, chunk, nice_min=1)[1:] == (0, 0, 0)


# --- the overflow fields ------------------------------------------------------------------------------
def test_overflow_fields_list_more_than_the_device_list_holds():
    """The growth tests' fields, by the oracle alone: at nice_min 1 the b40
    field [range start, +2e9) lists 170 413 numbers on 1e8 chunks and more than
    2^16 (the device list's first size) on 1e6 chunks too; the whole 1e9 field
    on the client's chunking lists 59 117 of its 1 389 117 candidates."""
    a, size = W.GROW_FIELD
    for chunk, exact in ((10 ** 8, 170_413), (10 ** 6, None)):
        ranges, cands, sq, surv = W.reference_field(a, size, 40, chunk)
        assert len(surv) > 2 ** 16
        assert exact is None or len(surv) == exact
    res, cands, ranges, sq = O.process_field_niceonly_sq(a, a + 10 ** 9, 40, W.THREADS, nice_min=1)
    assert (len(res.nice_numbers), cands) == (59_117, 1_389_117)
