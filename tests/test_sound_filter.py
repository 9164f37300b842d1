"""CPU tests of the sound niceonly filter (NICE_FILTER_SOUND): the MSD
recursion without Filter C on the host paths, the per-candidate prefix test's
host-evaluated hook against a Python restatement of its definition
(sound_restatement.py), its soundness, and the option check.
"""
import ctypes
import random

import pytest

import nice_amd as N
from nice_amd import _lib
from oracle import oracle as O

import sound_restatement as SR

FAST = [40, 42, 44, 45, 48, 49, 50, 52, 53, 54, 57, 58, 60, 62, 64, 65, 68, 80]
# window start a = s + K[b] (e - s) // 256: test_gpu_niceonly_bases.py's table,
# and for 40 / 50 / 52 / 53 / 54 / 80 windows whose sound field has prefix
# rejections and square survivors (found on the oracle); b64 has no candidate
# anywhere
K = {42: 27, 44: 2, 45: 2, 48: 1, 49: 10, 57: 31, 58: 7, 60: 8, 62: 24, 65: 21, 68: 23, 64: 128,
     40: 2, 50: 3, 52: 31, 53: 1, 54: 1, 80: 88}


@pytest.fixture(autouse=True)
def _restore_filter_c():
    """The oracle's Filter C switch is process-global: later tests rely on 1."""
    yield
    O.lib().oracle_set_filter_c(1)


def start(base):
    s, e = O.base_range(base)
    return s + K[base] * (e - s) // 256


def lib_ranges(a, e, base, floor, filt):
    n = ctypes.c_size_t()
    rc = _lib.lib().nice_msd_valid_ranges_ex(*N.api._split(a), *N.api._split(e), base, floor, filt, None, 0, n)
    assert rc in (_lib.NICE_OK, _lib.NICE_ERR_CAPACITY)
    buf = (ctypes.c_uint64 * (4 * max(n.value, 1)))()
    _lib.check(_lib.lib().nice_msd_valid_ranges_ex(*N.api._split(a), *N.api._split(e), base, floor, filt,
                                                   buf, n.value, n))
    return [(buf[4 * i] | (buf[4 * i + 1] << 64), buf[4 * i + 2] | (buf[4 * i + 3] << 64))
            for i in range(n.value)]


@pytest.mark.parametrize("base", [40, 50, 57, 80, 70])
def test_host_ranges_match_oracle(base):
    """nice_msd_valid_ranges_ex: filter 1 equals the oracle with Filter C off,
    filter 0 (and the old entry point) with it on, on seeded 1e6 windows at
    floors 250 and 64; at least one window differs between the two."""
    rng = random.Random(977 * base)
    s, e = O.base_range(base)
    differ = 0
    # two seeded windows (most of a range is pruned high up in both modes)
    # and the three chunks of a window that holds candidates
    a0 = start(base) if base in K else start_of(base)
    starts = [rng.randrange(s, e - 10 ** 6) for _ in range(2)] + [a0 + c * 10 ** 6 for c in range(3)]
    for floor in (250, 64):
        for a in starts:
            z = a + 10 ** 6
            sound, ref = lib_ranges(a, z, base, floor, 1), lib_ranges(a, z, base, floor, 0)
            assert sound == SR.oracle_ranges(a, z, base, floor, False)
            assert ref == SR.oracle_ranges(a, z, base, floor, True)
            assert [(r.range_start, r.range_end) for r in N.api.get_valid_ranges(N.FieldSize(a, z), base, floor)] == ref
            differ += sound != ref
    assert differ > 0


def test_b40_chunk_ranges_differ():
    a = 1_917_123_264_916
    assert len(lib_ranges(a, a + 10 ** 6, 40, 250, 0)) == 281
    sound = lib_ranges(a, a + 10 ** 6, 40, 250, 1)
    assert len(sound) == 760
    assert sound == SR.oracle_ranges(a, a + 10 ** 6, 40, 250, False)


def hook(base, s, e, n):
    return _lib.lib().nice_check_prefix_reject_inrange(base, *N.api._split(s), *N.api._split(e), *N.api._split(n))


@pytest.mark.parametrize("base", FAST)
def test_hook_matches_restatement_and_is_sound(base):
    """Every stride candidate of every sound leaf of the base's 3e6 window:
    the hook (the device code's leaf mask and rejection rule on the host)
    equals the restatement, and a rejected candidate is not nice."""
    a = start(base)
    leaves = SR.oracle_ranges(a, a + 3 * 10 ** 6, base, 250, False, 10 ** 6)
    n_cand = n_rej = 0
    for s, e in leaves:
        pre = SR.leaf_prefix(s, e, base)
        for n in SR.candidates(s, e, base):
            want = SR.rejected(pre, n, base)
            assert hook(base, s, e, n) == int(want), (s, e, n)
            if want:
                assert O.num_unique_digits(n, base) < base, (s, e, n)
            n_cand += 1
            n_rej += want
    if base != 64:
        assert n_cand > 0 and 0 < n_rej < n_cand


def test_hook_edge_leaves():
    """A leaf of one number rejects nothing; a leaf without a common prefix
    still rejects a candidate whose own low digits repeat; and a leaf whose
    prefix repeats rejects all."""
    base = 40
    s, e = O.base_range(base)
    rng = random.Random(5)
    for _ in range(2000):
        n = rng.randrange(s, e - 1)
        assert hook(base, n, n + 1, n) == 0
        # the whole range: the leading digits of first and last differ
        assert hook(base, s, e, n) == int(SR.rejected(SR.leaf_prefix(s, e, base), n, base))
        a = max(s, n - rng.randrange(1, 400))
        z = min(e, n + rng.randrange(1, 400))
        assert hook(base, a, z, n) == int(SR.rejected(SR.leaf_prefix(a, z, base), n, base))
    assert SR.leaf_prefix(s, e, base) == []


def test_hook_rejects_bad_arguments():
    s, e = O.base_range(40)
    assert hook(40, s, s + 10, s + 10) == _lib.NICE_ERR_INVALID  # n outside the leaf
    assert hook(40, s - 5, s + 10, s) == _lib.NICE_ERR_INVALID   # leaf outside the range
    assert hook(40, e - 5, e + 1, e - 1) == _lib.NICE_ERR_INVALID
    s70, _ = O.base_range(70)
    assert hook(70, s70, s70 + 10, s70) == _lib.NICE_ERR_INVALID  # no fast path


def cpu_niceonly(a, e, base, filt=None):
    out = (_lib.nice_number * 4096)()
    n = ctypes.c_size_t()
    if filt is None:
        rc = _lib.lib().nice_cpu_process_range_niceonly(*N.api._split(a), *N.api._split(e), base, 2, 2, out, 4096, n)
    else:
        rc = _lib.lib().nice_cpu_process_range_niceonly_ex(*N.api._split(a), *N.api._split(e), base, 2, 2, filt,
                                                           out, 4096, n)
    _lib.check(rc)
    return [out[i].number_lo | (out[i].number_hi << 64) for i in range(n.value)]


@pytest.mark.parametrize("base,size", [(40, 10 ** 6), (10, 53), (70, 10 ** 6)])
def test_cpu_api_sound(base, size):
    """nice_cpu_process_range_niceonly_ex: sound equals the oracle's
    process_range_niceonly with Filter C off, filter 0 and the old entry point
    the oracle with it on."""
    a = 47 if base == 10 else (1_917_123_264_916 if base == 40 else start_of(base))
    O.lib().oracle_set_filter_c(0)
    want_sound = [n for n, _ in O.process_range_niceonly(a, a + size, base)[0].nice_numbers]
    O.lib().oracle_set_filter_c(1)
    want_ref = [n for n, _ in O.process_range_niceonly(a, a + size, base)[0].nice_numbers]
    assert cpu_niceonly(a, a + size, base, 1) == want_sound
    assert cpu_niceonly(a, a + size, base, 0) == want_ref
    assert cpu_niceonly(a, a + size, base) == want_ref
    if base == 10:
        assert want_sound == [69]
    r = N.api.process_range_niceonly_cpu(N.FieldSize(a, a + size), base, filter="sound")
    assert [x.number for x in r.nice_numbers] == want_sound


def start_of(base):
    s, e = O.base_range(base)
    return s + 2 * (e - s) // 256


def test_filter_option_is_checked():
    """filter = 2 is NICE_ERR_INVALID on the CPU entry points (the GPU submit's
    check is in test_gpu_sound_filter.py) and a ValueError in Python."""
    out = (_lib.nice_number * 4)()
    n = ctypes.c_size_t()
    assert _lib.lib().nice_cpu_process_range_niceonly_ex(47, 0, 100, 0, 10, 2, 1, 2, out, 4, n) == _lib.NICE_ERR_INVALID
    assert _lib.lib().nice_msd_valid_ranges_ex(47, 0, 100, 0, 10, 250, 2, None, 0, n) == _lib.NICE_ERR_INVALID
    with pytest.raises(ValueError):
        N.GpuContext._nice_opts(filter="complete")
    assert N.GpuContext._nice_opts(filter="sound").filter == _lib.NICE_FILTER_SOUND
    assert N.GpuContext._nice_opts().filter == _lib.NICE_FILTER_REFERENCE
    assert ctypes.sizeof(_lib.nice_niceonly_opts) == 40
    assert N.api.NiceonlyStats(0, 0, 0, 0, 0.0, 0.0).prefix_rejected == 0
