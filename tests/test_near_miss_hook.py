"""The lowered-cutoff test hook, without a GPU: the oracle's cutoff variants
against brute force, nice_debug_fd_window / nice_debug_set_near_miss_cutoff's
argument checks, and the window table the GPU tests
(test_gpu_near_miss_list.py) rely on -- every window must give the oracle a
list to compare, or those tests would compare [] with [] again.
"""
import ctypes

import pytest

from nice_amd import _lib
from oracle import oracle as O

import near_miss_windows as W


def test_oracle_cutoff_variant_at_default_equals_old_entry_points(golden):
    for case in golden["reference"]["detailed"]:
        b = case["base"]
        s, e = O.base_range(b)
        if case["range"] != "base_range":
            e = s + case["size"]
        c = O.near_miss_cutoff(b)
        old = O.process_range_detailed(s, e, b)
        assert O.process_range_detailed(s, e, b, cutoff=c) == old, case["source"]
        assert O.process_field_detailed_mt(s, e, b, 4) == old, case["source"]
        assert O.process_field_detailed_mt(s, e, b, 4, cutoff=c) == old, case["source"]
        assert O.process_field_detailed_mt(s, e, b, 4, cutoff=c, chunk=997) == old, case["source"]
        assert old.distribution == [tuple(x) for x in case["distribution"]]
        assert old.nice_numbers == [tuple(x) for x in case["nice_numbers"]]


@pytest.mark.parametrize("base", [40, 57, 80])
def test_oracle_lowered_cutoff_is_the_brute_force_list(base):
    a, _ = W.window(base)
    e = a + 20_000
    old = O.process_range_detailed(a, e, base)
    uniq = [(n, O.num_unique_digits(n, base)) for n in range(a, e)]
    low, prod = W.low_cutoff(base), O.near_miss_cutoff(base)
    assert low < (low + prod) // 2 < prod
    # W0 + W - 2 (inside the histogram window: the GPU hook refuses it, the
    # oracle has no such limit) makes the 2e4 window's list longer
    for cutoff in (low - 1, low, (low + prod) // 2):
        want = [(n, u) for n, u in uniq if u > cutoff]
        r = O.process_range_detailed(a, e, base, cutoff=cutoff)
        assert r.distribution == old.distribution
        assert r.nice_numbers == want
        m = O.process_field_detailed_mt(a, e, base, 4, cutoff=cutoff, chunk=1500)
        assert m.distribution == old.distribution and m.nice_numbers == want
        assert W.oracle(a, e, base, cutoff) == ([0] + [c for _, c in old.distribution], want)
    assert len([1 for _, u in uniq if u > low - 1]) > 0, "an empty list proves nothing"


def test_fd_window_of_every_fd_base():
    L = _lib.lib()
    bases = W.fd_bases()
    assert sorted(W.WINDOW_FRAC) == bases
    for b in range(2, 129):
        if b in bases:
            w0, w = W.fd_window(b)
            assert w0 >= 1 and w >= 1
            assert w0 + w <= L.nice_near_miss_cutoff(b) + 1
            assert w0 + w <= b
        else:
            x, y = ctypes.c_uint32(), ctypes.c_uint32()
            assert L.nice_debug_fd_window(b, x, y) == _lib.NICE_ERR_INVALID


def test_set_near_miss_cutoff_checks_its_arguments():
    L = _lib.lib()
    assert L.nice_fd_kernel_base(70) == 0
    assert L.nice_debug_set_near_miss_cutoff(70, 65) == _lib.NICE_ERR_INVALID
    assert L.nice_debug_set_near_miss_cutoff(70, 0) == _lib.NICE_ERR_INVALID
    assert L.nice_debug_set_near_miss_cutoff(200, 0) == _lib.NICE_ERR_INVALID
    try:
        for b in W.fd_bases():
            w0, w = W.fd_window(b)
            assert L.nice_debug_set_near_miss_cutoff(b, w0 + w - 2) == _lib.NICE_ERR_INVALID
            assert L.nice_debug_set_near_miss_cutoff(b, b) == _lib.NICE_ERR_INVALID
            assert b"cutoff must be" in L.nice_last_error()
            assert L.nice_debug_set_near_miss_cutoff(b, w0 + w - 1) == _lib.NICE_OK
            assert L.nice_debug_set_near_miss_cutoff(b, b - 1) == _lib.NICE_OK
            assert L.nice_debug_set_near_miss_cutoff(b, 0) == _lib.NICE_OK
    finally:
        for b in W.fd_bases():
            L.nice_debug_set_near_miss_cutoff(b, 0)


def test_hook_leaves_the_cpu_api_and_the_public_validator_alone():
    """nice_cpu_process_range_detailed and nice_validate_detailed keep the
    production cutoff while the hook is set."""
    from nice_amd import api
    L = _lib.lib()
    a, e = W.window(40)
    want = O.process_range_detailed(a, e, 40)
    hist, low_list = W.oracle(a, e, 40, W.low_cutoff(40))
    assert len(low_list) > len(want.nice_numbers)

    def validate(lst):
        h = (ctypes.c_uint64 * 41)(*hist)
        arr = (_lib.nice_number * max(len(lst), 1))()
        for i, (n, u) in enumerate(lst):
            arr[i].number_lo, arr[i].number_hi, arr[i].num_uniques = n & O.MASK64, n >> 64, u
        return L.nice_validate_detailed(40, e - a, 0, h, arr, len(lst))

    with W.lowered(40):
        got = api.process_range_detailed_cpu(api.FieldSize(a, e), 40, threads=W.THREADS)
        assert [(x.number, x.num_uniques) for x in got.nice_numbers] == want.nice_numbers
        assert [(d.num_uniques, d.count) for d in got.distribution] == want.distribution
        assert validate(want.nice_numbers) == _lib.NICE_OK
        assert validate(low_list) == _lib.NICE_ERR_INVALID


@pytest.mark.parametrize("base", sorted(W.WINDOW_FRAC))
def test_window_table_gives_the_oracle_a_list(base):
    """What keeps the GPU tests from comparing empty lists: >= 8 listed numbers
    per 1e6 window at cutoff W0 + W - 1, by the oracle alone, and the windows
    lie inside one limb layout of the base's range."""
    a, e = W.window(base)
    s, r1 = O.base_range(base)
    assert s <= a and e + 11 <= r1
    assert not any(a < c < e + 11 for c in W.cuts_of(base))
    low = W.low_cutoff(base)
    hist, lst = W.oracle(a, e, base, low)
    assert len(lst) >= W.MIN_ENTRIES, (base, len(lst))
    assert len(lst) == sum(hist[low + 1:])
    assert all(u > low for _, u in lst) and [n for n, _ in lst] == sorted(n for n, _ in lst)
    assert W.oracle(a, e, base)[0] == hist
