"""CPU tests of the niceonly fast-base list (csrc/niceonly_bases.h) and of the
host-evaluated in-range limb paths (radix_fast.hpp) of the twelve bases that
joined 40/50/52/53/54/80 on it."""
import ctypes
import random

import pytest

import nice_amd as N
from nice_amd import _lib
from oracle import oracle as O

FAST = [40, 42, 44, 45, 48, 49, 50, 52, 53, 54, 57, 58, 60, 62, 64, 65, 68, 80]
NEW = [42, 44, 45, 48, 49, 57, 58, 60, 62, 64, 65, 68]


def _split(x):
    return x & ((1 << 64) - 1), x >> 64


def _residue_count(base):
    n = ctypes.c_size_t()
    m = ctypes.c_uint64()
    rc = _lib.lib().nice_stride_table(base, 2, ctypes.byref(m), None, 0, ctypes.byref(n))
    assert rc in (_lib.NICE_OK, _lib.NICE_ERR_CAPACITY), (base, rc)
    return n.value


def test_fast_list_is_fd_bases_with_residues():
    """The list's definition: a base is on it exactly if it has an FD kernel
    and its k = 2 stride table has at least one residue."""
    L = _lib.lib()
    got = []
    for b in range(2, 129):
        want = bool(L.nice_fd_kernel_base(b)) and _residue_count(b) >= 1
        assert bool(L.nice_niceonly_fast_base(b)) == want, b
        assert N.niceonly_fast_base(b) == want
        if want:
            got.append(b)
    assert got == FAST and set(NEW) < set(FAST)
    assert not N.niceonly_fast_base(70) and not N.niceonly_fast_base(129)


@pytest.mark.parametrize("base", NEW)
def test_new_base_is_nice_matches_oracle(base):
    """is_nice_fast on the range ends, 3000 seeded random in-range n and 500
    near-nice n (the ones that reach the cube scan)."""
    L = _lib.lib()
    rng = random.Random(base)
    s, e = O.base_range(base)
    ns = [s, e - 1] + [rng.randrange(s, e) for _ in range(3000)]
    deep = [n for n in (rng.randrange(s, e) for _ in range(40000)) if O.scan_depth(n, base) > base // 3]
    assert len(deep) >= 500
    for n in ns + deep[:500]:
        assert L.nice_check_is_nice_inrange(base, *_split(n)) == int(O.is_nice(n, base)), n
    assert L.nice_check_is_nice_inrange(base, *_split(s - 1)) == _lib.NICE_ERR_INVALID
    assert L.nice_check_is_nice_inrange(base, *_split(e)) == _lib.NICE_ERR_INVALID


@pytest.mark.parametrize("base", NEW)
def test_new_base_unique_matches_oracle(base):
    """unique_fast's digit bits at both range ends and on 2000 random n."""
    L = _lib.lib()
    rng = random.Random(7 * base)
    s, e = O.base_range(base)
    for n in [s, s + 1, e - 2, e - 1] + [rng.randrange(s, e) for _ in range(2000)]:
        assert L.nice_check_unique_inrange(base, *_split(n)) == O.num_unique_digits(n, base), n
    assert L.nice_check_unique_inrange(base, *_split(e)) == _lib.NICE_ERR_INVALID
    assert L.nice_check_unique_inrange(base, *_split(s - 1)) == _lib.NICE_ERR_INVALID


@pytest.mark.parametrize("base", NEW)
def test_new_base_msd_skippable_matches_oracle(base):
    """msd_skippable_fast on seeded ranges of every scale and inside one b^2
    block (Filter C), some skippable and some not."""
    L = _lib.lib()
    rng = random.Random(1000 + base)
    s, e = O.base_range(base)
    B = base * base
    cases = []
    for _ in range(1500):
        size = 10 ** rng.uniform(0, 9)
        a = rng.randrange(s, e - int(size) - 1)
        cases.append((a, a + max(1, int(size))))
    for _ in range(1500):
        blk = rng.randrange(s // B + 1, e // B - 1) * B
        a = blk + rng.randrange(B - 2)
        cases.append((a, rng.randrange(a + 1, blk + B + 1)))
    hits = 0
    for a, b in cases:
        want = int(O.has_duplicate_msd_prefix(a, b, base))
        hits += want
        assert L.nice_check_msd_skippable_inrange(base, *_split(a), *_split(b)) == want, (a, b)
    assert 0 < hits < len(cases)
    assert L.nice_check_msd_skippable_inrange(base, *_split(s - 1), *_split(s + 10)) == _lib.NICE_ERR_INVALID
    assert L.nice_check_msd_skippable_inrange(base, *_split(e - 10), *_split(e + 1)) == _lib.NICE_ERR_INVALID


def test_hooks_reject_bases_off_the_list():
    L = _lib.lib()
    for base in (43, 55, 67, 70):
        s, e = O.base_range(base)
        n = (s + e) // 2
        assert L.nice_check_is_nice_inrange(base, *_split(n)) == _lib.NICE_ERR_INVALID
        assert L.nice_check_unique_inrange(base, *_split(n)) == _lib.NICE_ERR_INVALID
        assert L.nice_check_msd_skippable_inrange(base, *_split(n), *_split(n + 100)) == _lib.NICE_ERR_INVALID
