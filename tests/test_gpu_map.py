"""The per-number unique-count map on the GPU (nice_unique_map: fd2_map_kernel
and generic_map_kernel): byte for byte against the oracle, against the
existing detailed kernels on ranges too long for the per-n oracle loop, in
place into a torch tensor at every alignment with guard bytes around it, over
two devices, and through survey.class_distribution.

Run on the MI355X box:  python -m pytest tests/test_gpu_map.py -m gpu -q
"""
import ctypes
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nice_amd as N
from nice_amd import _lib, api, survey
from oracle import oracle as O

import fd_carry_points as F
import near_miss_windows as W
from test_map import plan as map_plan

pytestmark = pytest.mark.gpu
MASK = (1 << 64) - 1
# Up to b58 (512 lanes, target chunk 81 or 161): full workgroups, a partial last one and a tail
# workgroup.  From b59 on (1024 or 512 lanes, target chunk 241) one partial workgroup of 1010 / 507
# lanes walking 99 / 197 numbers each -- several ring flushes per lane -- and a tail; full_size()
# is the window with a full workgroup at every base.
LONG = 100_003
FD_BASES = W.fd_bases()


def full_size(base):
    """Workgroup x target chunk + 1 numbers: two main workgroups, the first
    with all its lanes, and a tail."""
    rs, _ = O.base_range(base)
    wg = max(r[3] for r in map_plan(base, rs, rs + 10 ** 6))
    size = wg * ((80 if base <= 45 else 160 if base <= 58 else 240) + 1) + 1
    recs = map_plan(base, rs, rs + size)
    assert wg in (512, 1024) and [r[3] == wg for r in recs] == [True, False, False] and recs[-1][4] == 1
    return size


@pytest.fixture(scope="module")
def ctx():
    c = N.GpuContext(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def oracle_map(a, b, base):
    """The oracle's count of every n in [a, b), computed once per range: one
    process_range_detailed call that lists every number (cutoff 0), and for
    short ranges and at both ends num_unique_digits number by number."""
    r = O.process_range_detailed(a, b, base, cap=b - a, cutoff=0)
    assert [n for n, _ in r.nice_numbers] == list(range(a, b))
    m = np.array([u for _, u in r.nice_numbers], dtype=np.uint8)
    for n in list(range(a, b)) if b - a <= 1000 else [*range(a, a + 100), *range(b - 100, b)]:
        assert m[n - a] == O.num_unique_digits(n, base)
    return m


def cuts_of(base):
    buf = (ctypes.c_uint64 * 16)()
    n = ctypes.c_size_t()
    assert _lib.lib().nice_fd_segment_cuts(base, buf, 8, n) == 0
    return [buf[2 * i] | (buf[2 * i + 1] << 64) for i in range(n.value)]


def same(got, want):
    """Byte for byte; on a mismatch the first differing positions."""
    assert got.dtype == np.uint8 and got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad.size, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


# --- 1. oracle parity ---------------------------------------------------------------------
def layouts_in_combos_h(base):
    """The base's limb layouts in fd2_combos.h: one fd2_map_kernel (and one
    fd2_batch_kernel) instantiation each."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "nice_amd", "csrc", "fd2_combos.h")) as f:
        text = f.read()
    combos = re.findall(r"X\((\d+), \d+, \d+, \d+\)", text[text.index("#define FD2_COMBOS"):])
    assert len(combos) == 37
    return combos.count(str(base))


def test_the_old_bases_are_fd_bases():
    assert set(FD_BASES) >= {40, 45, 50, 64, 68, 80} and len(FD_BASES) == 24


@pytest.mark.parametrize("base", FD_BASES)
def test_fd_map_equals_oracle(ctx, base):
    """Every base with an FD kernel, every limb layout of it (each is an
    fd2_map_kernel instantiation of its own, and walk_map branches on the
    per-base switches of the kernel configuration: low-digit table or LSDX,
    TIGHT entry, one to three mask words, limbs decoded by VALU, 512 or 1024
    threads, n above 64 bits so that init_at takes the descriptor's digits).
    From the range start: a lone tail workgroup (1, 63), one partial workgroup
    (4 097: chunk 9, so lane runs start at every residue mod 16) and several
    workgroups with a partial last wave and a tail (100 003).  For every layout:
    100 003 numbers and a full workgroup, a partial one and a tail (full_size)
    from its first n, and 4 097 numbers ending at its last.  Across
    every limb-layout cut; across the range end and start, where the FD kernel
    and the generic one share one call."""
    rs, r1 = O.base_range(base)
    want = oracle_map(rs, rs + LONG, base)
    for size in (1, 63, 4097, LONG):
        same(ctx.unique_map(rs, rs + size, base), want[:size])
        st = ctx.map_stats()
        assert (st.fd_numbers, st.generic_numbers, st.generic_segments) == (size, 0, 0) and st.fd_segments == 1
        assert st.launches == 1
    cuts = cuts_of(base)
    # one cut between neighbouring layouts: by the limb counts' own arithmetic and by the header
    assert cuts == F.layout_cuts(base) and len(cuts) + 1 == layouts_in_combos_h(base)
    assert bool(cuts) == (layouts_in_combos_h(base) > 1)
    if base in (64, 68):
        assert not cuts
    edges = [rs] + cuts + [r1]
    for a, e in zip(edges, edges[1:]):
        for x, y in ((a, a + LONG), (a, a + full_size(base)), (e - 4097, e)):
            same(ctx.unique_map(x, y, base), oracle_map(x, y, base))
            st = ctx.map_stats()
            assert (st.fd_segments, st.fd_numbers, st.generic_numbers, st.launches) == (1, y - x, 0, 1), (x, y)
    # (a base with one limb layout has no cut: the same window in mid-range)
    for c in cuts or [rs + (r1 - rs) // 2]:
        same(ctx.unique_map(c - 300, c + 300, base), oracle_map(c - 300, c + 300, base))
        st = ctx.map_stats()
        assert st.fd_segments == (2 if cuts else 1) and st.fd_numbers == 600 and st.launches == st.fd_segments
    same(ctx.unique_map(r1 - 150, r1 + 150, base), oracle_map(r1 - 150, r1 + 150, base))
    st = ctx.map_stats()
    assert (st.fd_numbers, st.generic_numbers, st.fd_segments, st.generic_segments) == (150, 150, 1, 1)
    same(ctx.unique_map(rs - 150, rs + 150, base), oracle_map(rs - 150, rs + 150, base))


def test_generic_map_equals_oracle(ctx):
    got = ctx.unique_map(47, 100, 10)
    same(got, oracle_map(47, 100, 10))
    assert got[69 - 47] == 10
    s, _ = O.base_range(70)
    same(ctx.unique_map(s + 5, s + 5 + 10_007, 70), oracle_map(s + 5, s + 5 + 10_007, 70))
    st = ctx.map_stats()
    assert (st.fd_segments, st.generic_segments, st.fd_numbers, st.generic_numbers) == (0, 1, 0, 10_007)


# --- 2. consistency with the existing kernels ---------------------------------------------
@pytest.mark.parametrize("base,size", [(40, 3 * 10 ** 6), (80, 10 ** 6)])
def test_map_reproduces_the_detailed_field(ctx, base, size):
    """A map of a field is that field's histogram (bincount) and near-miss list
    (the positions above the cutoff), as process_range_detailed returns them."""
    rs, _ = O.base_range(base)
    hist, near = ctx.detailed_raw(rs, rs + size, base)
    assert ctx.kernel_stats().fd_kernel
    m = ctx.unique_map(rs, rs + size, base)
    assert ctx.map_stats().fd_numbers == size
    assert np.bincount(m, minlength=base + 1).tolist() == hist
    pos = np.nonzero(m > O.near_miss_cutoff(base))[0]
    assert [(rs + int(i), int(m[i])) for i in pos] == near


# --- 3. device mode -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_child():
    """tests/map_torch_child.py, run once: what needs torch on the GPU happens in
    a process where torch loaded its HIP runtime before the library did."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "map_torch_child.py")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("base", [40, 60, 80])
def test_device_mode_writes_in_place_at_any_alignment(ctx, torch_child, base):
    """Views at 0, 1, 3 and 15 mod 16 of one owned allocation with at least 64
    guard bytes on either side (100 003 numbers; 63: a lone tail workgroup; a
    tensor longer than the range): the interior equals the host-mode map and no
    guard byte changes (an overrun shows as a failed comparison, not a fault).
    b40 and b80 run 512 threads; b60 runs 1024, so the ring's dword stride is
    4 x 1024, and its low-digit table has the side carry table."""
    d = torch_child["device_mode"][str(base)]
    assert d["aligned"]
    assert [(r["off"], r["n"]) for r in d["runs"]] == [(64, LONG), (65, LONG), (67, LONG), (79, LONG), (64, 63),
                                                       (79, 63), (3, 4097)]
    for r in d["runs"]:
        assert r["guards"] and r["equal"] and r["same_tensor"], r
    assert d["stats"] == [4097, 0, 1]
    # the child's host-mode map is this process's, which the oracle test pins
    rs, _ = O.base_range(base)
    same(np.array(d["host_map_head"], dtype=np.uint8), oracle_map(rs, rs + LONG, base)[:4097])


def test_device_mode_argument_errors(torch_child):
    e = torch_child["device_errors"]
    # a device_index outside the context (either side), a bad flag, a buffer too short: nothing written
    assert e["rcs"] == [_lib.NICE_ERR_INVALID, _lib.NICE_ERR_INVALID, _lib.NICE_ERR_INVALID, _lib.NICE_ERR_CAPACITY]
    assert e["untouched"] and e["wrong_tensors"] == ["ValueError"] * 3


# --- 4. two devices -----------------------------------------------------------------------
def test_two_device_context_equals_one_device(ctx):
    """Host mode over GpuContext([0, 0]): the shard boundary (50 001 numbers in)
    falls inside a workgroup tile of the one-device plan."""
    rs, re = O.base_range(40)
    one = ctx.unique_map(rs, rs + LONG, 40)
    two = N.GpuContext([0, 0])
    try:
        same(two.unique_map(rs, rs + LONG, 40), one)
        st = two.map_stats()
        assert st.fd_segments == 2 and st.fd_numbers == LONG and st.launches == 2
        same(two.unique_map(re - 150, re + 151, 40), oracle_map(re - 150, re + 151, 40))
        same(two.unique_map(47, 48, 10), oracle_map(47, 48, 10))  # fewer numbers than devices
    finally:
        two.close()
    same(one, oracle_map(rs, rs + LONG, 40))


# --- 5. argument errors -------------------------------------------------------------------
def test_argument_errors(ctx):
    L = _lib.lib()
    rs, _ = O.base_range(40)
    buf = np.full(128, 0xEE, dtype=np.uint8)

    def call(base, a, b, out, cap, flags=0, dev=0):
        return L.nice_unique_map(ctx._h, a & MASK, a >> 64, b & MASK, b >> 64, base, out, cap, flags, dev)

    p = buf.ctypes.data
    for base, a, b in [(40, rs + 5, rs + 5), (40, rs + 9, rs + 5), (1, 47, 100), (129, 47, 100),
                       (40, rs, rs + (1 << 32) + 1)]:
        assert call(base, a, b, p, 1 << 40) == _lib.NICE_ERR_INVALID, (base, a, b)
    assert call(10, 47, 100, None, 128) == _lib.NICE_ERR_INVALID
    assert call(10, 47, 100, p, 128, flags=2) == _lib.NICE_ERR_INVALID
    # (refused before the pointer is looked at; with device memory: test_device_mode_argument_errors)
    for dev in (-1, 1):
        assert call(10, 47, 100, p, 128, flags=_lib.NICE_MAP_DEVICE, dev=dev) == _lib.NICE_ERR_INVALID
    # too short: nothing is written
    assert call(40, rs, rs + 100, p, 99) == _lib.NICE_ERR_CAPACITY
    assert (buf == 0xEE).all()
    assert call(40, rs, rs + 100, p, 100) == _lib.NICE_OK
    assert (buf[100:] == 0xEE).all()
    same(buf[:100].copy(), oracle_map(rs, rs + LONG, 40)[:100])


# --- 6. the class survey ------------------------------------------------------------------
def test_class_distribution(torch_child):
    """b40 by n mod 39 on the GPU (the map binned with torch, in the child):
    summed over the classes the table is survey_base's histogram of the same
    windows and seed (the batch kernel's), and it equals the table built from
    the CPU twin's maps."""
    table = torch_child["class_table"]
    assert len(table) == 39 and all(len(row) == 41 for row in table)
    assert [sum(row[u] for row in table) for u in range(41)] == torch_child["survey_distribution"]
    assert sum(map(sum, table)) == 48 * 2500
    assert table == survey.class_distribution(None, 40, 39, windows=48, window_size=2500, seed=11, threads=4)
