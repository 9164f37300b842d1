"""The FD kernels whose limb arithmetic runs on the f32 FMA pipe (Cfg::FMA,
fd2_kernel.hpp: b40's sibling-lane kernels) against the oracle's histogram and
near-miss list, and against their own integer form through the probe library;
and one base per other class of step, which keep the integer form today (they
pin what a later switch of the flag there has to reproduce).  nice_debug_set_near_miss_cutoff lowers the cutoff to the top of the
histogram window, so the list is not empty and every entry is compared.

A wrong limb (an FMA fed a wrapped integer, a flushed subnormal) corrupts
every later number of a lane's run, so the comparisons are exact.

Run on the MI355X box:  python -m pytest tests/test_gpu_fd_fma.py -m gpu -q -rA
"""
import functools
import json
import os
import subprocess
import sys

import pytest

import nice_amd as N
from nice_amd import _lib
from oracle import oracle as O

import near_miss_windows as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = N.GpuContext(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def want(a, e, base, cutoff):
    return W.oracle(a, e, base, cutoff)


def same(got, exp, cutoff, what, at_least=1):
    (h, lst), (hw, lw) = got, exp
    assert len(lw) >= at_least, f"{what}: the expected list has {len(lw)} entries"
    assert h == hw, f"{what}: histogram"
    assert lst == lw, f"{what}: list ({len(lst)} entries, expected {len(lw)})"
    assert len(lst) == sum(h[cutoff + 1:]), f"{what}: list length against the bins above the cutoff"
    print(f"near-miss entries, {what}: {len(lst)}")


def layout_end(base, k=0):
    """The end (exclusive) of the base's k-th limb layout: a segment ending
    there is the last one the layout holds; the range's end without cuts."""
    cuts = W.cuts_of(base)
    return cuts[k] if k < len(cuts) else O.base_range(base)[1]


# The smallest field that takes the pipelined sibling walk: four super-blocks
# of 3 B^2 numbers (B = 40^2) and a ragged remainder, the lane stride the walk
# picks on a 1e9 field forced (a lone field this short would otherwise leave
# the sibling kernel, plan_sib); 143 leaves an edge unit per block.
B40_FIELD = 4 * 3 * 40 ** 4 + 1_234_567
B40_STRIDE = 143


@pytest.mark.parametrize("where", ["range start", "end of the ND = 4 layout"])
def test_b40_pipelined_sibling_walk(ctx, where):
    """b40's bench kernel (three sibling lanes, pipelined walk, FMA limb
    arithmetic) at the range start and ending on the last number of the
    ND = 4 layout, where the limb values and sums are largest."""
    r0, _ = O.base_range(40)
    e = r0 + B40_FIELD if where == "range start" else layout_end(40)
    s = e - B40_FIELD
    assert s >= r0 and not any(s < cut < e for cut in W.cuts_of(40))
    lib = _lib.lib()
    with W.lowered(40) as c:
        exp = want(s, e, 40, c)
        try:
            assert lib.nice_debug_force_sib_stride(B40_STRIDE) == 0
            got = ctx.detailed_raw(s, e, 40)
            st = ctx.kernel_stats()
        finally:
            lib.nice_debug_force_sib_stride(0)
        assert (st.sib_lanes, st.sib_stride, st.fd_kernel) == (3, B40_STRIDE, True), st  # the sibling kernel ran
        same(got, exp, c, f"b40 pipelined sibling walk, {where}")


def test_b40_lookup_group_sibling_walk(ctx):
    """b40's other sibling kernel (per-sibling lookup groups, the layouts past
    ND = 4), ending on the last number of the range."""
    e = O.base_range(40)[1]
    s = e - B40_FIELD
    assert not any(s < cut < e for cut in W.cuts_of(40))
    lib = _lib.lib()
    with W.lowered(40) as c:
        exp = want(s, e, 40, c)
        try:
            assert lib.nice_debug_force_sib_stride(81) == 0
            got = ctx.detailed_raw(s, e, 40)
            st = ctx.kernel_stats()
        finally:
            lib.nice_debug_force_sib_stride(0)
        assert (st.sib_lanes, st.sib_stride, st.fd_kernel) == (3, 81, True), st
        same(got, exp, c, "b40 lookup-group sibling walk, range end")


@pytest.mark.parametrize("base", [44, 52, 58, 64, 80])
def test_other_base_classes(ctx, base):
    """(These kernels run the integer form in production: this pins their
    results where the limbs are largest, for the day the flag goes on there.)
    One base per class of step: b44 (three siblings, per-sibling lookups),
    b52 (two siblings, short table), b58 (bare-carry low-digit entry, TIGHT),
    b64 (B = 4096, no bias) and b80 (ES = 16, the multiply-high on t, limb 0
    by VALU): 1e6 numbers ending on the last number of the first limb layout's
    segment, where the limbs are largest.  Up there n^2 and n^3 begin with the
    same few digits for every n of the window and the lowered cutoff still lists
    nothing on most of these bases (the histogram is the comparison), so the
    base's near_miss_windows.py window, where the list has >= 8 entries, runs
    too."""
    e = layout_end(base)
    with W.lowered(base) as c:
        for (a, b), at_least in (((e - 10 ** 6, e), 0), (W.window(base), W.MIN_ENTRIES)):
            exp = want(a, b, base, c)
            got = ctx.detailed_raw(a, b, base)
            assert ctx.kernel_stats().fd_kernel
            same(got, exp, c, f"b{base} [{a}, {b})", at_least)


# --- the flag off and on, same kernel otherwise (probe library) ------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_LIB = os.path.join(ROOT, "nice_amd", "libnice_hip_probe.so")

_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import nice_amd as N
from nice_amd import _lib
import near_miss_windows as W
s, e, stride = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
ctx = N.GpuContext(0)
lib = _lib.lib()
with W.lowered(40) as c:
    assert lib.nice_debug_force_sib_stride(stride) == 0
    h, lst = ctx.detailed_raw(s, e, 40)
    st = ctx.kernel_stats()
    lib.nice_debug_force_sib_stride(0)
print(json.dumps({"hist": h, "list": lst, "sib": [st.sib_lanes, st.sib_stride, bool(st.fd_kernel)], "cutoff": c}))
ctx.close()
"""


def _probe_run(knob, s, e, stride):
    env = dict(os.environ, NICE_LIB_PATH=PROBE_LIB, NICE_FD2_SIB=str(knob))
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(s), str(e), str(stride)], env=env,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.splitlines()[-1])


@pytest.mark.skipif(not os.path.exists(PROBE_LIB), reason="no probe build (make -C nice_amd probe)")
@pytest.mark.parametrize("off,on,where,stride", [
    (142, 242, "start", B40_STRIDE),     # pipelined walk: NICE_FD2_SIB 142 integer, 242 FMA
    (131, 231, "end", 81),               # lookup-group walk: 131 integer, 231 FMA
])
def test_b40_flag_off_and_on(off, on, where, stride):
    """The same b40 sibling kernel with the limb arithmetic in its integer form
    and on the f32 pipe (the probe library's NICE_FD2_SIB cases; each in a
    process of its own, a process reading the knob once): histograms and
    near-miss lists at the lowered cutoff are equal, and not empty."""
    r0, r1 = O.base_range(40)
    s, e = (r0, r0 + B40_FIELD) if where == "start" else (r1 - B40_FIELD, r1)
    a, b = _probe_run(off, s, e, stride), _probe_run(on, s, e, stride)
    assert a["sib"] == b["sib"] == [3, stride, True], (a["sib"], b["sib"])
    assert sum(a["hist"]) == B40_FIELD and len(a["list"]) >= 1
    assert a["hist"] == b["hist"]
    assert a["list"] == b["list"]
    print(f"b40 NICE_FD2_SIB {off} / {on}: {len(a['list'])} near-miss entries, equal")
