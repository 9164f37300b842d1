"""One b40 1e9 field in rounds (mode 2) and on the persistent sibling grid
(mode 1), for a counters-only rocprofv3 --pmc pass (the two kernels have
different names, so the summary keeps them apart)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nice_amd as N  # noqa: E402
from nice_amd import _lib  # noqa: E402

L = _lib.lib()
ctx = N.GpuContext(0)
s = N.get_base_range_u128(40).range_start
for mode in (2, 1):
    assert L.nice_debug_force_sib_persistent(mode, 0) == 0
    assert L.nice_debug_force_sib_stride(143) == 0
    hist, _ = ctx.detailed_raw(s, s + 10 ** 9, 40)
    assert sum(hist) == 10 ** 9
    print(mode, ctx.kernel_stats())
ctx.close()
