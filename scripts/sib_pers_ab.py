"""Rounds (mode 2) against the persistent sibling grid (mode 1), alternated in
one process on the product library: b40 fields at the range start, pipelined
(both modes, depth 2; ms per step) and lone (synchronous detailed call: wall
and kernel_ms).

    python scripts/sib_pers_ab.py SIZE [SIZE ...]
"""
import statistics
import sys
import time

import os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nice_amd as N  # noqa: E402
from nice_amd import _lib  # noqa: E402
from nice_amd import dist as D  # noqa: E402

L = _lib.lib()
base = 40
ctx = N.GpuContext(0)
s = N.get_base_range_u128(base).range_start


def pipelined(field, steps):
    pipe = D.FieldPipeline(ctx, ctx, None, depth=2)
    for _ in range(8):
        pipe.step(field, base)
    pipe.drain()
    ctx.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        pipe.step(field, base)
    pipe.drain()
    ctx.synchronize()
    return (time.perf_counter() - t) / steps * 1e3


def lone(field, reps):
    wall, kern = [], []
    for _ in range(3):
        ctx.detailed_raw(field.range_start, field.range_end, base)
    for _ in range(reps):
        t = time.perf_counter()
        ctx.detailed_raw(field.range_start, field.range_end, base)
        wall.append((time.perf_counter() - t) * 1e3)
        kern.append(ctx.kernel_stats().kernel_ms)
    return statistics.median(wall), statistics.median(kern)


for arg in sys.argv[1:]:
    size = int(float(arg))
    field = N.FieldSize(s, s + size)
    steps = max(40, int(2e11 / size / 4))
    rows = {1: [], 2: []}
    for rep in range(4):
        for mode in (2, 1):
            assert L.nice_debug_force_sib_persistent(mode, 0) == 0
            p = pipelined(field, steps)
            st = ctx.kernel_stats()
            w, k = lone(field, 9)
            st2 = ctx.kernel_stats()
            rows[mode].append((p, w, k))
            print(f"size {size:.2e} mode {mode} rep {rep}: pipelined {p:.4f} ms/step (L {st.sib_stride} grid {st.sib_grid}); "
                  f"lone wall {w:.4f} kernel {k:.4f} (L {st2.sib_stride} grid {st2.sib_grid})", flush=True)
    for i, nm in enumerate(("pipelined ms/step", "lone wall ms", "lone kernel ms")):
        a = [r[i] for r in rows[2]]
        b = [r[i] for r in rows[1]]
        print(f"  {size:.2e} {nm}: rounds median {statistics.median(a):.4f} [{min(a):.4f}, {max(a):.4f}]  persistent median "
              f"{statistics.median(b):.4f} [{min(b):.4f}, {max(b):.4f}]  ratio {statistics.median(b) / statistics.median(a):.4f}")
L.nice_debug_force_sib_persistent(0, 0)
ctx.close()
