"""Phase stamps of the b40 sibling kernel on the bench field (probe build):
lone (synchronous) and pipelined (detailed + niceonly, depth 2).  Per
workgroup: DMA + init, thread 0's steps, wait for the other waves, flush;
per wave its finish time; the share of wave time outside the steps.

    python scripts/sib_pers_stamps.py SIZE [MODE]     (MODE: the sib-persistent hook's mode, if present)
"""
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import probe_lib  # noqa: E402,F401

import nice_amd as N  # noqa: E402
from nice_amd import _lib  # noqa: E402
from nice_amd import dist as D  # noqa: E402

L = _lib.lib()
L.nice_probe_fd2_stamps.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t]
L.nice_probe_fd2_stamps.restype = ctypes.c_int
L.nice_probe_fd2_last.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
GROUPS, WORDS = 65536, 32
size = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10 ** 9
mode = int(sys.argv[2]) if len(sys.argv) > 2 else None
if mode is not None:
    L.nice_debug_force_sib_persistent.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    L.nice_debug_force_sib_persistent.restype = ctypes.c_int
    assert L.nice_debug_force_sib_persistent(mode, 0) == 0
base = 40
ctx = N.GpuContext(0)
s = N.get_base_range_u128(base).range_start
field = N.FieldSize(s, s + size)


def read_stamps():
    geo = (ctypes.c_uint64 * 6)()
    L.nice_probe_fd2_last(geo)
    buf = (ctypes.c_uint64 * (GROUPS * WORDS))()
    assert L.nice_probe_fd2_stamps(0, buf, GROUPS * WORDS) == 0
    wgs = []
    for b in range(GROUPS):
        w = buf[WORDS * b: WORDS * b + WORDS]
        if w[0] == 0 or w[12] == 0:
            continue
        wgs.append((b, [w[2 * k] for k in range(16)], [w[2 * k + 1] for k in range(16)], list(w[20:28])))
    return geo, wgs


def report(tag, geo, wgs, nsib):
    """nsib: workgroups [0, nsib) are the sibling part (the others: edge, remainder)."""
    print(f"== {tag}: {len(wgs)} stamped workgroups; last launch grid {geo[0]} x {geo[1]}, L {geo[2]}, "
          f"{geo[3]} sibling units, remainder {geo[4]}, {geo[5]} per CU")
    # (pipelined: a slot can hold stamps of two fields' workgroups; keep the consistent ones)
    wgs = [x for x in wgs if 0 < x[2][6] - x[2][0] < 5e7 and 0 < x[1][6] - x[1][0] < 5e6]
    sib = [x for x in wgs if x[0] < nsib and x[2][0] <= x[2][14] <= x[2][15] <= x[2][4] <= x[2][6]]
    print(f"   {len(wgs)} consistent records, {len(sib)} of the sibling part")
    cyc = lambda x, a, b: x[2][b] - x[2][a]  # noqa: E731  shader clock
    med = statistics.median
    names = [("DMA+init (0->14)", 0, 14), ("steps t0 (14->15)", 14, 15), ("wait others (15->4)", 15, 4),
             ("flush (4->5)", 4, 5), ("arrive/finish (5->6)", 5, 6), ("life (0->6)", 0, 6)]
    for nm, a, b in names:
        d = [cyc(x, a, b) for x in sib if x[2][a] and x[2][b] and x[2][b] >= x[2][a]]
        if d:
            print(f"   {nm:22s} cycles median {med(d):10.0f}  mean {statistics.mean(d):10.0f}  max {max(d):10.0f}")
    # real-time (100 MHz) span and slot-time accounting
    rt0 = min(x[1][0] for x in wgs)
    rt1 = max(x[1][6] for x in wgs)
    life_rt = sum(x[1][6] - x[1][0] for x in wgs)
    print(f"   in-kernel span {(rt1 - rt0) / 100:.1f} us; sum of workgroup lives {life_rt / 100:.0f} us "
          f"= {life_rt / (rt1 - rt0):.1f} resident workgroups on average (512 slots)")
    # share of wave time outside steps: waves finish at w[k] (shader clock), start stepping at phase 1
    tot = out = 0
    spreads, idle = [], []
    for x in sib:
        ws = [t for t in x[3] if t]
        t0, t1, t6 = x[2][0], x[2][14], x[2][6]
        if len(ws) != 8 or not (t0 and t1 and t6) or t6 < t0 or min(ws) < t1 or max(ws) > t6:
            continue
        tot += 8 * (t6 - t0)
        out += 8 * (t6 - t0) - sum(t - t1 for t in ws)
        spreads.append(max(ws) - min(ws))
        idle.append(sum(max(ws) - t for t in ws) / 8)
    if tot:
        print(f"   per-wave finish stamps on {len(spreads)} workgroups: spread (last - first wave) median "
              f"{med(spreads):.0f} cycles, mean {statistics.mean(spreads):.0f}, max {max(spreads)}")
        print(f"   a wave's wait for the workgroup's slowest: mean {statistics.mean(idle):.0f} cycles "
              f"({statistics.mean(idle) * 8 * len(idle) / tot:.4f} of resident wave time)")
        print(f"   share of resident wave time outside the steps (DMA/init barrier, waiting for the slowest "
              f"wave, flush, arrival): {out / tot:.4f}")
    else:
        d3 = [cyc(x, 0, 6) for x in sib]
        d2 = [cyc(x, 2, 3) for x in sib]
        print(f"   (no per-wave stamps) thread 0 outside its steps: {1 - sum(d2) / sum(d3):.4f}")


# lone
for _ in range(3):
    ctx.detailed_raw(s, s + size, base)
ev = []
for _ in range(5):
    ctx.detailed_raw(s, s + size, base)
    ev.append(ctx.kernel_stats().kernel_ms)
assert L.nice_probe_fd2_stamps(1, None, 0) == 0
hist, _ = ctx.detailed_raw(s, s + size, base)
assert sum(hist) == size
st = ctx.kernel_stats()
print(f"b{base} {size:.1e} lone: kernel_ms unstamped median {statistics.median(ev):.4f}, stamped {st.kernel_ms:.4f}; "
      f"sib_lanes {st.sib_lanes} stride {st.sib_stride} launches {st.launches} "
      f"sib_grid {getattr(st, 'sib_grid', None)}")
geo, wgs = read_stamps()
B2 = base ** 4
upb = (B2 + geo[2] - 1) // geo[2] - (0 if B2 % geo[2] == 0 else 1)
sg = getattr(st, 'sib_grid', 0) or 0
nsib = sg if sg else (geo[3] + 511) // 512
report("lone", geo, wgs, nsib)

# pipelined, both modes
pipe = D.FieldPipeline(ctx, ctx, None, depth=2)
for _ in range(6):
    pipe.step(field, base)
pipe.drain()
assert L.nice_probe_fd2_stamps(1, None, 0) == 0
for _ in range(6):
    r = pipe.step(field, base)
    if r is not None:
        assert sum(d.count for d in r[1].distribution) == size
for r in pipe.drain():
    assert sum(d.count for d in r[1].distribution) == size
geo, wgs = read_stamps()
sg = getattr(ctx.kernel_stats(), 'sib_grid', 0) or 0
nsib = sg if sg else (geo[3] + 511) // 512
report("pipelined depth 2, both modes (stamps of the fields' last writers)", geo, wgs, nsib)
ctx.close()
