"""Child process of tests/test_gpu_map.py: the parts of the map that need torch
on the GPU -- device mode into a torch tensor, survey.class_distribution on a
GPU context.  torch and libnice_hip.so share one HIP runtime only when torch
loads its own first (bench.py's order); in a pytest process other tests have
loaded the library long before, so these run here, in a fresh process, once
for the whole test module.  Prints one JSON line: the raw outcomes, which the
tests assert on.
"""
import json
import os
import sys

import torch

torch.cuda.init()  # before the library loads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import nice_amd as N  # noqa: E402
from nice_amd import _lib, survey  # noqa: E402

LONG = 100_003
MASK = (1 << 64) - 1


def guarded(ctx, alloc, off, a, b, base, want, view_len=None):
    """The map of [a, b) into alloc[off:], every other byte of alloc a guard:
    (the guards are untouched, the interior equals want, the call returned its tensor)."""
    alloc.fill_(0xEE)
    n = b - a
    view = alloc[off:off + (n if view_len is None else view_len)]
    same_tensor = ctx.unique_map(a, b, base, out=view) is view and view.data_ptr() == alloc.data_ptr() + off
    host = alloc.cpu().numpy()
    guards = bool((host[:off] == 0xEE).all() and (host[off + n:] == 0xEE).all())
    return {"off": off, "n": n, "guards": guards, "equal": bool((host[off:off + n] == want[:n]).all()),
            "same_tensor": bool(same_tensor)}


def device_mode(ctx, base):
    rs = N.get_base_range_u128(base).range_start
    want = ctx.unique_map(rs, rs + LONG, base)  # host mode (the tests pin it to the oracle)
    alloc = torch.empty(LONG + 64 + 80, dtype=torch.uint8, device="cuda:0")
    out = {"aligned": alloc.data_ptr() % 16 == 0, "host_map_head": want[:4097].tolist(), "runs": []}
    for off in (64, 65, 67, 79):  # 0, 1, 3 and 15 mod 16, >= 64 guard bytes on either side
        out["runs"].append(guarded(ctx, alloc, off, rs, rs + LONG, base, want))
    for off in (64, 79):  # a lone tail workgroup: one byte per lane
        out["runs"].append(guarded(ctx, alloc, off, rs, rs + 63, base, want))
    # a tensor longer than the range: only the range's bytes are written
    out["runs"].append(guarded(ctx, alloc, 3, rs, rs + 4097, base, want, view_len=alloc.numel() - 3))
    st = ctx.map_stats()
    out["stats"] = [st.fd_numbers, st.generic_numbers, st.launches]
    return out


def device_errors(ctx):
    rs = N.get_base_range_u128(40).range_start
    L = _lib.lib()
    dbuf = torch.full((128,), 0xEE, dtype=torch.uint8, device="cuda:0")

    def call(cap, flags, dev):
        return L.nice_unique_map(ctx._h, rs & MASK, rs >> 64, (rs + 100) & MASK, (rs + 100) >> 64, 40,
                                 dbuf.data_ptr(), cap, flags, dev)

    rcs = [call(128, _lib.NICE_MAP_DEVICE, -1), call(128, _lib.NICE_MAP_DEVICE, 1), call(128, 2, 0),
           call(99, _lib.NICE_MAP_DEVICE, 0)]
    untouched = bool((dbuf == 0xEE).all())
    wrong = []
    for bad in (torch.empty(16, dtype=torch.uint8), torch.empty(16, dtype=torch.int32, device="cuda:0"),
                torch.empty((4, 4), dtype=torch.uint8, device="cuda:0")):
        try:
            ctx.unique_map(rs, rs + 10, 40, out=bad)
            wrong.append("accepted")
        except ValueError:
            wrong.append("ValueError")
    return {"rcs": rcs, "untouched": untouched, "wrong_tensors": wrong}


def main():
    ctx = N.GpuContext(0)
    try:
        kw = dict(windows=48, window_size=2500, seed=11)
        out = {"device_mode": {str(b): device_mode(ctx, b) for b in (40, 60, 80)},
               "device_errors": device_errors(ctx),
               "class_table": survey.class_distribution(ctx, 40, 39, **kw),
               "survey_distribution": survey.survey_base(ctx, 40, **kw).distribution}
    finally:
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
