"""The niceonly device MSD's batch plans and launch grids
(nice_amd/csrc/msd_plan.hpp), on the CPU: tests/msd_plan_dump.cpp is built
host-only from msd_plan.hpp and layout.h -- that compile is itself the check
that the two headers need no GPU toolchain -- and prints the plan and every
grid over chunk sizes, floors, chunk counts, device counts and CU counts.  What
is asserted is what the host code (abi_niceonly.cpp run_device_msd) and the
kernels (niceonly_msd.hpp, niceonly_wave.hpp) assume of a plan: batches tile
the caller's chunks exactly once, the buffer sizes the host narrows to 32 bits
fit them, a wave root fits StackNode::size, and every grid lies in [1, its cap].
"""
import itertools
import os
import re
import shutil
import subprocess
from collections import namedtuple

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nice_amd", "csrc")
U32 = 0xFFFFFFFF

CHUNKS = (10 ** 4, 10 ** 6, 10 ** 8, 2 ** 32 - 1, 2 ** 32, 2 ** 40, 2 ** 40 + 1)
FLOORS = (1, 64, 250, 2 ** 20, 2 ** 30, 2 ** 35)
MINES = (1, 7, 1000, 2 ** 24 + 1)
DEVICES = (1, 2, 8)
CUS = (64, 256, 304)
NOFUSE = (0, 1)

TOO_LARGE, TOO_LARGE_FOR_FLOOR = 1, 2  # kMsdChunkTooLarge, kMsdChunkTooLargeForFloor
FUSED_MAX = 1 << 14  # layout.h kFusedMaxCap
WAVES_PER_GROUP, STACK_CAP, STACK_NODE = 8, 2048, 16  # layout.h kWaveWG / 64, kStackCap, kStackNodeBytes

Plan = namedtuple("Plan", "err cpb per leaf_cap fcap wave wlevel wgrid wleaf_cap nbatches")
Case = namedtuple("Case", "chunk floor mine devices cus nofuse recs")


def ceil_div(a, b):
    return -(-a // b)


def one(case, tag):
    (r,) = [f for t, f in case.recs if t == tag]
    return r


def plan(case):
    return Plan(*one(case, "P"))


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("msd_plan") / "msd_plan_dump")
    # no GPU compiler and no GPU include path
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, os.path.join(ROOT, "tests", "msd_plan_dump.cpp"), "-o", exe],
                   check=True)
    grid = itertools.product(CHUNKS, FLOORS, MINES, DEVICES, CUS, NOFUSE)
    inp = "".join("%d %d %d %d %d %d\n" % g for g in grid)
    out = subprocess.run([exe], input=inp, capture_output=True, text=True, check=True).stdout
    res = []
    for line in out.splitlines():
        f = line.split()
        if f[0] == "K":
            res.append(Case(*map(int, f[1:]), []))
        else:
            res[-1].recs.append((f[0], tuple(map(int, f[1:]))))
    return res


def test_plan_headers_need_no_gpu_runtime():
    for name in ("msd_plan.hpp", "layout.h"):
        text = open(os.path.join(CSRC, name)).read()
        assert not re.search(r"\bhip|__device__|__global__|probe_knob|probe_set|getenv", text), name
        for inc in re.findall(r'#include\s+[<"]([^>"]+)[>"]', text):
            assert inc in ("stddef.h", "stdint.h", "algorithm", "layout.h"), (name, inc)


def test_grid_is_complete(cases):
    want = list(itertools.product(CHUNKS, FLOORS, MINES, DEVICES, CUS, NOFUSE))
    assert [tuple(c[:6]) for c in cases] == want and len(want) == 7 * 6 * 4 * 3 * 3 * 2
    kinds = {(bool(plan(c).fcap), bool(plan(c).wave)) for c in cases if not plan(c).err}
    assert kinds == {(True, False), (False, True)}  # fused and wave plans; the product never plans the level BFS alone
    for c in cases:
        assert one(c, "W")[0] == WAVES_PER_GROUP if not plan(c).err else len(c.recs) == 2


def test_errors(cases):
    """The two error strings, for exactly the cases that produce them: a chunk
    above 2^40; a wave plan whose nodes at the last level with splits (the
    deepest root level it may pick) still hold more than 2^26 numbers."""
    n = {TOO_LARGE: 0, TOO_LARGE_FOR_FLOOR: 0}
    for c in cases:
        err = plan(c).err
        fl = min(c.floor, 2 ** 30)
        last = 0
        while last < 22 and ceil_div(c.chunk, 2 ** last) >= 2 * fl:
            last += 1
        fused = one(c, "F")[0] and not c.nofuse
        if c.chunk > 2 ** 40:
            assert err == TOO_LARGE, c[:6]
        elif not fused and ceil_div(c.chunk, 2 ** last) > 2 ** 26:
            assert err == TOO_LARGE_FOR_FLOOR, c[:6]
        else:
            assert err == 0, c[:6]
        if err:
            n[err] += 1
    assert n[TOO_LARGE] == len(cases) // len(CHUNKS) and n[TOO_LARGE_FOR_FLOOR] > 0


def test_fused_cap(cases):
    for c in cases:
        (cap,) = one(c, "F")
        need = c.chunk // c.floor + 2
        if c.chunk >= 2 ** 32 or need > FUSED_MAX:
            assert cap == 0, c[:6]
        else:
            assert 64 <= cap <= FUSED_MAX and cap & (cap - 1) == 0 and cap >= need, c[:6]
            assert cap == 64 or cap // 2 < need, c[:6]  # the smallest such power of two
        if not plan(c).err:
            assert plan(c).fcap == (0 if c.nofuse else cap), c[:6]


def test_batches_tile_the_chunks(cases):
    n = 0
    for c in cases:
        pl = plan(c)
        if pl.err:
            continue
        n += 1
        ctx = (c[:6], pl)
        assert pl.cpb >= 1 and pl.cpb * pl.nbatches >= c.mine and (pl.nbatches - 1) * pl.cpb < c.mine, ctx
        if pl.wave and c.devices > 1:
            assert pl.nbatches >= min(c.mine, c.devices), ctx
        # what run_device_msd narrows to uint32_t
        assert pl.per <= U32 and pl.leaf_cap <= U32 and pl.wleaf_cap <= U32, ctx
        assert pl.wave == (pl.fcap == 0), ctx
    assert n > 1000


def test_wave_plans(cases):
    n = 0
    for c in cases:
        pl = plan(c)
        if pl.err or not pl.wave:
            continue
        n += 1
        ctx = (c[:6], pl)
        planner_last, _ = one(c, "L")
        assert pl.wlevel <= planner_last <= 22, ctx
        assert ceil_div(c.chunk, 2 ** pl.wlevel) <= 2 ** 26, ctx  # StackNode::size
        roots = pl.cpb << pl.wlevel
        assert roots < 2 ** 64 and roots + 64 <= pl.per, ctx  # launch_msd_wave's check; the root level's queue
        assert pl.wgrid * WAVES_PER_GROUP == 16 * max(256, c.cus), ctx
        assert one(c, "W") == (WAVES_PER_GROUP, pl.wgrid * WAVES_PER_GROUP * STACK_CAP * STACK_NODE), ctx
    assert n > 500


def test_last_levels(cases):
    for c in cases:
        if plan(c).err:
            continue
        planner, launcher = one(c, "L")
        assert planner <= 22 and launcher <= 22, c[:6]
        if c.floor <= 2 ** 30:
            assert planner == launcher, c[:6]
        else:
            assert planner >= launcher, c[:6]
        # the first level whose largest node cannot split (or 22)
        assert launcher == 22 or ceil_div(c.chunk, 2 ** launcher) < 2 * c.floor, c[:6]
        assert launcher == 0 or ceil_div(c.chunk, 2 ** (launcher - 1)) >= 2 * c.floor, c[:6]


def test_grids(cases):
    n = 0
    for c in cases:
        pl = plan(c)
        if pl.err:
            continue
        _, launcher = one(c, "L")
        tail = c.mine - (pl.nbatches - 1) * pl.cpb
        seen = set()
        for tag, f in c.recs:
            ctx = (c[:6], tag, f)
            if tag == "U":
                chunks, grid = f
                assert chunks in (pl.cpb, tail) and grid == min(chunks, 4 * c.cus) and 1 <= grid <= 4 * c.cus, ctx
            elif tag == "G":
                nchunks, level, grid = f
                seen.add((nchunks, level))
                assert 1 <= grid <= 2 * c.cus and grid == min(ceil_div(nchunks << level, 256), 2 * c.cus), ctx
            elif tag == "N":
                on_device, n_leaves, cap, grid = f
                waves = 32 * c.cus if on_device else ceil_div(n_leaves, 8)
                assert 1 <= grid <= cap and grid == max(1, min(ceil_div(waves, 4), cap)), ctx
                n += 1
        assert seen == {(m, lv) for m in (pl.cpb, tail) for lv in range(launcher + 1)}, c[:6]
    assert n > 1000
