"""The FD detailed kernel's launch plans (nice_amd/csrc/fd2_plan.hpp), on the
CPU: tests/fd2_plan_dump.cpp is built host-only from fd2_cfg.hpp and
fd2_plan.hpp -- that compile is itself the check that the two headers need no
GPU toolchain -- and prints the plans of the configurations fd2_part.hip
dispatches to over a grid of devices, starts and counts.  What is asserted is
what the device code (fd2_kernel.hpp) assumes of a launch: the numbers are
tiled exactly once, unit and block counts fit their 32-bit words, a chunk
stays inside the low-digit table and a lane's u16 counters, and the chunk's
parity keeps a wave's lookups off one bank.
"""
import os
import re
import shutil
import subprocess
from collections import namedtuple

import pytest

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nice_amd", "csrc")
BASES = (40, 44, 50, 52, 80)
SIB_CFGS = ("b40_sib3_pipe", "b40_sib3", "b44_sib3", "b52_sib2")
ALL_CFGS = SIB_CFGS + ("b40_512", "b50_big", "b80_big", "b80_512")
U32 = 0xFFFFFFFF

Cfg = namedtuple("Cfg", "WG B LDE SIB LSD PERS HQ TCHUNK")
Case = namedtuple("Case", "cfg cus per_cu start count overlapped forced recs")


def _cuts(base):
    """The n where a segment's limb layout changes (fd2_detailed.hip), by exact
    integer search; see tests/test_abi.py."""
    B = base * base

    def limbs(x):
        k = 0
        while x >= B ** k:
            k += 1
        return k

    def combo(e):
        return (limbs(2 * e + 1), limbs(3 * e * e + 3 * e + 1), limbs(6 * e + 6))

    s, e = O.base_range(base)
    cuts, a = [], s
    while combo(a + 1) != combo(e):
        lo, hi, cur = a + 1, e, combo(a + 1)
        while lo < hi:
            mid = (lo + hi) // 2
            if combo(mid) == cur:
                lo = mid + 1
            else:
                hi = mid
        cuts.append(lo - 1)
        a = lo - 1
    return cuts


def _starts(base):
    """The range's start, its middle, and 777 above a limb-layout cut (b44 and
    b52 keep one layout over their whole range: no third start)."""
    s, e = O.base_range(base)
    return [s, (s + e) // 2] + [c + 777 for c in _cuts(base)[:1]]


def ceil_div(a, b):
    return -(-a // b)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("fd2_plan") / "fd2_plan_dump")
    # no GPU compiler and no GPU include path
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, os.path.join(ROOT, "tests", "fd2_plan_dump.cpp"), "-o", exe],
                   check=True)
    inp = "".join("%d %d\n" % (b, s) for b in BASES for s in _starts(b))
    out = subprocess.run([exe], input=inp, capture_output=True, text=True, check=True).stdout
    cfgs, cases, picks = {}, [], {}
    for line in out.splitlines():
        f = line.split()
        tag = f[0]
        if tag == "K":
            cases.append(Case(f[1], int(f[2]), int(f[3]), int(f[4]), int(f[5]), int(f[6]), int(f[7]), []))
        elif tag == "C":
            cfgs[f[1]] = Cfg(*map(int, f[2:]))
        elif tag == "P":
            picks[f[1]] = (int(f[2]), int(f[3]))
        else:
            cases[-1].recs.append((tag, tuple(map(int, f[1:]))))
    return cfgs, cases, picks


def test_plan_headers_need_no_gpu_runtime():
    for name in ("fd2_cfg.hpp", "fd2_plan.hpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert not re.search(r"\bhip|__device__|__global__|probe_knob|g_force_sib_stride|getenv", text), name
        for inc in re.findall(r'#include\s+[<"]([^>"]+)[>"]', text):
            assert inc in ("algorithm", "cmath", "map", "mutex", "vector", "type_traits", "layout.h"), (name, inc)


def test_grid_is_complete(plans):
    cfgs, cases, _ = plans
    assert set(cfgs) == set(ALL_CFGS)
    per_start = 2 * 3 * 15  # devices x occupancies x counts
    nstarts = {b: len(_starts(b)) for b in BASES}
    assert nstarts == {40: 3, 44: 2, 50: 3, 52: 2, 80: 3}
    for name in ALL_CFGS:
        n = sum(1 for c in cases if c.cfg == name)
        variants = 2 + 2 * 106 if name in SIB_CFGS else 1  # overlapped 0 / 1, and every odd forced L in [45, 255]
        assert n == nstarts[int(name[1:3])] * per_start * variants, name
    # the dispatch reaches every kind of launch
    kinds = {(c.cfg, r[0]) for c in cases for r in c.recs}
    for name in SIB_CFGS:
        assert (name, "N") in kinds and (name, "S") in kinds and (name, "T") in kinds
    assert any(r[0] == "R" and r[1][4] for c in cases if c.cfg == "b80_big" for r in c.recs)  # persistent grid
    assert any(r[0] == "R" and not r[1][4] for c in cases if c.cfg == "b80_big" for r in c.recs)  # ... and rounds
    assert not any(r[0] in "EX" for c in cases for r in c.recs)


def test_pinned_picks(plans):
    """The bench field (b40, start 1 916 284 264 916, 1e9 numbers, the pipelined
    three-sibling kernel): the model's pick over [105, 210] at target 140, and
    the lone field's whole-rounds pick on 262 144 lanes (fd2_plan.hpp plan_sib)."""
    assert plans[2] == {"b40_sib3_pipe": (143, 159)}


def _check_regular(case, recs):
    at = 0
    for tag, f in recs:
        assert tag == "R", case[:7]
        wg, B, lsd, hq, pers, off, cnt, chunk, nunits, tail, grid, main_blocks, wave_cap = f
        ctx = (case[:7], f)
        assert off == at and cnt >= 1, ctx  # contiguous
        at += cnt
        assert nunits * chunk + tail == cnt and tail < chunk and 1 <= chunk <= B, ctx
        if lsd:
            assert chunk == 1 or chunk % 2 == 1, ctx
        else:
            assert chunk % 16 != 0, ctx
        assert nunits <= U32 and grid <= U32, ctx
        assert main_blocks == ceil_div(nunits, wg), ctx
        if pers:
            nb = ceil_div(nunits, 64) + ceil_div(tail, 64)
            assert 1 <= grid <= case.cus * case.per_cu and nunits <= 0xFFFFFFC0, ctx
            assert wave_cap == 65535 // chunk and ceil_div(nb, grid) <= (wg // 64) * wave_cap, ctx
        else:
            assert grid == main_blocks + ceil_div(tail, wg), ctx
            assert chunk <= 65535, ctx  # a lane's u16 window counter holds its one chunk
        if hq == 4:
            assert chunk <= 255, ctx
    assert at == case.count, case[:7]


def test_regular_launches(plans):
    cfgs, cases, _ = plans
    n = 0
    for c in cases:
        if cfgs[c.cfg].SIB == 1:
            _check_regular(c, c.recs)
            n += 1
        elif c.recs[0][0] == "N":
            _check_regular(c, c.recs[1:])
            n += 1
    assert n > 1000


def test_sibling_launches(plans):
    cfgs, cases, _ = plans
    n = 0
    for c in cases:
        P = cfgs[c.cfg]
        if P.SIB == 1:
            continue
        M, D, lmax = P.SIB, P.B * P.B, P.LDE - P.B
        SB = M * D
        if c.count < 4 * SB:
            assert c.recs[0][0] == "N", c[:7]
            continue
        if c.recs[0][0] == "N":
            # only the small-field fallback: a lone field, no forced stride
            assert not c.forced and not c.overlapped, c[:7]
            continue
        n += 1
        tag, (L, U, upb, r, has_edge, qmax) = c.recs[0]
        assert tag == "S", c[:7]
        ctx = (c[:7], c.recs[0])
        assert L % 2 == 1 and L <= D // 4 and L <= lmax and M * L <= 65535, ctx
        assert U == ceil_div(D, L) and 1 <= r <= L and has_edge == (r != L), ctx
        assert upb * L + (r if has_edge else 0) == D, ctx
        if c.forced:
            want = c.forced | 1
            if want > D // 4:
                want = (D // 4) | 1
            if want > lmax:
                want = lmax if lmax % 2 else lmax - 1
            assert L == want, ctx
        at = 0
        for i, (tag, f) in enumerate(c.recs[1:]):
            assert tag == "T", ctx
            off, Q, cnt, R, chunk, nunits, tail, sib_blocks, edge_blocks, main_blocks, grid = f
            ctx = (c[:7], c.recs[0], f)
            assert off == at and cnt >= 1, ctx
            at += cnt
            assert Q * upb <= U32 and Q <= qmax, ctx
            assert Q * SB + nunits * chunk + tail == cnt and R == nunits * chunk + tail, ctx
            last = i == len(c.recs) - 2
            if R:
                assert last and R < SB and 1 <= chunk <= lmax and tail < chunk, ctx
                assert chunk == 1 or chunk % 2 == 1, ctx
            else:
                assert nunits == 0 and tail == 0, ctx
            assert sib_blocks == ceil_div(Q * upb, P.WG), ctx
            assert edge_blocks == (ceil_div(Q, P.WG) if has_edge else 0), ctx
            assert main_blocks == ceil_div(nunits, P.WG), ctx
            assert grid == sib_blocks + edge_blocks + main_blocks + ceil_div(tail, P.WG) and 1 <= grid <= U32, ctx
        assert at == c.count, ctx
    assert n > 1000
