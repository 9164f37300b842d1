"""The persistent sibling grid's launch plans (nice_amd/csrc/fd2_plan.hpp
plan_sib_pers and plan_sib_launch), on the CPU.

tests/fd2_sib_pers_plan_dump.cpp is built host-only and prints, for the b40
pipelined-walk configuration over device shapes, field sizes, lane strides and
the test hook's modes, every launch of every segment -- and walks each launch's
grid the way the device code does (workgroup g takes the batches g + G k; the
unit of a lane from the batch index, in 32-bit words), counting how often each
sibling and edge unit is taken.  Asserted here is what fd2_kernel.hpp assumes
of such a launch.  The same program is run once more as an AddressSanitizer +
UndefinedBehaviorSanitizer build (host code with its own main).
"""
import os
import shutil
import subprocess
from collections import namedtuple

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nice_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "fd2_sib_pers_plan_dump.cpp")
U32 = 0xFFFFFFFF
M, D, WG = 3, 40 ** 4, 512
SB, NW = M * D, WG // 64
PERS_MIN_TENTHS = 40  # PlanKnobs::sib_pers_min

Case = namedtuple("Case", "cus per_cu count L mode max_wg overlapped recs")
T = namedtuple("T", "off Q cnt R sib_units edge_units sib_blocks edge_blocks main_blocks grid batches wave_cap "
                    "chunk nunits tail walked missed twice max_per_wg")


def _cxx():
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    return cxx


def _parse(out):
    cases = []
    for line in out.splitlines():
        f = line.split()
        if f[0] == "K":
            cases.append(Case(*map(int, f[1:]), []))
        else:
            cases[-1].recs.append((f[0], tuple(map(int, f[1:]))))
    return cases


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fd2_sib_pers") / "dump")
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-I", CSRC, SRC, "-o", exe], check=True)
    # odd lane strides 105, 113, ... 209 and 45, 61, 125, 143, 159, 255
    return _parse(subprocess.run([exe, "8"], capture_output=True, text=True, check=True).stdout)


def launches(c):
    return [T(*r) for tag, r in c.recs if tag == "T"]


def shape(c):
    return next(r for tag, r in c.recs if tag == "S")


def test_sweep_is_complete(cases):
    assert len(cases) == 4 * 2 * 7 * (6 + 14) * 7
    assert {c.cus for c in cases} == {8, 64, 256, 304} and {c.per_cu for c in cases} == {1, 2}
    assert not any(tag in "NX" for c in cases for tag, _ in c.recs)  # every field has >= 4 super-blocks, L forced
    walked = sum(1 for c in cases for t in launches(c) if t.walked)
    assert walked > 5000
    # the MI355X's bench field at the production stride: one launch, one round of resident workgroups
    c = next(c for c in cases if (c.cus, c.per_cu, c.count, c.L, c.mode, c.overlapped) == (256, 2, 10 ** 9, 143, 0, 1))
    (t,) = launches(c)
    assert shape(c)[:3] == (1, 512, 152) and (t.sib_blocks, t.batches, t.walked) == (512, 36367, 1)


def test_modes(cases):
    for c in cases:
        pers, grid, cap, upb, has_edge, r = shape(c)
        resident = c.cus * c.per_cu
        q = c.count // SB
        nb = -(-q * upb // 64) + (-(-q // 64) if has_edge else 0)
        if c.mode == 2:
            assert not pers, c[:7]
        elif c.mode == 1:
            assert pers and grid == (min(resident, c.max_wg) if c.max_wg else resident), c[:7]
        else:
            # production: pipelined fields of enough batches per resident wave; a lone field keeps rounds
            assert pers == (c.overlapped == 1 and 10 * nb >= PERS_MIN_TENTHS * resident * NW), c[:7]
            assert not pers or grid == resident
        if pers:
            # the lanes' u16 window counters: M L numbers per unit, wave_cap units
            assert cap >= 1 and cap * M * c.L <= 65535 < (cap + 1) * M * c.L, c[:7]
        assert has_edge == (D % c.L != 0) and upb == D // c.L and (r == D % c.L or not has_edge)


def test_every_unit_once(cases):
    """Each sibling unit and each edge unit belongs to exactly one (workgroup,
    batch, lane); a workgroup's batches are within its waves' caps."""
    for c in cases:
        pers, grid, cap, upb, has_edge, _ = shape(c)
        for t in launches(c):
            if not pers:
                assert (t.batches, t.wave_cap, t.walked) == (0, 0, 0)
                continue
            assert t.edge_blocks == 0 and t.wave_cap == cap
            assert t.sib_units == t.Q * upb and t.edge_units == (t.Q if has_edge else 0)
            assert t.batches == -(-t.sib_units // 64) + -(-t.edge_units // 64)
            # unit and batch counts (64 b + lane on the device) in 32 bits
            assert t.sib_units <= U32 - 63 and t.batches * 64 <= U32 and t.grid <= U32
            # at most one round of resident workgroups (the hook's cap below it)
            assert t.sib_blocks <= grid <= c.cus * c.per_cu
            assert t.sib_blocks == min(grid, -(-t.batches // NW))
            if t.Q:
                assert t.sib_blocks >= 1 and -(-t.batches // t.sib_blocks) <= NW * cap, (c[:7], t)
            if t.walked:
                assert (t.missed, t.twice) == (0, 0), (c[:7], t)
                assert t.max_per_wg == -(-t.batches // t.sib_blocks) <= NW * cap


def test_launches_tile_the_segment(cases):
    for c in cases:
        ts = launches(c)
        off = 0
        for i, t in enumerate(ts):
            assert t.off == off and t.cnt > 0 and t.cnt == t.Q * SB + t.R
            assert (t.R == 0 and t.nunits == 0 and t.tail == 0) or i == len(ts) - 1
            assert t.nunits * t.chunk + t.tail == t.R and t.tail < max(t.chunk, 1) + (t.R == 0)
            assert t.main_blocks == -(-t.nunits // WG)
            assert t.grid == t.sib_blocks + t.edge_blocks + t.main_blocks + -(-t.tail // WG)
            off += t.cnt
        assert off == c.count
        # the remainder's regular parts are the rounds plan's
        (o,) = [r for tag, r in c.recs if tag == "O"]
        last = ts[-1]
        assert (last.R, last.chunk, last.nunits, last.tail, last.main_blocks) == o, c[:7]
        assert o[0] == c.count % SB


def test_cap_overflow_splits(cases):
    """8 super-blocks at L = 143 on one workgroup: 2 239 batches against
    8 waves x 152, so the segment splits (tests/test_gpu_sib_persistent.py)."""
    c = next(c for c in cases if (c.cus, c.per_cu, c.count, c.L, c.mode, c.max_wg) == (256, 2, 8 * SB + 54321, 143, 1, 1))
    ts = launches(c)
    assert len(ts) >= 2 and sum(t.batches for t in ts) >= 2239 and all(t.batches <= 8 * 152 for t in ts)


def test_sanitized_build_runs_clean(tmp_path):
    """The dump program under ASan + UBSan, on a coarser stride sweep."""
    exe = str(tmp_path / "dump_san")
    r = subprocess.run([_cxx(), "-std=c++17", "-O1", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe, "104"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(_parse(r.stdout)) == 4 * 2 * 7 * (6 + 2) * 7
