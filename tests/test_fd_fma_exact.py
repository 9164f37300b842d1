"""The FD step's limb arithmetic on the f32 FMA pipe (Cfg::FMA, fma_bits in
nice_amd/csrc/fd2_kernel.hpp) is exact, on the CPU.

A u32 bit pattern x <= 2^24 read as an f32 is x 2^-149, so an FMA of two such
patterns with a true float constant returns the pattern of the integer
a K + c -- while every operand and result is an integer in [0, 2^24] and no
integer that wrapped below zero reaches an FMA.  tests/fd_fma_dump.cpp, built
host-only with plain -O2 (no fast-math) from fd2_cfg.hpp, evaluates every FMA
form of the step with fmaf on bit patterns for each of the 24 FD bases' limb
layouts, the flag on: exhaustively over t = ES u, u <= 5B + 4, with every
carry; over every S-limb sum; and whole C limbs in the step's order, over
every stored S limb, with N3's offset (wrapped) limbs.  Its compile is
the check of Cfg's static_asserts; its control column shows that the integer
form's order (the offset term first) does break an FMA, so the comparison can
fail.
"""
import os
import shutil
import subprocess
from collections import namedtuple

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nice_amd", "csrc")
LIM = 1 << 24

Row = namedtuple("Row", "base nd ne ne2 es bad_t1 bad_red bad_s bad_top bad_chain "
                        "max_t1 max_t max_ts lim_t1 lim_t lim_ts bad_wrong")


def _combos():
    import re
    text = open(os.path.join(CSRC, "fd2_combos.h")).read()
    body = text[text.index("#define FD2_COMBOS(X)"):]
    body = body[:body.index("\n\n")]
    return [tuple(int(v) for v in m) for m in re.findall(r"X\((\d+), (\d+), (\d+), (\d+)\)", body)]


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("fd_fma") / "fd_fma_dump")
    subprocess.run([cxx, "-std=c++17", "-O2", "-I", CSRC, os.path.join(ROOT, "tests", "fd_fma_dump.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return [Row(*(int(v) for v in ln.split()[1:])) for ln in out.splitlines() if ln.startswith("F ")]


def test_every_layout_of_every_fd_base(rows):
    combos = _combos()
    assert len({c[0] for c in combos}) == 24
    assert [(r.base, r.nd, r.ne, r.ne2) for r in rows] == combos


def test_every_form_equals_its_integer_expression(rows):
    bad = [(r.base, r.nd, r.ne, r.ne2, r[5:10]) for r in rows if any(r[5:10])]
    assert not bad, bad


def test_operands_stay_within_the_static_bounds(rows):
    for r in rows:
        seen = (r.max_t1, r.max_t, r.max_ts)
        lims = (r.lim_t1, r.lim_t, r.lim_ts)
        assert all(0 < s <= l <= LIM for s, l in zip(seen, lims)), r
        # the bounds are tight: the exhaustive loops reach them to within one
        # stored step
        assert all(l - s <= r.es for s, l in zip(seen, lims)), r


def test_the_control_order_does_fail(rows):
    """Adding N3's offset limb to C before the carry's FMA feeds
    it a wrapped integer: the dump must see that go wrong, for every layout
    with an offset at all (b64: B = 2^12, the bias 2^T - B is zero)."""
    assert all((r.bad_wrong > 0) == (r.base != 64) for r in rows), [(r.base, r.bad_wrong) for r in rows]
