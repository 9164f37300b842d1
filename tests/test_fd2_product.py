"""Which FD kernels the product library holds, on the CPU.

nice_amd/csrc/fd2_cfg.hpp says in one place what production runs for a
(base, limb combo): SmallCfg below 1e7 numbers, BigCfg from there, BatchCfg
for the batched calls.  tests/fd2_product_dump.cpp is built host-only from
that header and prints those configurations and everything the launchers
reach from them (NoSib, NoPers, SibPers); building it evaluates every Cfg
static_assert.  The fd2_kernel / fd2_batch_kernel instantiations in
libnice_hip.so (`nm -C`) must be that set exactly: a kernel no path can
launch, or a launch path without its kernel, fails here.
"""
import os
import re
import shutil
import subprocess

import pytest

from nice_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nice_amd", "csrc")
NCOMBOS = 37  # entries of FD2_COMBOS (fd2_combos.h)


@pytest.fixture(scope="module")
def reachable(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("fd2_product") / "fd2_product_dump")
    subprocess.run([cxx, "-std=c++17", "-O0", "-I", CSRC, os.path.join(ROOT, "tests", "fd2_product_dump.cpp"),
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    sets = {"K": set(), "B": set()}
    for line in out.splitlines():
        f = line.split()
        sets[f[0]].add(tuple(map(int, f[1:])))
    return sets


def _built(kernel):
    syms = subprocess.run(["nm", "-C", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return {tuple(int(x) for x in m.split(", "))
            for m in re.findall(kernel + r"<nice::fd2::Cfg<(-?\d+(?:, -?\d+)*)>", syms)}


def test_dump_covers_every_combo(reachable):
    combos = set(re.findall(r"X\((\d+), (\d+), (\d+), (\d+)\)", open(os.path.join(CSRC, "fd2_combos.h")).read()))
    combos = {tuple(map(int, c)) for c in combos}
    assert len(combos) == NCOMBOS
    assert {c[:4] for c in reachable["B"]} == combos and len(reachable["B"]) == NCOMBOS
    assert {c[:4] for c in reachable["K"]} == combos
    # Cfg<BASE, ND, NE, NE2, PROBE, WG, VD, LG, PERS, SIB>: per combo at least a
    # small-field and a big-field kernel, all distinct from the batch kernel's type
    assert all(len(c) == 10 and c[4] == 0 for c in reachable["K"] | reachable["B"])
    assert len(reachable["K"]) >= 2 * NCOMBOS - 8  # b59..64 (8 combos) run one kernel at every size
    assert not reachable["K"] & reachable["B"]


def test_library_holds_exactly_the_reachable_field_kernels(reachable):
    built = _built(r"\bfd2_kernel")
    assert built, "no fd2 kernels found"
    assert built - reachable["K"] == set(), "kernels no production path launches"
    assert reachable["K"] - built == set(), "production paths without a kernel"


def test_library_holds_exactly_the_batch_kernels(reachable):
    assert _built(r"\bfd2_batch_kernel") == reachable["B"]
