"""bench.py's plain run and --dump-outputs: dump_outputs() writes the last
field's results as float64 arrays (CPU); a plain run's line carries the
headline figures and none of what --full adds, and its dumped arrays equal the
committed oracle fixture of the field (gpu)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

FULL_ONLY = ("roofline", "cpu_baseline", "fixture_check", "verified_against_fixture",
             "detailed_ms_per_step", "niceonly_ms_per_step", "detailed_numbers_per_sec",
             "niceonly_numbers_per_sec", "t1_ms_per_step", "strong_efficiency")


def test_dump_outputs_arrays(tmp_path):
    import nice_amd as N
    from nice_amd.api import NiceonlyStats
    s = 2 ** 70  # numbers are u128: stored as offsets from the field's start
    field = N.FieldSize(s, s + 1000)
    det = N.FieldResults(distribution=[N.UniquesDistributionSimple(i, 10 * i) for i in range(1, 11)],
                         nice_numbers=[N.NiceNumberSimple(s + 5, 9), N.NiceNumberSimple(s + 999, 10)])
    nic = N.FieldResults(distribution=[], nice_numbers=[N.NiceNumberSimple(s + 999, 10)])
    st = NiceonlyStats(3, 700, 41, 2, 0.0, 0.0)
    out = tmp_path / "a" / "b"  # created when missing
    bench.dump_outputs(str(out), field, (field, det, nic, st))
    got = {p.name: np.load(p) for p in out.iterdir()}
    assert sorted(got) == ["detailed_distribution.npy", "detailed_near_misses.npy",
                           "niceonly_nice_numbers.npy", "niceonly_stats.npy"]
    assert all(a.dtype == np.float64 and a.size > 0 for a in got.values())
    assert got["detailed_distribution.npy"].tolist() == [10.0 * i for i in range(1, 11)]
    assert got["detailed_near_misses.npy"].tolist() == [2, 5, 9, 999, 10]
    assert got["niceonly_nice_numbers.npy"].tolist() == [1, 999]
    assert got["niceonly_stats.npy"].tolist() == [3, 700, 41]
    # a mode that did not run writes no file; empty lists still write their length
    only = tmp_path / "det"
    bench.dump_outputs(str(only), field, (field, N.FieldResults(det.distribution, []), None, None))
    assert sorted(p.name for p in only.iterdir()) == ["detailed_distribution.npy", "detailed_near_misses.npy"]
    assert np.load(only / "detailed_near_misses.npy").tolist() == [0]


def test_full_and_dump_outputs_are_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and (a.steps, a.warmup) == (7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                          "--warmup", "1", "--dump-outputs", str(tmp_path)],
                         capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    line = json.loads(lines[0])
    assert line["metric"] == "numbers checked/sec per node, detailed+niceonly, 1e9 @ base 40 field"
    assert line["unit"] == "numbers/s" and line["higher_is_better"] is True and line["dtype"] == "u32"
    assert line["steps"] == 3 and line["fields_checked"] == 3
    assert line["value"] == pytest.approx(1e9 / (line["ms_per_step"] / 1e3), rel=1e-9)
    assert not [k for k in FULL_ONLY if k in line]
    with open(os.path.join(ROOT, "tests", "golden", "oracle_fields.json")) as fh:
        fx = json.load(fh)
    det = next(c for c in fx["detailed"] if c["name"] == "b40_extra_large_1e9")
    nic = next(c for c in fx["niceonly"] if c["name"] == "b40_extra_large_1e9")
    s = int(det["start"])
    got = {n: np.load(tmp_path / n) for n in os.listdir(tmp_path)}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["detailed_distribution.npy"].tolist() == [c for _, c in det["distribution"]]
    assert got["detailed_near_misses.npy"].tolist() == (
        [len(det["near_misses"])] + [v for n, u in det["near_misses"] for v in (int(n) - s, u)])
    assert got["niceonly_nice_numbers.npy"].tolist() == (
        [len(nic["nice_numbers"])] + [int(n) - s for n in nic["nice_numbers"]])
    assert got["niceonly_stats.npy"][2] == nic["candidates"]
