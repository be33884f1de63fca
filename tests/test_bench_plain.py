"""The plain bench run (`bench.py --gpus 1 --steps K --warmup W`, no --full) and --dump-outputs: the result line keeps the contract fields,
the side measurements stay out of it, and the verdict of the last timed step lands in DIR/verdict.npy."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bench():
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        import bench
    finally:
        sys.argv = argv
    return bench


def test_options_of_the_plain_and_full_runs():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "--full" in p.stdout and "--dump-outputs" in p.stdout


def test_dump_outputs_writes_float64(tmp_path):
    bench = _bench()
    bench.dump_outputs(str(tmp_path / "out"), True)
    bench.dump_outputs(str(tmp_path / "bad"), False)
    assert os.listdir(tmp_path / "out") == ["verdict.npy"]
    v = np.load(tmp_path / "out" / "verdict.npy")
    assert v.dtype == np.float64 and v.tolist() == [1.0]
    assert np.load(tmp_path / "bad" / "verdict.npy").tolist() == [0.0]


@pytest.mark.gpu
def test_plain_run_dumps_the_last_verdict(tmp_path):
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "4096", "--dump-outputs", str(out)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == "BLS sig verifications/sec (batch)" and d["unit"] == "verifications/s" and d["higher_is_better"] is True
    assert d["dtype"] == "int64" and d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert abs(d["value"] - 4096 / (d["ms_per_step"] * 1e-3)) <= 1e-9 * d["value"]
    # what --full adds is not measured in a plain run
    assert "aux" not in d and "cpu_baseline" not in d and d["value_one_caller"] is None
    assert d["roofline"]["int_mad"]["ceiling"]["measured_on_this_box"] is False
    v = np.load(out / "verdict.npy")
    assert v.dtype == np.float64 and v.tolist() == [1.0]
