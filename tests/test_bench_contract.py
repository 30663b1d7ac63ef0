"""The driver depends on bench.py's CLI and output contract: one JSON line
from rank 0 with specific fields.  Run the real script on CPU with a tiny
config and validate the line so contract regressions are caught here, not
at round end on a GPU box."""

import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_contract():
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"),
         "--rows", "6000", "--dim", "4", "--active-set", "60",
         "--steps", "2", "--warmup", "1", "--max-iter", "5",
         "--device", "cpu"],
        capture_output=True, text=True, timeout=600, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])

    # fields the driver and judge read
    assert rec["metric"].startswith("rows/sec")
    assert isinstance(rec["value"], float) and rec["value"] > 0
    assert rec["unit"] == "rows/s"
    assert rec["n_gpus"] == 1
    assert rec["steps"] == 2 and rec["warmup"] == 1
    assert rec["ms_per_step"] > 0
    assert rec["higher_is_better"] is True
    assert rec["scaling"] == "strong"
    assert rec["vs_baseline"] is None      # reference publishes no numbers
    assert rec["data"] == "synthetic"
    assert rec["dtype"] in ("fp32", "fp64")
    cfg = rec["config"]
    assert cfg["rows"] == 6000 and cfg["dim"] == 4
    assert "parallelism" in cfg and cfg["parallelism"].endswith("dp1")
    # value must be whole-job rows/sec consistent with ms_per_step
    assert abs(rec["value"] - 6000 / (rec["ms_per_step"] / 1000.0)) \
        / rec["value"] < 1e-6


def _run_dump(out_dir, *extra):
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"),
         "--rows", "2000", "--dim", "3", "--active-set", "40",
         "--steps", "1", "--warmup", "0", "--max-iter", "4",
         "--device", "cpu", "--dump-outputs", str(out_dir), *extra],
        capture_output=True, text=True, timeout=600, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_bench_dump_outputs_and_full(tmp_path):
    """--dump-outputs writes the last timed fit's model arrays; the same
    arguments give the same inputs, so a second run (here with --full, which
    must keep working) reproduces them exactly on the fp64 CPU path."""
    import numpy as np
    rec_a = _run_dump(tmp_path / "a")
    rec_b = _run_dump(tmp_path / "b", "--full")
    assert rec_a["steps"] == rec_b["steps"] == 1
    assert rec_a["metric"] == rec_b["metric"]
    shapes = {"hyperparameters": (4,),      # C + 3 ARD scales (sigma2 fixed)
              "active_set": (40, 3),
              "magic_vector": (40,),
              "magic_matrix": (40, 40)}
    total = 0
    for name, shape in shapes.items():
        a = np.load(tmp_path / "a" / (name + ".npy"))
        b = np.load(tmp_path / "b" / (name + ".npy"))
        assert a.dtype == np.float64
        assert a.shape == shape
        assert np.isfinite(a).all()
        np.testing.assert_array_equal(a, b)
        total += a.nbytes
    assert total <= 64 * 2**20
    assert sorted(os.listdir(tmp_path / "a")) == sorted(
        n + ".npy" for n in shapes)
