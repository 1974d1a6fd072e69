"""bench.py's plain run against its `--full` run, at a small size: the plain run times its steps
and prints the headline line only (`--steps` sets the timed steps, `ms_per_step` is there, nothing
that takes a run of its own is measured) and `--dump-outputs` writes the last step's states;
`--full` adds scan_without_hll, host_ingest and valu_roofline (the CPU baseline is switched off
here: it runs for ten seconds by design)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 3_000_001  # not a multiple of 8: the last validity byte is partial


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--rows", str(ROWS)] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONUNBUFFERED="1"))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_its_states(gpu, tmp_path):
    out = _bench("--dump-outputs", str(tmp_path / "dump"))
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "rows/s" and out["higher_is_better"] is True and out["dtype"] == "int64+f64"
    assert out["ms_per_step"] > 0
    assert abs(out["value"] - ROWS / (out["ms_per_step"] * 1e-3)) <= 1e-9 * out["value"]
    assert out["roofline"]["kernel_ms"] > 0
    assert out["cpu_baseline"] is None and out["valu_roofline"] is None
    assert "scan_without_hll" not in out and "host_ingest" not in out
    assert sorted(os.listdir(tmp_path / "dump")) == ["hll_words.npy", "states.npy"]
    states = np.load(tmp_path / "dump" / "states.npy")
    words = np.load(tmp_path / "dump" / "hll_words.npy")
    assert states.dtype == np.float64 and states.shape == (65, 13)
    assert words.dtype == np.float64 and words.shape == (65, 104)
    assert (states[:, 1] == 1).all()  # every state has a value
    assert states[0, 2] == ROWS  # Size
    hll = [i for i in range(65) if words[i].any()]
    assert hll == list(range(8, 65, 8))  # the 8 ApproxCountDistinct, last of each column's 8
    # Completeness of every column: 5% NULLs drawn per row, so within 6 sigma of 95%
    sigma = (0.05 * 0.95 * ROWS) ** 0.5
    for i in range(1, 65, 8):
        assert states[i, 3] == ROWS and abs(states[i, 2] - 0.95 * ROWS) < 6 * sigma, states[i]


def test_full_run_adds_the_side_measurements(gpu):
    out = _bench("--full", "--no-cpu-baseline", "--e2e-batch-rows", "500000")
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["cpu_baseline"] is None
    assert out["scan_without_hll"]["analyzers"] == 57 and out["scan_without_hll"]["kernel_ms"] > 0
    assert out["host_ingest"]["rows_per_pass"] >= ROWS and out["host_ingest"]["pinned_rows_per_s"] > 0
    assert out["valu_roofline"]["peak"] > 0 and out["valu_roofline"]["hashes_per_launch"] == 8.0 * ROWS
