"""bench.py's plain run and --dump-outputs: a plain run times the steps and prints the line without the oracle check or the profiles of --full, and
the outputs it dumps for its last timed step are those the --full run of the same arguments checks against the oracle, bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "HNET_BENCH_SHARED_GPU")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "8", *argv]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_dumps_the_outputs_the_full_run_checks(tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path / "plain"))
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["ms_per_step"] > 0 and plain["value"] > 0
    for key in ("metric", "unit", "higher_is_better", "dtype"):
        assert key in plain
    assert "verify" not in plain and "roofline" not in plain and "cpu_baseline" not in plain
    full = _bench("--full", "--no-extras", "--no-cpu-baseline", "--no-latency", "--dump-outputs", str(tmp_path / "full"))
    assert full["verify"]["passed"] and full["verify"]["step"] == 3
    for name, shape in (("mean", (8, 8)), ("cov", (8, 8, 8))):
        a, b = np.load(tmp_path / "plain" / f"{name}.npy"), np.load(tmp_path / "full" / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == shape and np.isfinite(a).all()
        np.testing.assert_array_equal(a, b)
