"""GPU: bench.py's plain run and --dump-outputs -- two runs with the same arguments write the same outputs (up to the rounding of
the kernels' unordered fp32 atomics), so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bench(out_dir):
    env = {k: v for k, v in os.environ.items() if not k.startswith(("BL_", "BUGLAB_"))}  # (other tests switch modes through the environment)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "12", "--warmup", "3", "--graphs", "8",
                        "--nodes", "500", "--messages", "2500", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("{")][-1])


def test_two_plain_runs_dump_the_same_outputs(tmp_path):
    lines = [_bench(tmp_path / d) for d in ("a", "b")]
    for line in lines:
        assert line["steps"] == 12 and line["warmup"] == 3 and line["ms_per_step"] > 0 and line["full"] is False
        assert line["roofline"] is None and line["also"] is None and line["cpu_baseline"] is None
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert "loss.npy" in names and any(n.startswith("grad.") for n in names) and any(n.startswith("param.") for n in names)
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and a.shape == b.shape and np.isfinite(a).all(), n
        scale = float(np.abs(a).max()) if a.size else 0.0
        assert float(np.abs(a.astype(np.float64) - b).max(initial=0.0)) <= 1e-5 * scale + 1e-12, n
