"""`bench.py` without --full: one JSON line with the contract fields and nothing measured beyond the timed steps, and
--dump-outputs writing what the last timed training step computed (loss, updated weights and buffers, gradients)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_dumps_last_step(tmp_path):
    out_dir = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "4",
           "--width", "512", "--embed-dim", "256", "--depth", "2", "--heads", "4", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-1500:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["roofline"] is None and not {"strong", "parity_path", "cpu_baseline"} & set(d)

    files = sorted(os.listdir(out_dir))
    assert files == ["buffers.npy", "grads.npy", "loss.npy", "params.npy"], files
    arr = {f[:-4]: np.load(out_dir / f) for f in files}
    assert all(a.dtype == np.float32 for a in arr.values())
    assert sum(a.nbytes for a in arr.values()) <= 64 << 20
    assert arr["params"].shape == arr["grads"].shape and arr["params"].ndim == 1
    assert all(np.isfinite(a).all() for a in arr.values())
    assert float(np.abs(arr["grads"]).max()) > 0
    assert abs(float(arr["loss"]) - d["config"]["loss"]) <= 1e-6 * abs(d["config"]["loss"])
