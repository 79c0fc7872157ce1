"""GPU: bench.py's plain run and --dump-outputs.  The plain line carries the headline figures only (what --full adds is
absent); the dumped arrays are the last timed launch's outputs for the seeded inputs bench.synth makes, equal from run to
run and to the fp64 oracle on sampled batches."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import rel_fro
from oracle import ge2e_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N, M, D = 256, 64, 10, 256   # cfg2's shape at fewer batches per launch: dE (168 MB) is still sampled

pytestmark = pytest.mark.gpu


def run_bench(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_run_dumps_the_timed_launchs_outputs(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import bench
    runs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        j = run_bench("--steps", "3", "--warmup", "1", "--batches", str(B), "--dump-outputs", str(d))
        assert j["steps"] == 3 and j["ms_per_step"] > 0 and j["value"] > 0 and j["config"]["batches_per_launch"] == B
        assert not {"verify", "cpu_baseline", "forward_only", "latency_b1_us", "exact_f32"} & set(j), sorted(j)
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 << 20
        runs.append({f[:-4]: np.load(d / f) for f in os.listdir(d)})
    a, b = runs
    assert sorted(a) == ["batches", "dE", "db", "dw", "loss"]
    for name in a:
        assert a[name].dtype in (np.float32, np.float64) and np.array_equal(a[name], b[name]), name
    idx = a["batches"].astype(np.int64)
    assert 1 <= len(idx) < B and np.all(np.diff(idx) > 0) and idx[-1] < B
    assert a["loss"].shape == a["dw"].shape == a["db"].shape == (B,) and a["dE"].shape == (len(idx), N, M, D)
    E = bench.synth(B, N, M, D, 1234, "cuda:0")   # rank 0's inputs, as the child made them
    for j, i in list(enumerate(idx))[:3]:
        ref = orc.closed_form(E[i].cpu().numpy(), 10.0, -5.0)
        assert abs(float(a["loss"][i]) - ref["loss"]) <= 1e-4 * abs(ref["loss"])
        assert rel_fro(a["dE"][j], ref["dE"]) <= 1e-4
        assert abs(float(a["dw"][i]) - ref["dw"]) <= 1e-4 * abs(ref["dw"]) + 1e-5
        assert abs(float(a["db"][i]) - ref["db"]) <= 1e-4
