"""bench.py on the GPU: a plain run prints the line from the timed steps alone and, with
``--dump-outputs DIR``, writes the last step's output arrays as DIR/<name>.npy -- the arrays a caller of
BatchSolver.launch on the same shard receives (solves are bitwise repeatable,
test_repeated_solves_are_bitwise_identical)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER = 128  # one segment of C4 (M = 128 states per segment): the smallest shard bench.py accepts


def test_plain_run_dumps_what_the_timed_path_computed(tmp_path):
    from mpcracing import workload as wl
    from mpcracing.batch import solver_for_config
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    d = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--per-gpu", str(PER), "--dump-outputs", d], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["unit"] == "solves/s" and line["higher_is_better"] is True
    assert line["dtype"] == "fp32" and line["ms_per_step"] > 0
    assert abs(line["value"] - PER / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    # what --full measures is not part of a plain run
    for k in ("cpu_baseline", "agent_call", "pipelined", "shard_spread"):
        assert k not in line
    assert line["p50_latency_b1_ms"] is None and line["roofline"]["copy_gbs"] is None

    ref = solver_for_config("C4", PER, dispatch_order=1).solve(wl.make_batch("C4", per_gpu=PER))
    assert sorted(os.listdir(d)) == sorted(f"{k}.npy" for k in ref)
    total = 0
    for k, v in ref.items():
        a = np.load(os.path.join(d, f"{k}.npy"))
        total += a.nbytes
        assert a.dtype == np.float64 and a.shape == tuple(v.shape)
        assert np.array_equal(a, v.cpu().numpy().astype(np.float64), equal_nan=True), k
    assert total <= 64 << 20
    st = np.load(os.path.join(d, "status.npy")).astype(int)
    assert np.bincount(st, minlength=5)[:5].tolist() == list(line["status_hist"].values())
