"""-m gpu: bench.py as every change is measured with.  A plain run times --steps epochs of the workload and nothing else;
--dump-outputs writes what the last timed epoch computed (the model, the epoch's sums) as float64 .npy files; the same
arguments give the same bits (fixed-order sums, seeded inputs), and --full -- the secondary legs after the timed steps --
dumps the same model.  The tiny workload: 5e4 x 5e3, 16 nnz/row, k = 8, SGD, logistic loss."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("P", "w", "intercept", "loss", "viol")


def bench(out_dir, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "tiny", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir), *extra], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    return line, {name: np.load(os.path.join(str(out_dir), name + ".npy")) for name in NAMES}


def test_plain_run_times_the_steps_and_dumps_the_model(tmp_path):
    line, got = bench(tmp_path / "a")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 / 50_000 - 1) < 1e-3  # value = samples of one step / its time
    for key in ("roofline", "cpu_baseline", "predict", "exact_order", "time_to_target", "extra", "value_shuffled"):
        assert line[key] is None, key  # (--full's legs)
    assert got["P"].shape == (1, 8, 5000) and got["w"].shape == (5000,)
    assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in got.values())
    assert np.abs(got["w"]).max() > 0 and got["loss"][0] > 0
    assert sum(os.path.getsize(str(p)) for p in (tmp_path / "a").iterdir()) <= 64 << 20

    _, again = bench(tmp_path / "b")
    for name in NAMES:
        assert np.array_equal(got[name].view(np.uint64), again[name].view(np.uint64)), name

    full, dumped = bench(tmp_path / "c", "--full", "--no-cpu-baseline")
    assert full["roofline"]["frac"] > 0 and full["predict"]["value"] > 0 and full["exact_order"]["value"] > 0
    for name in NAMES:
        assert np.array_equal(got[name].view(np.uint64), dumped[name].view(np.uint64)), name
