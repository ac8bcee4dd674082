"""`python bench.py --steps K --dump-outputs DIR` on the GPU: exactly K launches are timed, and C of the last one is written.  Two runs whose last steps
land on the same input set (the headline rotates over 12 sets: steps 7 and 19 both end on set 6) dump the same array, bit for bit -- the inputs depend
on the arguments only.  A plain run (no --full) measures the headline and nothing else."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(steps, out, full=True):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2"]
    if full:                                  # the oracle check, without the secondary legs
        cmd += ["--full", "--no-sweep", "--no-l3", "--no-cpu-baseline"]
    cmd += ["--detail", "", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][-1])


@pytest.mark.gpu
def test_bench_times_exactly_steps_and_dumps_the_last_c(tmp_path):
    a = _bench(7, tmp_path / "a")
    b = _bench(19, tmp_path / "b")
    for line, steps in ((a, 7), (b, 19)):
        assert line["steps"] == steps and line["steps_timed"] == steps and line["verified"] is True
        assert line["ms_per_step"] > 0
    ca, cb = np.load(tmp_path / "a" / "C.npy"), np.load(tmp_path / "b" / "C.npy")
    assert ca.dtype == np.float32 and ca.shape == (4096, 32, 32)
    assert np.isfinite(ca).all() and np.abs(ca).max() > 0
    assert np.array_equal(ca, cb)


@pytest.mark.gpu
def test_plain_run_measures_the_headline_only(tmp_path):
    """Without --full: set-up, warm-up, the timed steps, the dump and the line -- no oracle check, no secondary leg, no CPU baseline."""
    line = _bench(5, tmp_path / "plain", full=False)
    assert line["steps"] == 5 and line["steps_timed"] == 5 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["verified"] is None
    for key in ("cpu_baseline", "sweep", "reuse", "ragged", "configs", "round4", "tpp", "pipelined", "l3_resident_us", "without_streaming_hint_us",
                "mfma_power_roof_TF", "single_call_us", "sharded_c_abi"):
        assert key not in line, key
    c = np.load(tmp_path / "plain" / "C.npy")
    assert c.shape == (4096, 32, 32) and np.abs(c).max() > 0
