"""bench.py --steps / --dump-outputs end to end at a small size: the result line counts the timed steps it was given, `ms_per_step` is
the time of one of them, and the dumped arrays are what the timed sweep returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["x", "v", "dL_dx", "dL_dv", "dL_dmu", "dL_dmu_total"]


def run_bench(steps, out):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2", "--total-batch", "8", "--grid", "40",
           "--fold-rows", "3", "--fold-gap", "0.05", "--cpu-steps", "0", "--tshirt", "0", "--secondary", "none", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), {f[:-4]: np.load(out / f) for f in os.listdir(out)}


def test_bench_steps_and_dumped_outputs(tmp_path):
    out = tmp_path / "dump"
    d, got = run_bench(3, out)
    assert d["steps"] == 3 and d["warmup"] == 2 and d["ms_per_step"] > 0
    assert abs(d["value"] - 8 * 3 / (d["ms_per_step"] * 3 * 1e-3)) <= 1e-6 * d["value"]
    assert sorted(got) == sorted(NAMES)
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64_000_000
    for name in ("x", "v", "dL_dx", "dL_dv"):
        assert got[name].shape == (8, 3 * 40 * 40) and got[name].dtype == np.float64 and np.isfinite(got[name]).all(), name
    assert got["dL_dmu"].shape == (8, 1) and got["dL_dmu_total"].shape == (1,)
    assert np.isclose(got["dL_dmu_total"][0], d["config"]["dL_dmu_sum_over_job"])
    assert np.isclose(got["dL_dmu"].sum(), got["dL_dmu_total"][0], rtol=1e-5, atol=1e-12)
    assert np.abs(got["dL_dx"]).max() > 0


def test_more_steps_than_one_window_repeat_the_window(tmp_path):
    """--steps beyond TIMED_WINDOW: that many steps are timed, as sweeps from the same warmed-up state, and the caller receives what one
    full window returns."""
    sys.path.insert(0, ROOT)
    import bench
    T = bench.TIMED_WINDOW
    d1, one = run_bench(T, tmp_path / "one")
    d2, more = run_bench(2 * T + 5, tmp_path / "more")
    assert d2["steps"] == 2 * T + 5 and d2["ms_per_step"] > 0
    for name in NAMES:
        np.testing.assert_array_equal(more[name], one[name], err_msg=name)
    assert d2["config"]["mean_pd_iters_per_step"] > 0
