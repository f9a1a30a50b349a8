"""CPU: bench.py's timed steps and --dump-outputs — how --steps splits into sweeps, which rollouts the dump writes (all, or a fixed seeded sample
that keeps the files under the cap) and what the files hold."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_sample_is_fixed_and_keeps_the_headline_dump_under_the_cap():
    B, dofs, small = 256, 30000, 8 * 257          # the headline workload: 256 rollouts of 10 000 vertices, one friction group
    rows = bench.dump_sample(B, dofs, small)
    assert np.array_equal(rows, bench.dump_sample(B, dofs, small))
    assert 0 < len(rows) < B and np.array_equal(rows, np.unique(rows)) and rows.max() < B
    assert len(rows) * 4 * 8 * dofs + small + 1024 <= bench.DUMP_BYTES
    assert np.array_equal(bench.dump_sample(8, dofs, 8 * 9), np.arange(8))          # small batches are written whole
    with pytest.raises(SystemExit):
        bench.dump_sample(1, bench.DUMP_BYTES // 8, 16)


def test_dump_writes_float64_arrays_of_the_sampled_rollouts(tmp_path):
    rng = np.random.default_rng(1)
    B, dofs = 256, 30000
    x, v, dx, dv = (rng.standard_normal((B, dofs)) for _ in range(4))
    dmu = rng.standard_normal((B, 1))
    rows = bench.dump_sample(B, dofs, 8 * (B + 1))
    bench.dump_outputs(str(tmp_path / "out"), rows, x, v, dx, dv, dmu, dmu.sum(axis=0).astype(np.float32))
    files = sorted(os.listdir(tmp_path / "out"))
    assert files == sorted(["x.npy", "v.npy", "dL_dx.npy", "dL_dv.npy", "dL_dmu.npy", "dL_dmu_total.npy"])
    assert sum(os.path.getsize(tmp_path / "out" / f) for f in files) <= bench.DUMP_BYTES
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in files}
    assert all(a.dtype == np.float64 for a in got.values())
    for name, full in (("x", x), ("v", v), ("dL_dx", dx), ("dL_dv", dv)):
        assert np.array_equal(got[name], full[rows]), name
    assert np.array_equal(got["dL_dmu"], dmu) and got["dL_dmu_total"].shape == (1,)


def test_timed_steps_are_sweeps_of_at_most_one_window_ending_on_a_full_one():
    T = bench.TIMED_WINDOW
    for K in (1, 3, T - 1, T, T + 1, 2 * T, 5 * T + 7, 1000):
        w = bench.timed_windows(K)
        assert sum(w) == K and all(0 < n <= T for n in w) and w[-1] == min(K, T), (K, w)
        slots = bench.timed_slots(5, K)
        assert len(slots) == K and min(slots) == 6 and max(slots) == 5 + min(K, T), K
