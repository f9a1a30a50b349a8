"""BatchedSim.check_episode reports unconverged adjoint solves (diffcloth_amd/functional.py). A diverged solve leaves a non-finite
relative residual (last_udiff = NaN / inf); it must be reported as the worst one — a warning, or RuntimeError when strict — never turn
into an error of the report itself. CPU only: the engine is a stub that serves the two calls check_episode makes."""
import re
import warnings

import numpy as np
import pytest

from diffcloth_amd.functional import BatchedSim


class StubEngine:
    """Statistics of a recorded episode: bwd[slot] = (converged [B], last_udiff [B])."""

    def __init__(self, bwd):
        self.bwd = bwd
        self.B = len(next(iter(bwd.values()))[0])
        self.tape = max(bwd)
        self.synced = 0

    def sync(self):
        self.synced += 1

    def get_stats(self, slot):
        conv, res = self.bwd[slot]
        fwd = {"converged": np.ones(self.B, np.int64)}
        bwd = {"converged": np.asarray(conv, np.int64), "last_udiff": np.asarray(res, np.float32)}
        return fwd, bwd


def sim_after_backward(bwd, strict):
    e = StubEngine(bwd)
    s = BatchedSim(e, step_num=e.tape, strict=strict)
    s.step_idx = e.tape
    s._bwd_slots = set(bwd)
    return s


NAN = float("nan")
EPISODES = {
    # NaN residuals only, on the unconverged rollouts of one step
    "all_nan": ({1: ([1, 0, 1], [1e-7, NAN, 2e-7]), 2: ([0, 0, 1], [NAN, NAN, 1e-7])}, 3, (1, 1)),
    # NaN after a finite unconverged residual at a later step: the NaN one is the worst
    "nan_after_finite": ({1: ([1, 0, 1], [1e-7, 3e-3, 1e-7]), 2: ([1, 1, 0], [1e-7, 1e-7, NAN])}, 2, (2, 2)),
    # NaN first, a larger finite residual later: still the NaN one
    "nan_before_finite": ({1: ([0, 1, 1], [NAN, 1e-7, 1e-7]), 2: ([1, 0, 1], [1e-7, 5e2, 1e-7])}, 2, (1, 0)),
    # infinity is as bad as NaN; mixed with a finite one in the same step
    "inf_and_finite": ({1: ([0, 0, 1], [4e-2, float("inf"), 1e-7])}, 2, (1, 1)),
    # finite residuals only: the largest is reported
    "finite": ({1: ([0, 1, 0], [2e-3, 1e-7, 9e-3]), 2: ([0, 1, 1], [1e-4, 1e-7, 1e-7])}, 3, (1, 2)),
}


def expected_worst(bwd, at):
    conv, res = bwd[at[0]]
    return float(np.float32(res[at[1]]))


@pytest.mark.parametrize("name", sorted(EPISODES))
def test_strict_raises_with_the_worst_rollout(name):
    bwd, nbad, at = EPISODES[name]
    s = sim_after_backward(bwd, strict=True)
    with pytest.raises(RuntimeError) as ei:
        s.check_episode()
    msg = str(ei.value)
    assert f"{nbad} adjoint solve(s) of this episode did not converge" in msg
    first_slot = min(k for k in bwd if 0 in bwd[k][0])
    first_bad = bwd[first_slot][0].index(0)
    assert f"first: step {first_slot}, rollout {first_bad}" in msg, msg
    assert f"at step {at[0]}, rollout {at[1]}" in msg, msg
    m = re.search(r"worst relative residual (\S+) at", msg)
    worst = float(m.group(1))
    want = expected_worst(bwd, at)
    if np.isfinite(want):
        assert worst == pytest.approx(want, rel=1e-2)
    else:
        assert not np.isfinite(worst)
    assert s.unconverged == nbad
    assert s.engine.synced == 1


@pytest.mark.parametrize("name", sorted(EPISODES))
def test_lenient_warns(name):
    bwd, nbad, at = EPISODES[name]
    s = sim_after_backward(bwd, strict=False)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        s.check_episode()
    msgs = [str(w.message) for w in rec if issubclass(w.category, RuntimeWarning)]
    assert len(msgs) == 1, [str(w.message) for w in rec]
    assert f"at step {at[0]}, rollout {at[1]}" in msgs[0]
    assert s.unconverged == nbad


def test_converged_episode_is_silent():
    s = sim_after_backward({1: ([1, 2, 1], [1e-7, 3e-5, 1e-7]), 2: ([1, 1, 1], [1e-7, 1e-7, 1e-7])}, strict=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        s.check_episode()
    assert s.unconverged == 0


def test_slots_without_backward_are_not_judged():
    # converged == 0 of a slot the backward sweep has not reached is the forward's business, not this report's
    s = sim_after_backward({1: ([1, 1], [1e-7, 1e-7]), 2: ([0, 0], [NAN, NAN])}, strict=True)
    s._bwd_slots = {1}
    s.check_episode()
    assert s.unconverged == 0
