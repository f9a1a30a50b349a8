"""self_detect_rollout (csrc/dc_selflib.h) against the fp64 oracle off the clean fold: the cases of tests/selfdetect_cases.py — random clouds
with hubs and loops, contacts that exist only at the end of the step, pairs the reference's sweep window never visits, the 1.0 cut, y as
the longest axis, the 512-cell cap, the 512- and 1024-thread instances, a sphere seeding the layering frontier, folded stacks hundreds of
layers deep — and batches whose rollouts hold different contact counts. tests/test_selfdetect_companion.py asserts on the CPU that every
decision of these inputs keeps a margin of ~100 fp32 ulps and that each targeted branch is live, so the pair set, the layer of every pair
and the primitive contacts must EQUAL the oracle's. The clouds run one PD iteration (only the detection is under test; the step may
report converged = 0)."""
import numpy as np
import pytest

import selfdetect_cases as sc

pytestmark = pytest.mark.gpu
NORMAL_TOL = 5e-6


def compare_rollout(e, st, slot, b, name):
    """detection and layering of rollout b at `slot` against the oracle's run of case `name`"""
    case, o, ref, layered, contacts = sc.reference(name)
    got = e.get_self_contacts(slot, rollout=b)
    have = sorted((int(l), int(a), int(c)) for l, (a, c) in zip(got["layer"], got["pairs"]))
    assert st["self_overflow"][b] == 0
    assert st["self_contacts"][b] == ref["nself"] == got["count"]
    assert got["layers"] == ref["nlayers"]
    assert have == layered                                   # the same pairs and the same layer for every pair
    assert np.all(np.diff(got["layer"]) >= 0)                # stored in layer order
    for l in range(got["layers"]):
        ids = got["pairs"][got["layer"] == l].reshape(-1)
        assert len(ids) == len(set(ids.tolist()))            # no vertex twice in a layer
    nmap = {(int(a), int(c)): n for a, c, n in zip(contacts["p1"], contacts["p2"], contacts["normal"])}
    err = max(np.abs(n - nmap[(int(a), int(c))]).max() for (a, c), n in zip(got["pairs"], got["normal"]))
    prim = e.get_contacts(slot)[0][b]
    want_prim = set(o.prim_contacts(ref["id"])["particle"].tolist())
    print(f"\n[{name}] rollout {b}: contacts {got['count']} layers {got['layers']} primitive contacts {len(want_prim)} worst normal error {err:.2e}")
    assert err <= NORMAL_TOL
    assert st["prim_contacts"][b] == ref["nprim"] and set(np.nonzero(prim >= 0)[0].tolist()) == want_prim
    return got


def run_batch(names, tape_steps=1):
    cases = [sc.reference(n)[0] for n in names]
    e = sc.engine_of(cases[0])
    e.alloc_batch(len(names), tape_steps)
    e.set_state(0, np.stack([c["X"].reshape(-1) for c in cases]), np.stack([c["Vel"].reshape(-1) for c in cases]))
    return e, e.step_forward(0)


@pytest.mark.parametrize("name", sc.ALL)
def test_detection_and_layering_equal_the_oracle(name):
    e, st = run_batch([name])
    try:
        compare_rollout(e, st, 1, 0, name)
    finally:
        e.close()


@pytest.mark.parametrize("names", [("cloud_hubs", "cloud_hubs_b", "cloud_hubs_c"), ("cloud_window_b", "planted_window", "cloud_window_c")],
                         ids=["hubs", "window"])
def test_batch_of_different_contact_counts(names):
    """per-rollout scratch (cell sort, raw pairs, layering tables, meta): every rollout against its own oracle run"""
    e, st = run_batch(names)
    try:
        counts = [compare_rollout(e, st, 1, b, n)["count"] for b, n in enumerate(names)]
        assert len(set(counts)) == len(names)
    finally:
        e.close()


def contact_arrays(e, slot, B):
    return [e.get_self_contacts(slot, rollout=b) for b in range(B)]


def assert_same_contacts(a, b):
    for p, q in zip(a, b):
        assert p["count"] == q["count"] and p["layers"] == q["layers"]
        for k in ("pairs", "layer", "normal"):
            np.testing.assert_array_equal(p[k], q[k])


@pytest.mark.parametrize("names", [("cloud_hubs", "cloud_hubs_b", "cloud_hubs_c"), ("stack4",), ("cloud_1024_threads",)], ids=["hubs", "stack4", "n6241"])
def test_same_step_twice_is_bitwise_equal(names):
    """the pair list is collected with atomics in any order; the rank sort and the stable partition make the result deterministic"""
    e, st = run_batch(names)
    try:
        first = contact_arrays(e, 1, len(names))
        x1 = e.get_state(1)
        e.step_forward(0)
        assert_same_contacts(first, contact_arrays(e, 1, len(names)))
        for p, q in zip(x1, e.get_state(1)):
            np.testing.assert_array_equal(p, q)
        assert first[0]["count"] > 50
    finally:
        e.close()


@pytest.mark.parametrize("names", [("cloud_hubs", "cloud_hubs_b", "cloud_hubs_c"), ("stack4",)], ids=["hubs", "stack4"])
def test_inlined_detection_of_the_fused_kernel_is_bitwise_the_standalone_one(names):
    """dc_rollout_forward over TWO steps is one launch of the fused forward kernel with the detection inlined per step (a sweep of one step
    is not fused: it launches k_self_detect and the step kernel like dc_step_forward); two dc_step_forward calls launch k_self_detect and
    the step kernel per step. The launch count the engine reports proves the fused launch; the second step detects on the state the
    first one left (the clouds: after one PD iteration)."""
    S = 2
    e, st = run_batch(names, tape_steps=S)
    try:
        B = len(names)
        e.step_forward(1)
        stepped = [dict(contacts=contact_arrays(e, s, B), state=e.get_state(s), prim=e.get_contacts(s), record=e.get_record(s)) for s in (1, 2)]
        e.kernel_times(reset=True)
        e.rollout_forward(0, S)
        assert e.kernel_times()["fwd_launches"] == 1         # fused: one launch for both steps (two when every step is launched)
        for s, want in zip((1, 2), stepped):
            assert_same_contacts(want["contacts"], contact_arrays(e, s, B))
            for a, b in zip(want["state"] + want["prim"] + want["record"], e.get_state(s) + e.get_contacts(s) + e.get_record(s)):
                np.testing.assert_array_equal(a, b)
            assert want["contacts"][0]["count"] > 50
    finally:
        e.close()
