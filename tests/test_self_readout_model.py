"""The fp64 model of the self-contact read-out (tests/self_readout_model.py: the rule of dc_get_self_contact_readout) against the fp64 oracle
on eight cases of tests/selfdetect_cases.py, and the measurement the GPU tests' gate comes from. No GPU.

  * the walk reproduces the oracle's SelfContact::d and type of every contact, and r_p + r_self its Record::r, to 1e-12;
  * every state occurs; leaving out the r_p start or reversing the layer order changes d (the GPU test can only pass if the kernel does both);
  * GATE: 4 x the worst deviation of the fp32 replay from the fp64 walk (self_readout_model.py's header has the figures);
  * the share of contacts whose decision lies inside MARGIN_RECORD is at most 2 % per case (measured: 0 on all eight).
"""
import numpy as np
import pytest

import self_readout_model as srm

EXACT = 1e-12


@pytest.fixture(scope="module")
def walks():
    """per case: the oracle's record and the fp64 walk on it, computed once and left unchanged"""
    return {name: srm.oracle_walk(name) for name in srm.CASES}


@pytest.mark.parametrize("name", srm.CASES)
def test_the_walk_is_the_oracles_layered_friction(walks, name):
    q = walks[name]
    sc, w, pc = q["sc"], q["w"], q["pc"]
    assert len(sc["layer"]) >= 10
    # the primitive part: d = f under a static sphere, r_p the oracle's own
    if len(pc["particle"]):
        assert np.abs(pc["d"] - q["f"][pc["particle"]]).max() <= EXACT * np.abs(q["f"]).max()
        assert np.abs(pc["r"] - q["rp"][pc["particle"]]).max() <= EXACT * np.abs(q["f"]).max()
    ed = np.linalg.norm(w["d"] - sc["d"], axis=1) / w["s"]
    er = np.abs(q["rp"] + w["r_self"] - q["r"]).max() / np.abs(q["r"]).max()
    print(f"\n[{name}] {len(sc['layer'])} contacts, {int(sc['layer'].max()) + 1} layers, {len(pc['particle'])} primitive contacts: "
          f"worst |d - oracle d| / s {ed.max():.1e}, |r_p + r_self - r| / max |r| {er:.1e}")
    assert ed.max() <= EXACT
    np.testing.assert_array_equal(w["state"], sc["type"] + 1)
    assert er <= EXACT
    # sum of the self part over the vertices: every pair adds +r_k and -r_k
    assert np.abs(w["r_self"].sum(axis=0)).max() <= EXACT * np.linalg.norm(w["r"], axis=1).sum()


def test_every_state_occurs(walks):
    counts = {name: np.bincount(walks[name]["w"]["state"], minlength=4)[1:] for name in srm.CASES}
    print("\ntake-off / stick / slide: " + ", ".join(f"{n} {c[0]} / {c[1]} / {c[2]}" for n, c in counts.items()))
    assert np.all(counts["stack4_sphere"] >= 1), counts["stack4_sphere"]
    assert np.all(sum(counts.values()) >= 5)


@pytest.mark.parametrize("name", ["with_sphere", "stack4_sphere"])
def test_the_primitive_start_matters(walks, name):
    q = walks[name]
    bare = srm.walk(q["f"], q["mass"], q["pairs"], q["sc"]["layer"], q["sc"]["normal"], rp=None)
    change = np.linalg.norm(bare["d"] - q["w"]["d"], axis=1) / q["w"]["s"]
    print(f"\n[{name}] g = f alone moves d by up to {change.max():.1e} s at {int(np.sum(change > 100 * srm.GATE))} contacts")
    assert np.sum(change > 100 * srm.GATE) >= 1


@pytest.mark.parametrize("name", ["stack3", "stack4_29"])
def test_the_layer_order_matters(walks, name):
    q = walks[name]
    rev = srm.walk(q["f"], q["mass"], q["pairs"], q["sc"]["layer"], q["sc"]["normal"], rp=q["rp"], reverse_layers=True)
    change = np.linalg.norm(rev["d"] - q["w"]["d"], axis=1) / q["w"]["s"]
    print(f"\n[{name}] the layers in reverse order move d by up to {change.max():.1e} s at {int(np.sum(change > 100 * srm.GATE))} contacts")
    assert np.sum(change > 100 * srm.GATE) >= 5


def test_gate_from_the_fp32_replay(walks):
    worst = {}
    for name in srm.CASES:
        q = walks[name]
        sc, w = q["sc"], q["w"]
        mu = q["case"]["sphere"]["mu"] if q["case"]["sphere"] is not None else 0.0
        rp32 = srm.prim_part(q["f"], q["pc"]["particle"], q["pc"]["normal"], mu, dt=np.float32)
        rep = srm.walk(q["f"], q["mass"], q["pairs"], sc["layer"], sc["normal"], rp=rp32, replay=True)
        np.testing.assert_array_equal(rep["state"], w["state"], err_msg=name)        # (no decision of these cases lies inside the margin)
        ed = np.linalg.norm(rep["d"] - w["d"], axis=1) / w["s"]
        er = np.linalg.norm(rep["r"] - w["r"], axis=1) / (w["k"] * w["s"])
        worst[name] = (float(ed.max()), float(er.max()), int(sc["layer"].max()) + 1)
    lines = [f"  {n}: d {a:.2e}  r {b:.2e}  ({nl} layers)" for n, (a, b, nl) in worst.items()]
    top = max(max(a, b) for a, b, _ in worst.values())
    print("\nfp32 replay against the fp64 walk, relative to s_k (d) and k s_k (r):\n" + "\n".join(lines) + f"\nworst {top:.3e}; 4 x worst = {4 * top:.3e}; GATE = {srm.GATE:.1e}")
    assert 4 * top <= srm.GATE <= 1e-5
    assert srm.GATE <= 1.25 * 4 * top, "the recorded GATE is looser than the measurement it stands for"


@pytest.mark.parametrize("name", srm.CASES)
def test_decisions_keep_the_margin(walks, name):
    q = walks[name]
    inside = srm.decision_margin(q["sc"]["normal"], q["w"]["d"], q["w"]["s"]) <= srm.MARGIN_RECORD
    print(f"\n[{name}] {int(inside.sum())} of {len(inside)} decisions inside MARGIN_RECORD = {srm.MARGIN_RECORD}")
    assert inside.sum() <= srm.MAX_UNSAFE_SHARE * len(inside)
