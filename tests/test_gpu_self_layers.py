"""Hundreds of contact layers through the layered friction passes and the adjoint's transposed layer walk: the folded stacks of
tests/selfdetect_cases.py (stack3: 193 layers; stack4 on a sphere: 409 layers, hubs of degree 5, primitive contacts seeding the frontier;
stack4_29: 524 layers on 841 vertices; zigzag40: 241 layers on 1 600 vertices, the one deep list whose working set fits the LDS of the
one-workgroup kernels) against the fp64 oracle — forward, then backward in every adjoint_mode, end to end against the
oracle's direct solve and on one and the same record in both directions (tests/records.py), flat 1e-4. zigzag40 and stack4 again in a
context built with DC_SELF_LDS=0 (test_layered_passes_with_and_without_lds works out which path each build takes), stack4_29 split over
two workgroups on both self-friction paths.
The parity tests before these stop at two layers (tests/test_gpu_selfcontact.py).

The oracle's own dL/dx, dL/dv, dL/dmu move by little (<= 2.2e-7 on the stacks) under a float32 rounding of its x_new on these states
(measured per case below and entered in the ledger): they are well conditioned, no gate is widened."""
import numpy as np
import pytest

import ledger
import records
import selfdetect_cases as sc
from diffcloth_amd import capi
from test_gpu_selfdetect_cases import compare_rollout
from test_gpu_split_self_friction import env

pytestmark = pytest.mark.gpu
POS_TOL, R_TOL, GRAD_TOL = 4.5e-5, 2e-3, 1e-4          # the gates of tests/test_gpu_selfcontact.py and BASELINE.json's flat 1e-4
STACKS = ["stack3", "stack4_sphere", "stack4_29", "zigzag40"]
DENSE_MAX_N = 768                                      # adjoint_mode 2 is refused above (kDenseMaxN, csrc/dc_adjoint_dense.h)
ITER_CAP = 400                                         # dc_params::adjoint_iter_cap's default (Simulation.cpp:1562)
_BACKWARD = {}


def oracle_backward(name):
    """seed gradients, the oracle's direct solve on its own record, the record as dc_set_record takes it, and the sensitivity of the
    oracle's own gradients to a float32 rounding of x_new (on a second record of the same step: the shared one stays as it is)"""
    if name not in _BACKWARD:
        case, o, ref, _, _ = sc.reference(name)
        rng = np.random.default_rng(5)
        gx = sc.f32(rng.standard_normal(case["X"].size)); gv = sc.f32(0.01 * rng.standard_normal(case["X"].size))
        rb = o.step_backward(ref["id"], gx, gv, is_start=False, direct=True)
        assert rb["converged"] and rb["direct_residual"] <= 1e-12
        ref2 = o.step(case["X"].reshape(-1), case["Vel"].reshape(-1))
        o.override_record(ref2["id"], x=sc.f32(ref2["x"]))
        sens = grad_errors(o.step_backward(ref2["id"], gx, gv, is_start=False, direct=True), rb, 0)
        _BACKWARD[name] = dict(gx=gx, gv=gv, rb=rb, rec=records.oracle_record(o, ref), sens=max(sens.values()))
    return _BACKWARD[name]


def grad_errors(g, rb, b=0):
    pick = (lambda a: a[b]) if np.ndim(g["dL_dx"]) == 2 else (lambda a: a)
    out = dict(dx=records.rel(pick(g["dL_dx"]), rb["dL_dx"]), dv=records.rel(pick(g["dL_dv"]), rb["dL_dv"]))
    if len(rb["dL_dmu"]):
        out["dmu"] = records.mu_err(pick(g["dL_dmu"]), rb["dL_dmu"])
    return out


def fmt(d):
    return " ".join(f"{k} {v:.1e}" for k, v in d.items())


def forward(e, name, tag):
    """one step from the case's state: detection as in tests/test_gpu_selfdetect_cases.py, state and record against the oracle"""
    case, o, ref, _, _ = sc.reference(name)
    e.set_state(0, case["X"].reshape(-1), case["Vel"].reshape(-1))
    st = e.step_forward(0)
    compare_rollout(e, st, 1, 0, name)
    x1, v1 = e.get_state(1)
    f, r = e.get_record(1)
    rf, rr = o.record_fr(ref["id"])
    dx = np.abs(x1[0] - ref["x"]).max()
    er = np.linalg.norm(r[0] - rr) / np.linalg.norm(rr)
    print(f"[{tag}] forward: PD iterations {st['pd_iters'][0]} (oracle {ref['iters']}), converged {st['converged'][0]}, max|dx| {dx:.2e}, rel err r {er:.2e}")
    assert st["converged"][0] in (1, 2) and ref["converged"]
    assert st["pd_iters"][0] == ref["iters"]                 # the layered passes change nothing about the convergence
    assert dx <= POS_TOL and er <= R_TOL
    return dict(x=x1, v=v1, f=f, r=r, contacts=e.get_self_contacts(1), prim=e.get_contacts(1))


def backward_three_ways(e, name, fw, tag, test):
    """end to end against the oracle's direct solve; the oracle on the engine's record; the engine on the oracle's record"""
    case, o, ref, _, _ = sc.reference(name)
    bk = oracle_backward(name)
    gb = e.step_backward(1, bk["gx"], bk["gv"], is_start=False)
    e2e = grad_errors(gb, bk["rb"])
    ref2 = o.step(case["X"].reshape(-1), case["Vel"].reshape(-1))         # a record of its own for the adoption
    matched = records.oracle_adopts_gpu_record(o, ref2["id"], e, 1, 0, case["X"].reshape(-1), fw["x"][0], fw["v"][0], fw["f"][0], case["h"], normals=fw["prim"][1])
    assert matched == ref["nself"]
    adopt = grad_errors(gb, o.step_backward(ref2["id"], bk["gx"], bk["gv"], is_start=False, direct=True))
    records.upload_oracle_records(e, 1, [bk["rec"]])
    gt = e.step_backward(1, bk["gx"], bk["gv"], is_start=False)
    forced = grad_errors(gt, bk["rb"])
    print(f"[{tag}] backward: used_direct {gb['used_direct'][0]} converged {gb['converged'][0]} adjoint iterations {gb['adjoint_iters'][0]} refine {gb['refine_cycles'][0]} "
          f"fp64 iterations {gb['fp64_iters'][0]} workgroups {gb['workgroups'][0]}; end to end {fmt(e2e)}; oracle adopts the engine's record {fmt(adopt)}; "
          f"engine on the oracle's record {fmt(forced)}; oracle's own float32-x_new sensitivity {bk['sens']:.1e}")
    ledger.add(test, tag, 0, max(e2e.values()), sensitivity=bk["sens"], gate=GRAD_TOL, same_record_adopt=max(adopt.values()),
               same_record_forced=max(forced.values()))
    assert gb["converged"][0] in (1, 2) and gt["converged"][0] in (1, 2)
    assert max(adopt.values()) <= GRAD_TOL and max(forced.values()) <= GRAD_TOL      # the adjoint kernels, on one and the same record
    assert max(e2e.values()) <= GRAD_TOL
    return gb, gt


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("name", STACKS)
def test_deep_layers_forward_and_backward(name, mode):
    case = sc.reference(name)[0]
    tag = f"{name} mode {mode}"
    if mode == 2 and len(case["X"]) > DENSE_MAX_N:
        with pytest.raises(capi.DcError) as info:                         # reported, not a quiet change of solver
            sc.engine_of(case, adjoint_mode=2)
        assert "adjoint_mode 2" in str(info.value)
        return
    e = sc.engine_of(case, adjoint_mode=mode)
    try:
        e.alloc_batch(1, 1)
        print()
        fw = forward(e, name, tag)
        for gb in backward_three_ways(e, name, fw, tag, "test_deep_layers_forward_and_backward"):
            if mode == 0:
                # the reference's iteration u <- u + P^-1 (g - K u), every product a transposed walk over the layers. Its fp32 iterates do not
                # settle to the 1e-9 per vertex asked for here (the fp64 oracle's do, in 39 ... 123 iterations), so it runs into its cap and
                # the direct solve takes over from its last iterate, as in the reference (Simulation.cpp:1589-1594) — reported, not silent
                assert (gb["used_direct"][0], gb["adjoint_iters"][0]) == (1, ITER_CAP)
                assert gb["workgroups"][0] == 1
            else:
                assert gb["used_direct"][0] == mode
            if mode == 3:
                # the band holds P's pattern; a contact that couples outside it is flagged and the rollout takes the fp64 iteration — reported
                assert gb["converged"][0] == 1 and gb["residual_verified"][0] == 1
                fell_back = gb["fp64_iters"][0] > 0
                assert (gb["refine_cycles"][0] == 0) == fell_back, (gb["refine_cycles"][0], gb["fp64_iters"][0])
                print(f"[{tag}] band {e.adjoint_band()}: " + ("out-of-band contacts flagged, fp64 fall-back reported" if fell_back else "factors used"))
    finally:
        e.close()


def snapshot(e, name, tag, test):
    fw = forward(e, name, tag)
    gb, gt = backward_three_ways(e, name, fw, tag, test)
    return fw, gb, gt


def assert_bitwise(a, b, what):
    fa, ga, ta = a
    fb, gb, tb = b
    for k in ("x", "v", "f", "r"):
        np.testing.assert_array_equal(fa[k], fb[k], err_msg=f"{what}: {k}")
    assert fa["contacts"]["count"] == fb["contacts"]["count"] and fa["contacts"]["layers"] == fb["contacts"]["layers"]
    for k in ("pairs", "layer", "normal"):
        np.testing.assert_array_equal(fa["contacts"][k], fb["contacts"][k], err_msg=f"{what}: contact {k}")
    for p, q in zip(fa["prim"], fb["prim"]):
        np.testing.assert_array_equal(p, q, err_msg=f"{what}: primitive contacts")


def working_set(name):
    """(floats the layered passes need in LDS, floats the one-workgroup forward kernel offers them) for the oracle's contact list"""
    case, _, ref, layered, _ = sc.reference(name)
    M = len({v for _, a, b in layered for v in (a, b)})
    return sc.self_lds_need(M, ref["nself"], ref["nlayers"]), sc.forward_lds_floats(len(case["X"]))


@pytest.mark.parametrize("name", ["zigzag40", "stack4_sphere"])
def test_layered_passes_with_and_without_lds(name):
    """DC_SELF_LDS=0 (read by dc_build) sends the layered friction passes and the adjoint's layer walk through global memory. The engine
    reports no path, so which one a default build takes is worked out here from the kernels' own rule (need <= offered floats):
      zigzag40 (1 600 vertices, 280 contacts, 241 layers, 5 563 floats of 6 144): the default build runs the passes in LDS — the single-wave
        walk beyond kWideLayers — forward, and in the adjoint (two element windows: >= 8 N / 2 = 6 400 floats); the switch changes the path.
      stack4_sphere (256 vertices, 5 915 floats of 1 536): the one-workgroup passes run in global memory under either setting; the two
        builds are compared as the same path (what the switch must then leave untouched).
    Both builds against the oracle at the gates above; the contact arrays of the two builds bit for bit equal."""
    case = sc.reference(name)[0]
    need, offered = working_set(name)
    fits = need <= offered
    assert fits == (name == "zigzag40"), (need, offered)
    out = {}
    for lds in (1, 0):
        with env(DC_SELF_LDS=lds):
            e = sc.engine_of(case, adjoint_mode=1)
        try:
            lay = e.layout()
            assert lay["packet_kernel"]                    # the kernel whose budget forward_lds_floats restates
            if fits:
                assert lay["element_windows"] and need <= sc.adjoint_lds_floats_at_least(len(case["X"]), lay["windows"]), lay
            with env(DC_CLUSTER=1):                        # one workgroup per rollout, forward and backward: the budgets worked out above
                e.alloc_batch(1, 1)
            assert e.cluster() == 1
            print()
            out[lds] = snapshot(e, name, f"{name} DC_SELF_LDS={lds}", "test_layered_passes_with_and_without_lds")
            assert out[lds][1]["workgroups"][0] == 1 and out[lds][2]["workgroups"][0] == 1
        finally:
            e.close()
    fa, fb = out[1][0], out[0][0]
    assert fa["contacts"]["count"] == fb["contacts"]["count"] and fa["contacts"]["layers"] == fb["contacts"]["layers"]
    for k in ("pairs", "layer", "normal"):
        np.testing.assert_array_equal(fa["contacts"][k], fb["contacts"][k])
    for p, q in zip(fa["prim"], fb["prim"]):
        np.testing.assert_array_equal(p, q)
    d = {k: float(np.abs(fa[k] - fb[k]).max()) for k in ("x", "v", "r")}
    print(f"[{name}] working set {need} floats, forward offers {offered}: " + ("LDS against global-memory passes" if fits else "global-memory passes in both builds")
          + f": max |diff| {fmt(d)}; gradients dx {records.rel(out[0][1]['dL_dx'][0], out[1][1]['dL_dx'][0]):.1e}")


def test_split_rollout_both_self_friction_paths():
    """stack4_29 on two workgroups per rollout: every part walks the 524 layers itself (DC_SELF_REDUNDANT=1) or part 0 alone does (=0);
    dc_get_self_friction_path proves the path. Both against the oracle, and bitwise equal to each other."""
    name = "stack4_29"
    case = sc.reference(name)[0]
    out = {}
    for redundant in (1, 0):
        e = sc.engine_of(case, adjoint_mode=1)
        try:
            with env(DC_CLUSTER=2, DC_SELF_REDUNDANT=redundant):
                e.alloc_batch(1, 1)
            assert e.cluster() == 2
            e.self_friction_path(reset=True)
            print()
            out[redundant] = snapshot(e, name, f"{name} K=2 DC_SELF_REDUNDANT={redundant}", "test_split_rollout_both_self_friction_paths")
            path = e.self_friction_path()
            print(f"[{name}] K=2 redundant={redundant}: PD iterations with a self-friction pass / taken redundantly {path.tolist()}")
            assert path[0, 0] > 0 and path[0, 1] == (path[0, 0] if redundant else 0)
        finally:
            e.close()
    assert_bitwise(out[1], out[0], "redundant against part 0 alone")
    for k in ("dL_dx", "dL_dv", "dL_dmu"):
        np.testing.assert_array_equal(out[1][1][k], out[0][1][k], err_msg=k)
        np.testing.assert_array_equal(out[1][2][k], out[0][2][k], err_msg=k + " on the oracle's record")
