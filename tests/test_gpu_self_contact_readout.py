"""Self-contact read-out on the device (dc_get_self_contact_readout, dc_get_self_contact_readout_dev, Engine.self_contact_readout,
BatchedSim.self_contact_readout): per pair {id1, id2, layer, state} and {r_k, jn_k}, per vertex the sum of the +-r_k, per record the totals.

Partner: the fp64 walk of tests/self_readout_model.py, which tests/test_self_readout_model.py holds to the fp64 oracle's SelfContact::d, its
types and Record::r on the same cases. Gates — those of the model's header, no new tolerance:
  r_k, jn_k        |diff| <= GATE k s_k, s_k = |g_A| / m_A + |g_B| / m_B the scale of the friction law's argument at that pair, k the reduced mass
                   (GATE = 4 x the worst deviation of an fp32 replay of the same expressions, measured on the CPU). Where g = f + r_p has
                   cancelled to nothing on BOTH sides (two vertices sticking to the sphere: s_k = 0 in fp64, a rounding residue in any fp32
                   evaluation) the scale is that of the sum's operands, self_readout_model.degenerate(): the flap's three steps have twelve, eleven and ten such
                   pairs (the kernel's r_k there: at most 3.7e-9 against operands of 3), the oracle's cases none
  r_self,i         |diff| <= GATE x the sum of k s_k over the pairs that contain i
  state            equal wherever the decision keeps MARGIN_RECORD from both boundaries of the law
  sums             |diff| <= SUM_RTOL x the sum of the terms' magnitudes; counts exact when no decision lies inside the margin
  sum_i r_self,i   zero to GATE x sum |r_k|
On the engine's own records the model is evaluated on the record the engine reports (get_record, get_contacts, get_self_contacts), and the
stored R is held to r_p + r_self within 2 GATE max |f + R|.
"""
import ctypes as C

import numpy as np
import pytest
import torch          # before the engine's library: both must share ONE HIP runtime (torch's), see tests/test_gpu_functional.py

import contact_readout_scenes as cs
import records
import self_readout_model as srm
import selfdetect_cases as sd
import test_gpu_contact_readout as cr
from diffcloth_amd import capi
from diffcloth_amd.functional import BatchedSim, sim_rollout, sim_step

pytestmark = pytest.mark.gpu
GATE, f32 = srm.GATE, cs.f32
PAD = np.array([-1, -1, -1, 0], dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------- comparison with a walk
def compare(out, k, b, pairs, layer, normal, w, lines, tag, nlayers=None):
    """record k, rollout b of a host-form read-out against the fp64 walk `w` on (pairs, layer, normal); contacts are matched by (id1, id2)"""
    P, I, V, T = out["pairs"][k, b], out["impulse"][k, b], out["vertex_impulse"][k, b], out["totals"][k, b]
    Cn = len(layer)
    assert T[0] == Cn and T[1] == (int(np.max(layer)) + 1 if nlayers is None else nlayers) and T[2] == len(np.unique(pairs)), (tag, T[:3])
    assert np.all(P[Cn:] == PAD) and np.all(I[Cn:] == 0), tag
    where = {(int(a), int(c)): q for q, (a, c) in enumerate(P[:Cn, :2])}
    assert len(where) == Cn, tag
    idx = np.array([where[(int(a), int(c))] for a, c in pairs], dtype=np.int64)
    np.testing.assert_array_equal(P[idx, 2], layer, err_msg=tag)
    assert np.all(np.diff(P[:Cn, 2]) >= 0), tag                          # listed in layer order
    flat = srm.degenerate(w)               # g cancelled to nothing on both sides: the operands' scale (self_readout_model.degenerate)
    ks = w["k"] * np.where(flat, w["o"], w["s"])
    assert np.all(I[idx][ks == 0] == 0), tag                             # (f = r = 0 on both sides: zeros, exactly)
    ks = np.where(ks == 0, 1e-300, ks)
    er = np.linalg.norm(I[idx, :3] - w["r"], axis=1) / ks
    ej = np.abs(I[idx, 3] - w["jn"]) / ks
    assert np.all(I[:, 3] >= 0), tag
    safe = (srm.decision_margin(normal, w["d"], w["s"]) > srm.MARGIN_RECORD) & ~flat
    scale_v = np.zeros(len(V))
    np.add.at(scale_v, pairs[:, 0], ks)
    np.add.at(scale_v, pairs[:, 1], ks)
    ev = np.linalg.norm(V - w["r_self"], axis=1)
    touched = scale_v > 0
    sum_r = np.linalg.norm(w["r"], axis=1).sum()
    counts = np.array([np.sum(w["state"] == q) for q in (1, 2, 3)])
    lines.append(f"{tag}: {Cn} contacts, {int(T[1])} layers, {int(T[2])} vertices; states {T[5:8].astype(int)} (model {counts}), {int(np.sum(~safe))} inside the margin, {int(flat.sum())} with g = 0 on both sides; "
                 f"worst |r_k diff| / k s {er.max():.2e}  |jn diff| / k s {ej.max():.2e}  |r_self diff| / sum k s {np.max(ev[touched] / scale_v[touched]):.2e} (GATE {GATE:.1e}); "
                 f"sum jn diff {abs(T[3] - w['jn'].sum()):.2e}  sum |r_T| diff {abs(T[4] - w['rt'].sum()):.2e} / {sum_r:.2e}; |sum_i r_self| {np.linalg.norm(V.sum(axis=0)):.2e}")
    assert er.max() <= GATE and ej.max() <= GATE, lines[-1]
    np.testing.assert_array_equal(P[idx, 3][safe], w["state"][safe], err_msg=tag)
    assert np.all(V[~touched] == 0), tag
    assert np.all(ev <= GATE * scale_v), lines[-1]
    assert abs(T[3] - w["jn"].sum()) <= srm.SUM_RTOL * sum_r and abs(T[4] - w["rt"].sum()) <= srm.SUM_RTOL * sum_r, lines[-1]
    assert T[5:8].sum() == Cn and np.all(np.abs(T[5:8] - counts) <= np.sum(~safe)), lines[-1]
    np.testing.assert_array_equal(T[5:8], [np.sum(P[:Cn, 3] == q) for q in (1, 2, 3)], err_msg=tag)
    assert np.linalg.norm(V.sum(axis=0)) <= GATE * sum_r, lines[-1]
    # the totals are the sums of what is listed
    assert T[3] == pytest.approx(I[:Cn, 3].sum(), rel=1e-12), tag


def handed_in(names, tape=1, slots=(1,), **params):
    """an engine holding the ORACLE's records of `names` (one rollout each) at `slots`, and their walks"""
    refs = [sd.reference(n) for n in names]
    e = sd.engine_of(refs[0][0], **params)
    e.alloc_batch(len(names), tape)
    recs = [records.oracle_record(o, ref) for _, o, ref, _, _ in refs]
    for s in slots:
        records.upload_oracle_records(e, s, recs)
    return e, [srm.oracle_walk(n) for n in names]


def compare_oracle(out, k, b, q, lines, tag):
    compare(out, k, b, q["pairs"], q["sc"]["layer"], q["sc"]["normal"], q["w"], lines, tag)


# ---------------------------------------------------------------------------------------------------------------- oracle records handed in
@pytest.mark.parametrize("names", [("stack3",), ("stack4_sphere",), ("zigzag40",), ("stack4_29",), ("with_sphere",), ("cloud_hubs", "cloud_hubs_b", "cloud_hubs_c")],
                         ids=lambda n: n[0] if len(n) == 1 else "hubs_batch")
def test_oracle_records_handed_in(names):
    e, qs = handed_in(names)
    lines = []
    try:
        out = e.self_contact_readout(1)
        for b, (n, q) in enumerate(zip(names, qs)):
            compare_oracle(out, 0, b, q, lines, n)
        assert len({int(t[0]) for t in out["totals"][0]}) == len(names)          # a batch: different counts per rollout
    finally:
        print("\n[self-contact read-out, oracle records]\n" + "\n".join(lines))
        e.close()


# ---------------------------------------------------------------------------------------------------------------- the engine's own records
def own_walk(e, slot, b, mu):
    """the fp64 walk on the record the engine reports for rollout b (static primitives: d = f)"""
    f, R = e.get_record(slot)
    grp, nrm = e.get_contacts(slot)
    lst = e.get_self_contacts(slot, rollout=b, cap=e.max_self_contacts)
    m = f32(e.vertex_data()[0])
    ids = np.nonzero(grp[b] >= 0)[0]
    rp = srm.prim_part(f[b], ids, nrm[b].reshape(-1, 3)[ids], mu)
    w = srm.walk(f[b], m, lst["pairs"], lst["layer"], lst["normal"], rp=rp)
    return lst, w, rp, f[b].reshape(-1, 3), R[b].reshape(-1, 3)


def check_own(e, out, k, slot, b, mu, lines, tag):
    lst, w, rp, f, R = own_walk(e, slot, b, mu)
    Cn = lst["count"]
    assert Cn >= 10, tag
    np.testing.assert_array_equal(out["pairs"][k, b][:Cn, :2], lst["pairs"], err_msg=tag)           # dc_get_self_contacts, exactly and in its order
    np.testing.assert_array_equal(out["pairs"][k, b][:Cn, 2], lst["layer"], err_msg=tag)
    compare(out, k, b, lst["pairs"], lst["layer"], lst["normal"], w, lines, tag, nlayers=lst["layers"])
    # the stored R is r_p + r_self of the stored f
    verts = np.unique(lst["pairs"])
    miss = np.linalg.norm(R[verts] - (rp[verts] + out["vertex_impulse"][k, b][verts]), axis=1).max()
    bound = 2 * GATE * np.linalg.norm(f[verts] + R[verts], axis=1).max()
    lines.append(f"{tag}: worst |R - (r_p + r_self)| {miss:.2e}, bound {bound:.2e}")
    assert miss <= bound, lines[-1]
    return Cn


def test_own_records_stack4_sphere():
    case = sd.reference("stack4_sphere")[0]
    e = sd.engine_of(case)
    e.alloc_batch(1, 1)
    e.set_state(0, case["X"].reshape(1, -1), case["Vel"].reshape(1, -1))
    st = e.step_forward(0)
    lines = []
    try:
        assert st["self_overflow"][0] == 0
        out = e.self_contact_readout(1)
        check_own(e, out, 0, 1, 0, case["sphere"]["mu"], lines, "stack4_sphere, own step")
        assert out["totals"][0, 0, 1] > 100                             # a deep list: the one-wave walk
    finally:
        print("\n[self-contact read-out, own record]\n" + "\n".join(lines))
        e.close()


def flap_engine():
    sc = cs.scene("flap")
    e = cr.make_engine(sc)
    cr.prepare(sc, e)
    for s in range(sc.steps):
        e.set_state(s, sc.Xe[s], sc.Ve[s])
        assert np.all(e.step_forward(s)["converged"] == 1)
    return sc, e


def test_own_records_flap_on_the_sphere():
    sc, e = flap_engine()
    lines = []
    try:
        out = e.self_contact_readout(1, sc.steps)
        wide = 0
        for s in range(sc.steps):
            check_own(e, out, s, s + 1, 0, sc.mu[0][0], lines, f"flap, step {s}")
            wide += out["totals"][s, 0, 1] <= 8
        assert wide >= 1                                                # a wide list: the whole workgroup takes a layer
        # primitive and self contact at one vertex: the primitive start is live on this scene
        grp = e.get_contacts(1)[0][0]
        assert np.sum(grp[np.unique(out["pairs"][0, 0][:int(out["totals"][0, 0, 0]), :2])] >= 0) >= 1
    finally:
        print("\n[self-contact read-out, flap]\n" + "\n".join(lines))
        e.close()


# ---------------------------------------------------------------------------------------------------------------- bit for bit
def same(a, b, keys=("pairs", "impulse", "vertex_impulse", "totals")):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def dev_form(e, slot0, nslots, cap, dtype, offset=0):
    """the _dev form into buffers that start `offset` elements into their allocation; returns numpy copies and the guard elements"""
    dev = torch.device("cuda", 0)
    B, N = e.B, e.N
    shapes = dict(pairs=(nslots, B, cap, 4), impulse=(nslots, B, cap, 4), vertex_impulse=(nslots, B, N, 3), totals=(nslots, B, 8))
    raw, view = {}, {}
    for k, shp in shapes.items():
        dt = torch.int32 if k == "pairs" else dtype
        raw[k] = torch.full((int(np.prod(shp)) + offset,), -7, dtype=dt, device=dev)
        view[k] = raw[k][offset:].view(shp)
    e.self_contact_readout_dev(slot0, nslots, cap, view["pairs"], view["impulse"], view["vertex_impulse"], view["totals"])
    e.sync()
    return {k: v.cpu().numpy() for k, v in view.items()}, [float(raw[k][0]) for k in raw if offset]


def test_bit_for_bit_forms_ranges_repeats_caps_and_views(monkeypatch):
    # slot 1: the oracle's stack4_sphere record, slot 2: its stack3 record (the same mesh; no primitive contact)
    e, (q4,) = handed_in(("stack4_sphere",), tape=2)
    o3, ref3 = sd.reference("stack3")[1:3]
    records.upload_oracle_records(e, 2, [records.oracle_record(o3, ref3)])
    lines = []
    try:
        cap = 1024
        host = e.self_contact_readout(1, 2, cap=cap)
        compare_oracle(host, 0, 0, q4, lines, "slot 1")
        compare_oracle(host, 1, 0, srm.oracle_walk("stack3"), lines, "slot 2")
        same(host, e.self_contact_readout(1, 2, cap=cap))                            # twice the same call
        for s in range(2):                                                          # a range = per-slot calls
            one = e.self_contact_readout(s + 1, 1, cap=cap)
            for k in host:
                np.testing.assert_array_equal(host[k][s], one[k][0])
        only = e.self_contact_readout(2, 1, cap=cap, pairs=False, impulse=False, vertex_impulse=False)      # an output alone
        assert only["pairs"] is None and only["impulse"] is None and only["vertex_impulse"] is None
        np.testing.assert_array_equal(only["totals"][0], host["totals"][1])
        np.testing.assert_array_equal(e.self_contact_readout(2, 1, cap=0, pairs=False, impulse=False, totals=False)["vertex_impulse"][0], host["vertex_impulse"][1])
        np.testing.assert_array_equal(e.self_contact_readout(1, 1, cap=cap, impulse=False, vertex_impulse=False, totals=False)["pairs"][0], host["pairs"][0])
        # host form = _dev form in fp64, and in fp32 up to the cast; output views that are not 16-byte aligned
        for dtype, offset in ((torch.float64, 0), (torch.float64, 1), (torch.float32, 0), (torch.float32, 1)):
            got, guards = dev_form(e, 1, 2, cap, dtype, offset)
            np.testing.assert_array_equal(got["pairs"], host["pairs"])
            for k in ("impulse", "vertex_impulse", "totals"):
                np.testing.assert_array_equal(got[k], host[k] if dtype == torch.float64 else host[k].astype(np.float32), err_msg=k)
            assert all(g == -7 for g in guards)
        # cap smaller than the count: the prefix, and sums that still hold every contact
        Cn = int(host["totals"][0, 0, 0])
        small = e.self_contact_readout(1, 2, cap=Cn // 3)
        np.testing.assert_array_equal(small["pairs"], host["pairs"][:, :, :Cn // 3])
        np.testing.assert_array_equal(small["impulse"], host["impulse"][:, :, :Cn // 3])
        same(small, host, keys=("vertex_impulse", "totals"))
        # the global-memory walk = the LDS walk
        monkeypatch.setenv("DC_TEST_SELFRO_LDS", "64")
        same(host, e.self_contact_readout(1, 2, cap=cap))
        got, _ = dev_form(e, 1, 2, cap, torch.float32)
        np.testing.assert_array_equal(got["impulse"], host["impulse"].astype(np.float32))
        np.testing.assert_array_equal(got["totals"], host["totals"].astype(np.float32))
        monkeypatch.delenv("DC_TEST_SELFRO_LDS")
        same(host, e.self_contact_readout(1, 2, cap=cap))
    finally:
        print("\n[self-contact read-out, bit for bit]\n" + "\n".join(lines))
        e.close()


def test_global_memory_walk_on_wide_layers_and_a_batch(monkeypatch):
    """the hubs batch (three rollouts, different counts; its scratch planes are per rollout) and the flap's wide layers under a small LDS plan"""
    e, qs = handed_in(("cloud_hubs", "cloud_hubs_b", "cloud_hubs_c"))
    sc, ef = flap_engine()
    try:
        host, hf = e.self_contact_readout(1), ef.self_contact_readout(1, sc.steps)
        monkeypatch.setenv("DC_TEST_SELFRO_LDS", "1")
        same(host, e.self_contact_readout(1))
        same(hf, ef.self_contact_readout(1, sc.steps))
        assert host["totals"][0, :, 0].min() > 50 and hf["totals"][:, 0, 0].min() >= 10
    finally:
        e.close()
        ef.close()


def test_fused_sweep_records_equal_per_step_records():
    names = ("cloud_hubs", "cloud_hubs_b", "cloud_hubs_c")
    cases = [sd.reference(n)[0] for n in names]
    e = sd.engine_of(cases[0])
    e.alloc_batch(len(names), 2)
    X, Vel = np.stack([c["X"].reshape(-1) for c in cases]), np.stack([c["Vel"].reshape(-1) for c in cases])
    try:
        e.set_state(0, X, Vel)
        e.step_forward(0)
        e.step_forward(1)
        a = e.self_contact_readout(1, 2)
        e.set_state(0, X, Vel)
        e.rollout_forward(0, 2)
        same(a, e.self_contact_readout(1, 2))
        assert a["totals"][:, :, 0].min() > 20
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------- other paths and inputs
def test_split_kernels_records(monkeypatch):
    monkeypatch.setenv("DC_CLUSTER", "2")
    case = sd.reference("stack4_29")[0]
    e = sd.engine_of(case)
    e.alloc_batch(1, 1)
    assert e.cluster() == 2
    e.set_state(0, case["X"].reshape(1, -1), case["Vel"].reshape(1, -1))
    st = e.step_forward(0)
    lines = []
    try:
        assert st["self_overflow"][0] == 0
        check_own(e, e.self_contact_readout(1), 0, 1, 0, 0.0, lines, "stack4_29, K = 2")
    finally:
        print("\n[self-contact read-out, 29 x 29, K = 2]\n" + "\n".join(lines))
        e.close()


def test_renumbered_mesh(monkeypatch):
    monkeypatch.setenv("DC_RENUMBER", "1")
    e, (q,) = handed_in(("stack3",))
    lines = []
    try:
        assert e.layout()["renumbered"]
        compare_oracle(e.self_contact_readout(1), 0, 0, q, lines, "stack3, renumbered")          # ids and vertex rows in the caller's numbering
    finally:
        print("\n[self-contact read-out, renumbered]\n" + "\n".join(lines))
        e.close()


def assert_empty(out, N):
    assert np.all(out["pairs"] == PAD) and np.all(out["impulse"] == 0) and np.all(out["vertex_impulse"] == 0) and np.all(out["totals"] == 0)
    assert out["vertex_impulse"].shape[-2:] == (N, 3)


@pytest.mark.parametrize("selfcollision", [1, 0])
def test_no_self_contacts(selfcollision):
    """the flat cloth at rest (a record without self contacts), and the folded stack on a context with self-collision off"""
    case = sd.reference("stack3")[0]
    e = sd.engine_of(case, selfcollision_enabled=selfcollision)
    e.alloc_batch(2, 1)
    X = case["X"].reshape(1, -1) if not selfcollision else case["V"].reshape(1, -1)
    e.set_state(0, np.tile(X, (2, 1)), np.zeros((2, X.shape[1])))
    e.step_forward(0)
    try:
        assert e.get_self_contacts(1)["count"] == 0
        assert_empty(e.self_contact_readout(1, cap=16), e.N)
        got, _ = dev_form(e, 1, 1, 16, torch.float32, offset=1)
        assert_empty(got, e.N)
    finally:
        e.close()


def test_batched_sim_after_sim_step_and_sim_rollout(monkeypatch):
    sc = cs.scene("flap")
    e = cr.make_engine(sc)
    S, B = sc.steps, sc.nb
    cr.prepare(sc, e)
    sim = BatchedSim(e, S)
    dev = torch.device("cuda", 0)
    syncs = []
    real_sync = capi.Engine.sync
    monkeypatch.setattr(capi.Engine, "sync", lambda self: (syncs.append(1), real_sync(self))[1])
    side = torch.cuda.Stream(device=dev)
    a = torch.zeros((B, 0), device=dev)
    cap = 512
    try:
        with torch.cuda.stream(side):
            x = torch.as_tensor(sc.Xe[0], dtype=torch.float32, device=dev)
            v = torch.as_tensor(sc.Ve[0], dtype=torch.float32, device=dev)
            for s in range(S):
                x, v = sim_step(sim, x, v, a)
            n0 = len(syncs)
            got = sim.self_contact_readout(cap=cap)
            got64 = sim.self_contact_readout(2, 1, cap=cap, dtype=torch.float64)
            full = sim.self_contact_readout(1, 1, totals=False, vertex_impulse=False)
            assert len(syncs) == n0                                     # nothing on the path synchronises
        side.synchronize()
        host = e.self_contact_readout(1, S, cap=cap)
        assert got["pairs"].dtype == torch.int32 and got["pairs"].shape == (S, B, cap, 4) and got["vertex_impulse"].shape == (S, B, sc.N, 3)
        assert full["pairs"].shape == (1, B, e.max_self_contacts, 4) and full["totals"] is None
        for k in host:
            assert got[k].is_cuda and not got[k].requires_grad
            np.testing.assert_array_equal(got[k].cpu().numpy(), host[k].astype(got[k].cpu().numpy().dtype))
            np.testing.assert_array_equal(got64[k].cpu().numpy()[0], host[k][1])
        assert host["totals"][:, :, 0].min() >= 10
        # after a sim_rollout forward pass, on the side stream
        with torch.cuda.stream(side):
            x0 = torch.as_tensor(sc.Xe[0], dtype=torch.float32, device=dev).requires_grad_(True)
            v0 = torch.as_tensor(sc.Ve[0], dtype=torch.float32, device=dev)
            sim_rollout(sim, x0, v0, None, steps=S)
            n0 = len(syncs)
            roll = sim.self_contact_readout(1, cap=cap)
            assert len(syncs) == n0
        side.synchronize()
        host = e.self_contact_readout(1, S, cap=cap)
        for k in host:
            assert not roll[k].requires_grad
            np.testing.assert_array_equal(roll[k].cpu().numpy(), host[k].astype(roll[k].cpu().numpy().dtype))
        assert host["totals"][:, :, 0].min() >= 10
        with pytest.raises(ValueError, match="step"):
            sim.self_contact_readout(1, S + 1)
    finally:
        e.close()


def test_refusals():
    case = sd.reference("stack3")[0]
    e = sd.engine_of(case)
    e.alloc_batch(2, 3)
    lib, h = e.lib, e.h
    buf = np.zeros(2 * 3 * e.N * 16)
    p = C.c_void_p(buf.ctypes.data)
    try:
        for args, msg in (((0, 1, 4, p, p, p, p), "slot 0"), ((1, 0, 4, p, p, p, p), "nslots"), ((2, 3, 4, p, p, p, p), "past the tape"),
                          ((1, 1, 4, None, None, None, None), "all null"), ((1, 1, 0, p, None, None, None), "cap < 1"), ((1, 1, 0, None, p, p, p), "cap < 1")):
            for name, extra in (("dc_get_self_contact_readout", ()), ("dc_get_self_contact_readout_dev", (0,))):
                assert getattr(lib, name)(h, *args, *extra) == 1, (name, msg)           # DC_ERR_INVALID
                assert msg in lib.dc_last_error(h).decode(), (name, lib.dc_last_error(h))
        assert np.all(buf == 0)
        with pytest.raises(capi.DcError, match="past the tape"):
            e.self_contact_readout(3, 2)
    finally:
        e.close()
