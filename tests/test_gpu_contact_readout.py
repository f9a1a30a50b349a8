"""Contact read-out on the device (dc_get_contact_readout, dc_get_contact_readout_dev, Engine.contact_readout, BatchedSim.contact_readout):
per vertex the state of the friction law (0 none, 1 take-off, 2 stick, 3 slide) and the normal impulse of the PRIMITIVE part of r, per primitive
group the row {J, tau, sum jn, take-off, stick, slide}.

Partner: the fp64 oracle's prim_contacts (particle, prim = group, type, normal, d, r) and x_new of the same teacher-forced steps
(tests/contact_readout_scenes.py, which also says which margin a decision must keep to be compared, and why). Gates — no new tolerance:
  jn per vertex    |jn - r.n of the oracle| <= GATE_R |d_i|: the gate of the record's r (2e-3, tests/test_gpu_parity.py) on the scale of the law's
                   argument at that contact (|r(d)| <= |d|, and r is 1-Lipschitz in d up to the factor 1 + mu)
  J, sum jn        |diff| <= SUM_RTOL sum |r_p,i|;  tau: |diff| <= SUM_RTOL sum |x_i - c| |r_p,i|   (1e-4, as dL/dw is gated)
On scenes without self contacts the record's r IS r_p, so the read-out is also held to the engine's own dc_get_record: jn = r.n and J = -sum r
to fp32 rounding of a re-evaluation (1e-6 of the contact's |r|).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch          # before the engine's library: both must share ONE HIP runtime (torch's), see tests/test_gpu_functional.py

import contact_readout_scenes as cs
import records
import test_gpu_primitive_velocities as pv
from diffcloth_amd import capi
from diffcloth_amd.functional import BatchedSim, sim_rollout, sim_step

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, f32 = cs.H, cs.f32
REEVAL = 1e-6          # a re-evaluation of the same fp32 expression in another kernel: contraction may differ by an ulp or two


def spins_of(sc):
    om = np.zeros((sc.nb, sc.G, 3))
    for p in sc.prims:
        if p.get("oracle_rotates"):
            om[:, p["group"]] = (0.0, cs.SURFACE_SPEED / p["radius"], 0.0)
    return om


def make_engine(sc, V=None, F=None):
    return pv.make_engine(sc.V if V is None else V, sc.F if F is None else F, sc.prims, att=sc.att, selfcollision=int(sc.selfcollision), fabric=sc.fabric)


def prepare(sc, e, tape=None):
    e.alloc_batch(sc.nb, sc.steps if tape is None else tape)
    e.set_mu(sc.mu)
    if np.abs(sc.W).max() > 0:
        e.set_primitive_velocities(sc.W)
    if np.abs(spins_of(sc)).max() > 0:
        e.set_primitive_spins(spins_of(sc))
    if np.abs(sc.D).max() > 0:
        e.set_primitive_offset_schedule(0, sc.D)


def run_steps(sc, e, steps=None):
    """the engine's own steps from the shared (oracle) states; returns the read-out of every record, taken right after its step (teacher forcing
    overwrites the state of slot s, the x_new of record s, before step s runs)"""
    outs = []
    for s in range(sc.steps if steps is None else steps):
        e.set_state(s, sc.Xe[s], sc.Ve[s])
        st = e.step_forward(s, fixed_pts=None if sc.XF is None else sc.XF[s])
        assert np.all(st["converged"] == 1)
        outs.append(e.contact_readout(s + 1, 1))
    return {k: np.concatenate([o[k] for o in outs]) for k in outs[0]}


def own_record_d(sc, e, slot):
    """per rollout (n [N][3], d [N][3], mu [N], r [N][3], group [N]) of the engine's own record, d re-formed in fp64 from the fp32 values the
    kernel reads: d = f - m (w + radius (omega x n)) (no scene here sets the engine's rotates flag)"""
    f, r = e.get_record(slot)
    grp, nrm = e.get_contacts(slot)
    m = f32(e.vertex_data()[0])
    w, om = e.get_primitive_velocities(slot), e.get_primitive_spins(slot)
    radius = np.array([next(p["radius"] for p in sc.prims if p["group"] == g) for g in range(sc.G)])
    sphere = np.array([next(p["kind"] for p in sc.prims if p["group"] == g) == capi.DC_PRIM_SPHERE for g in range(sc.G)])
    out = []
    for b in range(sc.nb):
        g = np.maximum(grp[b], 0)
        n = nrm[b].reshape(-1, 3)
        vout = w[b][g] + np.where(sphere[g], radius[g], 0.0)[:, None] * np.cross(om[b][g], n)
        out.append((n, f[b].reshape(-1, 3) - m[:, None] * vout, sc.mu[b][g], r[b].reshape(-1, 3), grp[b]))
    return out


def check(sc, e, out, lines, steps=None, oracle_states=True, self_contacts=False, centre=None):
    worst = dict(jn=0.0, J=0.0, tau=0.0, sjn=0.0)
    for s in range(sc.steps if steps is None else steps):
        own = own_record_d(sc, e, s + 1)
        for b in range(sc.nb):
            ex = sc.expected(s, b, None if centre is None else centre[s][b])
            st, jn, wr = out["state"][s, b], out["normal_impulse"][s, b], out["wrench"][s, b]
            n, d, mu, r, grp = own[b]
            tag = f"step {s} rollout {b}"
            # the contact set, and zero everywhere else
            np.testing.assert_array_equal(st != 0, ex["state"] != 0, err_msg=tag)
            np.testing.assert_array_equal(st != 0, grp >= 0, err_msg=tag)
            assert np.all(jn[st == 0] == 0) and np.all(jn[st == 1] == 0) and np.all(jn >= 0), tag
            # state: the oracle's type outside the margin of an own record; the rule on the engine's own record at every contact off the boundary
            if oracle_states:
                sel = ex["safe_step"] & (ex["state"] != 0)
                np.testing.assert_array_equal(st[sel], ex["state"][sel], err_msg=tag)
            ids = np.nonzero(grp >= 0)[0]
            clear = cs.decision_margin(n[ids], d[ids], mu[ids]) > cs.MARGIN_RECORD
            np.testing.assert_array_equal(st[ids][clear], cs.classify(n[ids], d[ids], mu[ids])[clear], err_msg=tag)
            assert clear.sum() >= len(ids) - max(1, len(ids) // 50), tag
            # jn against the oracle
            ej = np.abs(jn - ex["jn"])
            ok = ej <= cs.GATE_R * ex["dnorm"]
            worst["jn"] = max(worst["jn"], float(np.max(ej[ids] / ex["dnorm"][ids])) if len(ids) else 0.0)
            for g in range(sc.G):
                row, want, (sr, st_) = wr[g], ex["rows"][g], ex["scales"][g]
                assert row[7:10].sum() == want[7:10].sum() == np.sum(grp == g), tag
                np.testing.assert_array_equal(row[7:10], [np.sum(st[grp == g] == k) for k in (1, 2, 3)], err_msg=tag)
                eJ, et, es = np.linalg.norm(row[0:3] - want[0:3]), np.linalg.norm(row[3:6] - want[3:6]), abs(row[6] - want[6])
                lines.append(f"{tag} group {g}: contacts {int(want[7:10].sum())} (take-off/stick/slide engine {row[7:10].astype(int)} oracle {want[7:10].astype(int)}) "
                             f"|J diff| {eJ:.2e} / {sr:.2e}  |tau diff| {et:.2e} / {st_:.2e}  |sum jn diff| {es:.2e}  worst jn/|d| {worst['jn']:.2e}")
                if sr == 0.0:
                    assert np.all(row == 0.0), lines[-1]           # a group nothing touches: a row of zeros
                    continue
                worst["J"] = max(worst["J"], eJ / sr); worst["tau"] = max(worst["tau"], et / st_); worst["sjn"] = max(worst["sjn"], es / sr)
                assert eJ <= cs.SUM_RTOL * sr and et <= cs.SUM_RTOL * st_ and es <= cs.SUM_RTOL * sr, lines[-1]
                assert row[6] == pytest.approx(jn[grp == g].sum(), rel=1e-12), tag
                if not self_contacts:                              # the record's r is r_p: the engine's own record says the same
                    rg = r[grp == g]
                    assert np.linalg.norm(row[0:3] + rg.sum(axis=0)) <= REEVAL * np.linalg.norm(rg, axis=1).sum(), lines[-1]
            if not self_contacts:
                rn = np.einsum("kd,kd->k", r, n)
                assert np.all(np.abs(jn - rn)[ids] <= REEVAL * np.linalg.norm(r[ids], axis=1) + 1e-30), tag
            assert np.all(ok), f"{tag}: jn off at {np.nonzero(~ok)[0]}"
    lines.append(f"worst: jn/|d| {worst['jn']:.2e} (gate {cs.GATE_R:.0e})  J {worst['J']:.2e}  tau {worst['tau']:.2e}  sum jn {worst['sjn']:.2e} (gate {cs.SUM_RTOL:.0e})")
    return worst


def run_scene(name, check_kw=None, **kw):
    sc = cs.scene(name)
    e = make_engine(sc)
    prepare(sc, e)
    out = run_steps(sc, e)
    lines = []
    try:
        check(sc, e, out, lines, **(check_kw or {}))
    finally:
        print(f"\n[contact read-out, scene {name}]\n" + "\n".join(lines))
    return sc, e, out


def hand_in_oracle_records(sc, e, s):
    m3 = pv.mass3(e)
    recs = []
    for b in range(sc.nb):
        ref, wt = sc.ref[s][b], np.tile(sc.W[b, 0], sc.N)
        q = dict(x=ref["x"] + wt * H, v=ref["v"] + wt, f=ref["f"] + m3 * wt, r=ref["r"], prim=-np.ones(sc.N, dtype=np.int32), normal=np.zeros((sc.N, 3)))
        pc = ref["pc"]
        q["prim"][pc["particle"]] = pc["prim"]
        q["normal"][pc["particle"]] = pc["normal"]
        q["normal"] = q["normal"].reshape(-1)
        q["self"] = None
        recs.append(q)
    records.upload_oracle_records(e, s + 1, recs)


# ---- static sphere; moving and spinning sphere ----
@pytest.mark.parametrize("name", ["static", "moving_spinning"])
def test_sphere_against_the_oracle_own_steps_and_handed_in_records(name):
    sc, e, out = run_scene(name)
    c = sc.census()
    assert c["takeoff"] >= 1 and c["stick"] >= 5 and c["slide"] >= 5
    # the oracle's record handed in: every contact outside the fp32 margin has the oracle's type, the counts are the oracle's
    for s in range(sc.steps):
        hand_in_oracle_records(sc, e, s)
        got = e.contact_readout(s + 1, 1)
        for b in range(sc.nb):
            ex = sc.expected(s, b)
            sel = ex["safe_record"]
            np.testing.assert_array_equal(got["state"][0, b][sel], ex["state"][sel], err_msg=f"step {s} rollout {b}")
            if sel.all():
                np.testing.assert_array_equal(got["wrench"][0, b][:, 7:10], ex["rows"][:, 7:10])
            assert np.all(np.abs(got["normal_impulse"][0, b] - ex["jn"]) <= cs.GATE_R * ex["dnorm"])
            for g in range(sc.G):
                assert np.linalg.norm(got["wrench"][0, b, g, 0:3] - ex["rows"][g, 0:3]) <= cs.SUM_RTOL * ex["scales"][g, 0]
                assert np.linalg.norm(got["wrench"][0, b, g, 3:6] - ex["rows"][g, 3:6]) <= cs.SUM_RTOL * ex["scales"][g, 1]
    e.close()


def test_per_rollout_mu():
    sc, e, out = run_scene("mu")
    counts = out["wrench"][:, :, 0, 7:10].sum(axis=0)           # [rollout][take-off, stick, slide] over the steps
    assert counts[0, 1] < counts[1, 1] and counts[0, 2] > counts[1, 2], counts
    # mu is the context's CURRENT value: the same records read with the two values swapped give the other decision where it matters
    e.set_mu(sc.mu[::-1].copy())
    swapped = e.contact_readout(1, 1)
    assert np.all(swapped["state"][0, 0][out["state"][0, 0] != 0] >= 2) and np.any(swapped["state"][0, 0] != out["state"][0, 0])
    e.close()


def test_primitive_part_under_self_contact():
    """the folded flap lying on the sphere: the layered passes added the self-contact response to the stored r at vertices that are in both kinds of
    contact; J is the oracle's sum over prim_contacts, which the record's total r over the same vertices misses"""
    sc = cs.scene("flap")
    e = make_engine(sc)
    prepare(sc, e)
    out = run_steps(sc, e)
    lines = []
    seen = 0
    try:
        check(sc, e, out, lines, self_contacts=True)
        for s in range(sc.steps):
            ref = sc.ref[s][0]
            pc = ref["pc"]
            assert ref["nself"] >= 10 and len(pc["particle"]) >= 5
            gate = cs.SUM_RTOL * np.linalg.norm(pc["r"], axis=1).sum()
            total_o = -ref["r"].reshape(-1, 3)[pc["particle"]].sum(axis=0)
            miss_o = np.linalg.norm(total_o + pc["r"].sum(axis=0))
            total_e = -e.get_record(s + 1)[1][0].reshape(-1, 3)[pc["particle"]].sum(axis=0)
            miss_e = np.linalg.norm(total_e - out["wrench"][s, 0, 0, 0:3])
            lines.append(f"step {s}: sum of the record's TOTAL r over the contact vertices misses the primitive part by {miss_o:.2e} (oracle) {miss_e:.2e} (engine), gate {gate:.2e}")
            if miss_o > 100 * gate:
                seen += 1
                assert miss_e > 100 * gate, lines[-1]
    finally:
        print("\n[contact read-out, flap on the sphere]\n" + "\n".join(lines))
    assert seen >= 1, "no step in which the self-contact layers changed r at the primitive contacts by 100 gates"
    e.close()


# ---- kinds and groups ----
def test_three_groups_one_out_of_reach():
    sc, e, out = run_scene("three_groups")
    assert np.all(out["wrench"][:, :, 1, :] == 0) and np.all(out["wrench"][:, :, 0, 7:10].sum(axis=-1) >= 5) and np.all(out["wrench"][:, :, 2, 7:10].sum(axis=-1) >= 5)
    e.close()


def test_offset_schedule_moves_the_reference_point():
    sc, e, out = run_scene("offset_schedule")
    lines = []
    built = f32(np.asarray(sc.prims[0]["center"]))
    for s in range(1, sc.steps):
        for b in range(sc.nb):
            ex, wrong = sc.expected(s, b), sc.expected(s, b, centre=[built])
            miss = np.linalg.norm(out["wrench"][s, b, 0, 3:6] - wrong["rows"][0, 3:6])
            lines.append(f"step {s} rollout {b}: tau about the BUILT centre would be off by {miss:.2e}, gate {cs.SUM_RTOL * ex['scales'][0, 1]:.2e}")
            assert np.linalg.norm(wrong["rows"][0, 3:6] - ex["rows"][0, 3:6]) > 100 * cs.SUM_RTOL * ex["scales"][0, 1], lines[-1]      # on the oracle alone
            assert miss > 100 * cs.SUM_RTOL * ex["scales"][0, 1], lines[-1]
    print("\n".join(lines))
    e.close()


@pytest.mark.parametrize("name", ["plane", "capsule", "bowl", "discretised_sphere"])
def test_other_kinds(name):
    sc, e, out = run_scene(name)
    assert sc.census()["contacts"] >= 20
    e.close()


def test_lower_leg_torque_is_about_its_first_childs_centre():
    """one group of three flattened primitives (joint sphere, foot capsule, leg capsule): the oracle reports ONE primitive; tau is about the centre
    of the first child, which is not the collection's centre"""
    sc, e, out = run_scene("lower_leg")
    assert e.ngroups == 1 and len(sc.prims) == 3
    first = f32(np.asarray(sc.prims[0]["center"]))
    np.testing.assert_array_equal(e.get_primitive_centers(1)[:, 0], np.tile(first, (sc.nb, 1)))
    collection = first - f32(np.asarray(sc.prims[0]["center"]) - np.asarray(sc.prims[1]["center"]))      # the foot capsule's centre = the LowerLeg's own
    assert np.linalg.norm(collection - first) > 1.0
    for b in range(sc.nb):
        ex, wrong = sc.expected(0, b), sc.expected(0, b, centre=[collection])
        gate = cs.SUM_RTOL * ex["scales"][0, 1]
        assert ex["rows"][0, 7:10].sum() >= 10
        assert np.linalg.norm(wrong["rows"][0, 3:6] - ex["rows"][0, 3:6]) > 100 * gate          # on the oracle alone
        assert np.linalg.norm(out["wrench"][0, b, 0, 3:6] - wrong["rows"][0, 3:6]) > 100 * gate
    e.close()


# ---- bit for bit ----
def test_bit_for_bit_forms_ranges_repeats_sweeps_and_handed_in_records():
    sc = cs.scene("static")
    e = make_engine(sc)
    prepare(sc, e)
    run_steps(sc, e)
    S, B, N, G = sc.steps, sc.nb, sc.N, sc.G
    host = e.contact_readout(1, S)
    again = e.contact_readout(1, S)
    for k in host:
        np.testing.assert_array_equal(host[k], again[k])
    for s in range(S):                                              # a whole range = per-slot calls
        one = e.contact_readout(s + 1, 1)
        for k in host:
            np.testing.assert_array_equal(host[k][s], one[k][0])
    only = e.contact_readout(2, 1, state=False, normal_impulse=False)          # each output alone
    assert only["state"] is None and only["normal_impulse"] is None
    np.testing.assert_array_equal(only["wrench"][0], host["wrench"][1])
    np.testing.assert_array_equal(e.contact_readout(2, 1, wrench=False, normal_impulse=False)["state"][0], host["state"][1])
    np.testing.assert_array_equal(e.contact_readout(2, 1, wrench=False, state=False)["normal_impulse"][0], host["normal_impulse"][1])
    dev = torch.device("cuda", 0)
    for dtype in (torch.float64, torch.float32):
        st = torch.full((S, B, N), -7, dtype=torch.int32, device=dev)
        jn = torch.full((S, B, N), -7.0, dtype=dtype, device=dev)
        wide = torch.full((S * B * G * 10 + 1,), -7.0, dtype=dtype, device=dev)
        wr = wide[1:].view(S, B, G, 10)                             # an output view that is not 16-byte aligned
        e.contact_readout_dev(1, S, st, jn, wr)
        e.sync()
        np.testing.assert_array_equal(st.cpu().numpy(), host["state"])
        cast = (lambda a: a) if dtype == torch.float64 else (lambda a: a.astype(np.float32))
        np.testing.assert_array_equal(jn.cpu().numpy(), cast(host["normal_impulse"]))
        np.testing.assert_array_equal(wr.cpu().numpy(), cast(host["wrench"]))
        assert float(wide[0]) == -7.0
    # the engine's own record read back and handed in again: the same read-out
    s = 1
    x, v = e.get_state(s + 1)
    f, r = e.get_record(s + 1)
    grp, nrm = e.get_contacts(s + 1)
    e.set_record(s + 1, x, v, f, grp, nrm, r=r)                      # (one primitive: group id = primitive index)
    back = e.contact_readout(s + 1, 1)
    for k in host:
        np.testing.assert_array_equal(back[k][0], host[k][s])
    # records of a fused sweep = records of per-step calls (free running from the first state)
    e.clear_schedules()
    e.set_primitive_offsets(sc.D[0])
    for fused in (False, True):
        e.set_state(0, sc.Xe[0], sc.Ve[0])
        if fused:
            e.rollout_forward(0, S)
            b_ = e.contact_readout(1, S)
        else:
            for k in range(S):
                e.step_forward(k)
            a_ = e.contact_readout(1, S)
    for k in host:
        np.testing.assert_array_equal(a_[k], b_[k])
    assert np.any(a_["state"][S - 1] != 0)
    e.close()


def test_odd_vertex_count_and_renumbered_mesh():
    """289 vertices (n % 4 = 1) throughout; here the same grid with permuted vertex ids, which the engine renumbers: per-vertex outputs arrive in
    the CALLER's ids"""
    sc = cs.scene("static")
    assert sc.N % 4 != 0
    rng = np.random.default_rng(9)
    perm = rng.permutation(sc.N)                   # new id k holds old vertex perm[k]
    inv = np.argsort(perm)
    Vp, Fp = sc.V[perm], inv[sc.F]
    e = make_engine(sc, Vp, Fp)
    assert e.layout()["renumbered"]
    prepare(sc, e)
    p3 = (3 * perm[:, None] + np.arange(3)).reshape(-1)
    for s in range(sc.steps):
        e.set_state(s, sc.Xe[s][:, p3], sc.Ve[s][:, p3])
        e.step_forward(s)
    out = e.contact_readout(1, sc.steps)
    grp = np.stack([e.get_contacts(s + 1)[0] for s in range(sc.steps)])
    r = np.stack([e.get_record(s + 1)[1] for s in range(sc.steps)]).reshape(sc.steps, sc.nb, sc.N, 3)
    nrm = np.stack([e.get_contacts(s + 1)[1] for s in range(sc.steps)]).reshape(sc.steps, sc.nb, sc.N, 3)
    np.testing.assert_array_equal(out["state"] != 0, grp >= 0)
    rn = np.einsum("sbkd,sbkd->sbk", r, nrm)
    assert np.all(np.abs(out["normal_impulse"] - rn) <= REEVAL * np.linalg.norm(r, axis=-1))
    for s in range(sc.steps):
        for b in range(sc.nb):
            ex = sc.expected(s, b)
            np.testing.assert_array_equal(out["state"][s, b] != 0, ex["state"][perm] != 0)
            sel = ex["safe_step"][perm]
            np.testing.assert_array_equal(out["state"][s, b][sel], ex["state"][perm][sel])
            assert np.all(np.abs(out["normal_impulse"][s, b] - ex["jn"][perm]) <= cs.GATE_R * ex["dnorm"][perm])
            assert np.linalg.norm(out["wrench"][s, b, 0, 3:6] - ex["rows"][0, 3:6]) <= cs.SUM_RTOL * ex["scales"][0, 1]
    e.close()


# ---- other kernels' records ----
@pytest.mark.parametrize("cluster", [2, 4])
def test_split_kernels_records(cluster, monkeypatch):
    monkeypatch.setenv("DC_CLUSTER", str(cluster))
    sc = cs.scene("split")
    e = make_engine(sc)
    prepare(sc, e)
    assert e.cluster() == cluster
    out = run_steps(sc, e)
    lines = []
    try:
        check(sc, e, out, lines)
    finally:
        print(f"\n[contact read-out, 29 x 29, K = {cluster}]\n" + "\n".join(lines))
    e.close()


@pytest.mark.parametrize("name", ["DC_DENSE_MAX_N", "DC_WINDOWS"])
def test_kernel_families_selected_at_build(name, monkeypatch):
    monkeypatch.setenv(name, "0")
    sc = cs.scene("static")
    e = make_engine(sc)
    lay = e.layout()
    assert not (lay["dense_inverse"] if name == "DC_DENSE_MAX_N" else lay["element_windows"])
    e.close()
    run_scene("static")[1].close()


def test_global_memory_forward_family():
    """DC_FWD_VARIANT is read once per process by the launchers: the static scene in a child process"""
    env = dict(os.environ)
    env["DC_FWD_VARIANT"] = "global"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k", "test_three_groups_one_out_of_reach"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0, f"{tail}\n{r.stderr[-2000:]}"
    assert "1 passed" in tail and "failed" not in tail, tail


# ---- torch ----
def test_batched_sim_contact_readout_after_sim_step_and_sim_rollout(monkeypatch):
    sc = cs.scene("static")
    e = make_engine(sc)
    S, B = sc.steps, sc.nb
    prepare(sc, e)
    sim = BatchedSim(e, S)
    dev = torch.device("cuda", 0)
    syncs = []
    real_sync = capi.Engine.sync
    monkeypatch.setattr(capi.Engine, "sync", lambda self: (syncs.append(1), real_sync(self))[1])
    side = torch.cuda.Stream(device=dev)
    a = torch.zeros((B, 0), device=dev)
    with torch.cuda.stream(side):
        x = torch.as_tensor(sc.Xe[0], dtype=torch.float32, device=dev)
        v = torch.as_tensor(sc.Ve[0], dtype=torch.float32, device=dev)
        for s in range(S):
            x, v = sim_step(sim, x, v, a)
        n0 = len(syncs)
        got = sim.contact_readout()
        got64 = sim.contact_readout(2, 1, dtype=torch.float64)
        assert len(syncs) == n0                                     # nothing on the path synchronises
    side.synchronize()
    host = e.contact_readout(1, S)
    assert got["state"].dtype == torch.int32 and got["state"].shape == (S, B, sc.N) and got["wrench"].shape == (S, B, sc.G, 10)
    for k in host:
        assert got[k].is_cuda and not got[k].requires_grad
        np.testing.assert_array_equal(got[k].cpu().numpy(), host[k].astype(got[k].cpu().numpy().dtype))
        np.testing.assert_array_equal(got64[k].cpu().numpy()[0], host[k][1])
    assert np.any(host["state"] != 0)
    # after a sim_rollout forward pass
    with torch.cuda.stream(side):
        x0 = torch.as_tensor(sc.Xe[0], dtype=torch.float32, device=dev).requires_grad_(True)
        v0 = torch.as_tensor(sc.Ve[0], dtype=torch.float32, device=dev)
        xs, vs = sim_rollout(sim, x0, v0, None, steps=S, primitive_offsets=torch.as_tensor(sc.D, dtype=torch.float32, device=dev))
        n0 = len(syncs)
        roll = sim.contact_readout(1)
        assert len(syncs) == n0
    side.synchronize()
    host = e.contact_readout(1, S)
    for k in host:
        assert not roll[k].requires_grad
        np.testing.assert_array_equal(roll[k].cpu().numpy(), host[k].astype(roll[k].cpu().numpy().dtype))
    assert np.any(host["state"] != 0)
    with pytest.raises(ValueError, match="step"):
        sim.contact_readout(1, S + 1)
    e.close()


# ---- refusals, on a device context ----
def test_refusals():
    sc = cs.scene("static")
    e = make_engine(sc)
    e.alloc_batch(2, 3)
    lib, h = e.lib, e.h
    import ctypes as C
    buf = np.zeros(2 * 3 * sc.N * 10)
    p = C.c_void_p(buf.ctypes.data)
    i = C.c_int
    for args, msg in (((i(0), i(1), p, p, p), "slot 0"), ((i(1), i(0), p, p, p), "nslots"), ((i(2), i(3), p, p, p), "past the tape"),
                      ((i(1), i(1), None, None, None), "all null")):
        for name, extra in (("dc_get_contact_readout", ()), ("dc_get_contact_readout_dev", (i(0),))):
            assert getattr(lib, name)(h, *args, *extra) == 1, (name, msg)           # DC_ERR_INVALID
            assert msg in lib.dc_last_error(h).decode(), (name, lib.dc_last_error(h))
    assert np.all(buf == 0)
    e.close()
    e = pv.make_engine(sc.V, sc.F, [])
    e.alloc_batch(1, 1)
    e.set_state(0, sc.Xe[0][:1], sc.Ve[0][:1])
    e.step_forward(0)
    with pytest.raises(capi.DcError, match="no primitive group"):
        e.contact_readout(1, 1)
    out = e.contact_readout(1, 1, wrench=False)                    # the per-vertex outputs of a scene without primitives: zeros
    assert np.all(out["state"] == 0) and np.all(out["normal_impulse"] == 0)
    e.close()
