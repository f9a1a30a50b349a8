"""Gradients of a loss on the contact read-out (dc_set_contact_readout_gradients[_dev], Engine.set_contact_readout_gradients[_dev],
sim_rollout(contact_readout=True)) against the fp64 model of tests/readout_grad_model.py, which tests/test_readout_grad_model.py holds to
central differences of the oracle.

Same record on both sides, both directions (tests/records.py): the oracle's record handed in with dc_set_record, and the oracle adopting the
engine's own record. Gate: records.rel <= 1e-4, the project's flat same-record gate; sums over a group or over the vertices use the SUM_RTOL
rule of tests/contact_readout_scenes.py (|diff| <= 1e-4 x the sum of the terms' magnitudes). A contact whose decision the engine reports
differently from the oracle (inside MARGIN_RECORD of a boundary of the friction law) takes the engine's reported case in the model's terms."""
import contextlib
import os

import numpy as np
import pytest
import torch          # before the engine's library: both must share ONE HIP runtime (torch's), see tests/test_gpu_functional.py

import contact_readout_scenes as cs
import readout_grad_scenes as gs
import records
import test_gpu_contact_readout as cr
from diffcloth_amd import capi
from diffcloth_amd.functional import BatchedSim, sim_rollout

pytestmark = pytest.mark.gpu
H, f32, rel = cs.H, cs.f32, records.rel
GATE = 1e-4
ARRAYS = ("dL_dx", "dL_dv", "dL_dfext_vec")


@contextlib.contextmanager
def cluster_env(k):
    old = os.environ.get("DC_CLUSTER")
    os.environ["DC_CLUSTER"] = str(k)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("DC_CLUSTER", None)
        else:
            os.environ["DC_CLUSTER"] = old


def engine_for(S, mode=1, cluster=None):
    sc = S.sc
    e = cr.pv.make_engine(sc.V, sc.F, sc.prims, att=sc.att, mode=mode, selfcollision=int(sc.selfcollision), fabric=sc.fabric)
    if cluster is None:
        cr.prepare(sc, e)
    else:
        with cluster_env(cluster):
            cr.prepare(sc, e)
        assert e.cluster() == cluster
    return e


def hand_in(S, e, s):
    """state s and the oracle's record s + 1 (with its motion row, for a moving scene) on the engine"""
    sc = S.sc
    e.set_state(s, sc.Xe[s], sc.Ve[s])
    records.upload_oracle_records(e, s + 1, S.oracle_records(s), x_fixed=None if sc.XF is None else sc.XF[s])
    if np.abs(sc.W).max() > 0:
        e.set_primitive_velocity_schedule(s, sc.W[None])
    if np.abs(cr.spins_of(sc)).max() > 0:
        e.set_primitive_spin_schedule(s, cr.spins_of(sc)[None])


def sum_gate(diff, terms):
    return np.linalg.norm(diff) <= cs.SUM_RTOL * np.linalg.norm(np.asarray(terms).reshape(-1, 3), axis=1).sum()


def compare_step(S, e, s, gb, fg, pg, lines, is_start, weights=True, param_rows=True, tag=""):
    """one backward step of every rollout against the model; returns the worst relative error of the arrays"""
    sc = S.sc
    state = e.contact_readout(s + 1, 1, normal_impulse=False, wrench=False)["state"][0]
    worst = 0.0
    for b in range(sc.nb):
        want = S.backward(s, b, S.gx[s, b], S.gv[s, b], ix=S.ix[s, b], iv=S.iv[s, b], is_start=is_start, weights=weights, state=state[b])
        t = want["terms"]
        unsafe = int(np.sum((t["case"] != 0) & ~sc.safe(s, b, cs.MARGIN_RECORD)))
        adopted = t["case"] != t["own_case"]
        # a case taken from the engine is a contact inside the margin of a boundary of the law; everywhere else the engine decides as the oracle
        assert not np.any(adopted & sc.safe(s, b, cs.MARGIN_RECORD)), (s, b, np.nonzero(adopted)[0])
        got = dict(dL_dx=gb["dL_dx"][b], dL_dv=gb["dL_dv"][b], dL_dfext_vec=fg[b])
        errs = {k: rel(got[k], want[k]) for k in ARRAYS}
        part = {k: rel(want[k], want["plain"][k]) for k in ARRAYS}
        emu = records.mu_err(gb["dL_dmu"][b], want["dL_dmu"])
        lines.append(f"{tag}step {s} rollout {b} is_start {int(is_start)}: " + " ".join(f"{k} {v:.2e} (read-out's part {part[k]:.1e})" for k, v in errs.items()) +
                     f" dL_dmu {emu:.2e} [{gb['dL_dmu'][b]} / {want['dL_dmu']}] cases {np.bincount(t['case'], minlength=4)[1:]} inside the margin {unsafe}")
        assert max(errs.values()) <= GATE and emu <= GATE, lines[-1]
        assert np.all(gb["converged"] >= 1)
        worst = max(worst, max(errs.values()))
        if len(sc.att):
            exf = rel(gb["dL_dxfixed"][b], want["dL_dxfixed"])
            pxf = rel(want["dL_dxfixed"], want["plain"]["dL_dxfixed"])
            lines.append(f"    dL_dxfixed {exf:.2e} (read-out's part {pxf:.1e})")
            assert exf <= GATE, lines[-1]
        if param_rows:
            ek = rel(pg["dL_dk"][b][[0, 1]], want["dL_dk"][[0, 1]])
            if len(sc.att):       # dL/dk_att on its own, a sum over the attachments of h^2 (x_fixed - x_new) . y~: the SUM_RTOL rule on its terms
                a3 = (3 * np.asarray(sc.att)[:, None] + np.arange(3)).reshape(-1)
                terms = (sc.XF[s, b] - sc.ref[s][b]["x"][a3]) * want["dL_dxfixed"] / S.oracles[b].params["k_att"]
                ea = abs(pg["dL_dk"][b][2] - want["dL_dk"][2])
                lines.append(f"    dL/dk_att {pg['dL_dk'][b][2]:+.6e} model {want['dL_dk'][2]:+.6e} without the read-out's part {want['plain']['dL_dk'][2]:+.2e} "
                             f"|diff| {ea:.2e} / {np.abs(terms.reshape(-1, 3).sum(axis=1)).sum():.2e}")
                assert ea <= cs.SUM_RTOL * np.abs(terms.reshape(-1, 3).sum(axis=1)).sum(), lines[-1]
            ed = abs(pg["dL_ddensity"][b] - want["dL_ddensity"]) / max(abs(want["dL_ddensity"]), 1e-30)
            sf = want["dL_dfext_vec"].reshape(-1, 3)
            lines.append(f"    d_param: dL_dk {ek:.2e} dL_ddensity {ed:.2e} sum_dfext {pg['sum_dfext'][b]} / {sf.sum(axis=0)}")
            assert ek <= GATE and ed <= GATE, lines[-1]
            assert sum_gate(pg["sum_dfext"][b] - sf.sum(axis=0), sf), lines[-1]
    return worst


def run_handed_in(name, mode=1, cluster=None, weights=True, steps=None, param_rows=True):
    S = gs.scene(name)
    sc = S.sc
    e = engine_for(S, mode, cluster)
    lines = []
    try:
        for s in range(sc.steps if steps is None else steps):
            hand_in(S, e, s)
            e.set_contact_readout_gradients(1, None, None)          # the record under test alone carries weights (the one below would add its part to dL_dx)
            if weights:
                e.set_contact_readout_gradients(s + 1, S.wj[s][None], S.ww[s][None])
            is_start = s % 2 == 0
            gb = e.step_backward(s + 1, S.gx[s], S.gv[s], S.ix[s], S.iv[s], is_start=is_start)
            compare_step(S, e, s, gb, e.get_force_gradient(), e.get_param_gradients(s + 1), lines, is_start, weights, param_rows, tag=f"[{name} mode {mode}] ")
    finally:
        print("\n" + "\n".join(lines))
    return S, e


# ---- same record: the oracle's, handed in ----
@pytest.mark.parametrize("name,mode", [("static", 0), ("static", 1), ("static", 2), ("static", 3), ("mu", 1)])
def test_oracle_records_handed_in(name, mode):
    S, e = run_handed_in(name, mode)
    e.close()


def test_the_term_matters():
    """on the model alone the read-out's part is at least 100 gates of every compared array; and the engine without weights misses by that"""
    S = gs.scene("static")
    sc = S.sc
    for s in range(sc.steps):
        for b in range(sc.nb):
            want = S.backward(s, b, S.gx[s, b], S.gv[s, b], ix=S.ix[s, b], iv=S.iv[s, b])
            for k in ARRAYS:
                assert rel(want[k], want["plain"][k]) >= 100 * GATE, (s, b, k)
            assert records.mu_err(want["plain"]["dL_dmu"], want["dL_dmu"]) >= 100 * GATE
    e = engine_for(S)
    hand_in(S, e, 0)
    gb = e.step_backward(1, S.gx[0], S.gv[0], S.ix[0], S.iv[0], is_start=True)
    fg = e.get_force_gradient()
    for b in range(sc.nb):
        want = S.backward(0, b, S.gx[0, b], S.gv[0, b], ix=S.ix[0, b], iv=S.iv[0, b], is_start=True)
        got = dict(dL_dx=gb["dL_dx"][b], dL_dv=gb["dL_dv"][b], dL_dfext_vec=fg[b])
        for k in ARRAYS:
            assert rel(got[k], want[k]) >= 100 * GATE and rel(got[k], want["plain"][k]) <= GATE, (b, k)
    e.close()


# ---- further same-record scenes ----
@pytest.mark.parametrize("name", ["flap", "three_groups", "capsule", "offset_schedule", "clipped"])
def test_further_scenes(name):
    S, e = run_handed_in(name, param_rows=name != "flap")
    sc = S.sc
    if name == "clipped":               # two clipped vertices in stick / slide contact: the attachment terms (dL_dxfixed, dL/dk_att, the seed's operator)
        for s in range(sc.steps):
            for b in range(sc.nb):
                want = S.backward(s, b, S.gx[s, b], S.gv[s, b], ix=S.ix[s, b], iv=S.iv[s, b])
                assert np.any(want["terms"]["case"][list(sc.att)] >= 2), (s, b)
                assert rel(want["dL_dxfixed"], want["plain"]["dL_dxfixed"]) >= 100 * GATE, (s, b)      # the term matters, on the model alone
        hand_in(S, e, 0)                # ... and the engine without weights misses dL_dxfixed by that
        e.set_contact_readout_gradients(1, None, None)
        gb = e.step_backward(1, S.gx[0], S.gv[0], S.ix[0], S.iv[0], is_start=True)
        for b in range(sc.nb):
            want = S.backward(0, b, S.gx[0, b], S.gv[0, b], ix=S.ix[0, b], iv=S.iv[0, b], is_start=True)
            assert rel(gb["dL_dxfixed"][b], want["dL_dxfixed"]) >= 100 * GATE and rel(gb["dL_dxfixed"][b], want["plain"]["dL_dxfixed"]) <= GATE, b
    if name == "three_groups":          # the group out of reach: its weights move nothing, its dL_dmu is exactly zero
        hand_in(S, e, 0)
        ww = S.ww[0].copy()
        e.set_contact_readout_gradients(1, S.wj[0][None], ww[None])
        a = e.step_backward(1, S.gx[0], S.gv[0], is_start=True)
        ww[:, 1] = 1e6
        e.set_contact_readout_gradients(1, S.wj[0][None], ww[None])
        b = e.step_backward(1, S.gx[0], S.gv[0], is_start=True)
        for k in ("dL_dx", "dL_dv", "dL_dmu"):
            np.testing.assert_array_equal(a[k], b[k])
        assert np.all(a["dL_dmu"][:, 1] == 0.0)
    if name == "flap":
        assert all(sc.ref[s][0]["nself"] >= 10 for s in range(sc.steps))
    e.close()


def test_moving_and_spinning_obstacle_gradients():
    S = gs.scene("moving_spinning")
    sc = S.sc
    e = engine_for(S)
    lines = []
    try:
        for s in range(sc.steps):
            hand_in(S, e, s)
            e.set_contact_readout_gradients(1, None, None)          # the record under test alone carries weights
            e.set_contact_readout_gradients(s + 1, S.wj[s][None], S.ww[s][None])
            gb = e.step_backward(s + 1, S.gx[s], S.gv[s], is_start=True)
            dw, dom = e.get_primitive_velocity_gradients(s + 1, 1)[0], e.get_primitive_spin_gradients(s + 1, 1)[0]
            state = e.contact_readout(s + 1, 1, normal_impulse=False, wrench=False)["state"][0]
            for b in range(sc.nb):
                t, ww = S.terms(s, b, state=state[b])
                o = S.oracles[b]
                rows, scale = gs.model.motion_gradients(o, S.rid[s][b], S.gx[s, b], S.gv[s, b], t, ww, S.radius)
                plain = np.abs(t["motion"]).max()
                for g in range(sc.G):
                    ew, eo = np.linalg.norm(dw[b, g] - rows[g, 0:3]), np.linalg.norm(dom[b, g] - rows[g, 3:6])
                    lines.append(f"step {s} rollout {b} group {g}: dL/dw {dw[b, g]} model {rows[g, 0:3]} |diff| {ew:.2e} / {scale[g, 0]:.2e}; dL/domega {dom[b, g]} "
                                 f"model {rows[g, 3:6]} |diff| {eo:.2e} / {scale[g, 1]:.2e}; the read-out's part up to {plain:.2e}")
                    assert ew <= cs.SUM_RTOL * scale[g, 0] and eo <= cs.SUM_RTOL * scale[g, 1], lines[-1]
                    assert plain >= 100 * cs.SUM_RTOL * scale[g, 0], lines[-1]
                want = S.backward(s, b, S.gx[s, b], S.gv[s, b], is_start=True, state=state[b])
                for k in ("dL_dx", "dL_dv"):
                    assert rel(gb[k][b], want[k]) <= GATE, (s, b, k, rel(gb[k][b], want[k]))
    finally:
        print("\n" + "\n".join(lines))
    e.close()


# ---- the engine's own records, a fused sweep: the production path ----
def own_records(S, e):
    """the engine's own teacher-forced steps; every oracle adopts the engine's record of its steps. Returns the tape's states per slot."""
    sc = S.sc
    for s in range(sc.steps):
        e.set_state(s, sc.Xe[s], sc.Ve[s])
        st = e.step_forward(s, fixed_pts=None if sc.XF is None else sc.XF[s])
        assert np.all(st["converged"] == 1)
    xs, vs = e.get_states(0, sc.steps + 1)
    for s in range(sc.steps):
        f = e.get_record(s + 1)[0]
        grp, nrm = e.get_contacts(s + 1)
        for b in range(sc.nb):
            pc = sc.ref[s][b]["pc"]
            np.testing.assert_array_equal(np.nonzero(grp[b] >= 0)[0], np.sort(pc["particle"]))          # the same contact set
            S.primitives_at(S.oracles[b], s, b)
            records.oracle_adopts_gpu_record(S.oracles[b], S.rid[s][b], e, s + 1, b, xs[s, b], xs[s + 1, b], vs[s + 1, b], f[b], H, normals=nrm)
    return xs, vs


def restore_oracle_records(S):
    sc = S.sc
    for s in range(sc.steps):
        for b in range(sc.nb):
            S.oracles[b].override_record(S.rid[s][b], x=sc.ref[s][b]["x"], f=sc.ref[s][b]["f"])


def sweep(S, e, weights=True, dev=None, keep=True, upload=True):
    """seed schedule (upload = False: what the context holds), carried gradient, weights, ONE backward sweep over all steps; everything it leaves"""
    sc = S.sc
    T = sc.steps
    e.keep_force_gradients(keep)
    if upload:
        e.set_seed_schedule(0, np.concatenate([np.zeros((1, sc.nb, 3 * sc.N)), S.ix[1:T]]), np.concatenate([np.zeros((1, sc.nb, 3 * sc.N)), S.iv[1:T]]))
    e.set_gradient(S.gx[T - 1], S.gv[T - 1])
    if weights == "zero":
        e.set_contact_readout_gradients(1, np.zeros_like(S.wj[:T]), np.zeros_like(S.ww[:T]))
    elif weights and dev is None:
        e.set_contact_readout_gradients(1, S.wj[:T], S.ww[:T])
    elif weights:
        e.set_contact_readout_gradients_dev(1, T, *dev)
    e.rollout_backward(T, T)
    dx, dv, dmu = e.get_gradient()
    out = dict(dx=dx, dv=dv, dmu=dmu, par=np.stack([np.concatenate([v for v in e.get_param_gradients(s).values()], axis=None) for s in range(1, T + 1)]))
    if keep:
        out["fg"] = e.get_force_gradients(1, T)
    return out


def model_chain(S, x_top, weights=True, state=None):
    """the same sweep on the model: the carried gradient handed down step by step, dL_dmu accumulated"""
    sc = S.sc
    T = sc.steps
    out = []
    for b in range(sc.nb):
        gx, gv, dmu = S.gx[T - 1, b], S.gv[T - 1, b], 0.0
        for s in range(T - 1, -1, -1):
            z = np.zeros(3 * sc.N)
            r = S.backward(s, b, gx, gv, ix=S.ix[s, b] if s else z, iv=S.iv[s, b] if s else z, is_start=(s == 0), weights=weights,
                           state=None if state is None else state[s, b], x=x_top[b] if s == T - 1 else None)
            gx, gv, dmu = r["dL_dx"], r["dL_dv"], dmu + r["dL_dmu"]
        out.append(dict(dx=gx, dv=gv, dmu=dmu))
    return out


def test_own_records_fused_sweep_and_its_invariants():
    S = gs.scene("static")
    sc = S.sc
    T = sc.steps
    e = engine_for(S)
    lines = []
    try:
        xs, vs = own_records(S, e)
        state = e.contact_readout(1, T, normal_impulse=False, wrench=False)["state"]
        # the last slot holds the engine's own state, not the oracle's: the torque arm of the last record is taken there
        x_top = [xs[T, b] - np.tile(sc.W[b, 0], sc.N) * H for b in range(sc.nb)]
        e.kernel_times(reset=True)
        never = sweep(S, e, weights=False)
        plain_launches = e.kernel_times(reset=True)["bwd_launches"]
        got = sweep(S, e)
        launches = e.kernel_times(reset=True)["bwd_launches"]
        assert plain_launches == 1 and launches == 3, (plain_launches, launches)      # the plain sweep enqueues no kernel of the read-out's
        want, plain = model_chain(S, x_top, state=state), model_chain(S, x_top, weights=False)
        for b in range(sc.nb):
            ex, ev, em = rel(got["dx"][b], want[b]["dx"]), rel(got["dv"][b], want[b]["dv"]), records.mu_err(got["dmu"][b], want[b]["dmu"])
            px, pv_ = rel(plain[b]["dx"], want[b]["dx"]), rel(plain[b]["dv"], want[b]["dv"])
            lines.append(f"fused sweep over the engine's own records, rollout {b}: dL_dx {ex:.2e} dL_dv {ev:.2e} dL_dmu {em:.2e} (the read-out's part: {px:.1e}, {pv_:.1e}); "
                         f"without weights against the plain model {rel(never['dx'][b], plain[b]['dx']):.2e}")
            assert max(ex, ev, em) <= GATE, lines[-1]
            assert min(px, pv_) >= 100 * GATE and rel(never["dx"][b], plain[b]["dx"]) <= GATE, lines[-1]
        # the same sweep twice: the same bits
        again = sweep(S, e)
        for k in got:
            np.testing.assert_array_equal(got[k], again[k], err_msg=k)
        # the caller's schedule is never written: after two seeded sweeps the schedule the context HOLDS (not uploaded again) gives the plain sweep
        e.set_contact_readout_gradients(1, None, None)
        kept = sweep(S, e, weights=False, upload=False)
        for k in never:
            np.testing.assert_array_equal(never[k], kept[k], err_msg=k)
        # zeros, never set and cleared: the same gradients
        zero = sweep(S, e, weights="zero")
        e.set_contact_readout_gradients(1, None, None)
        cleared = sweep(S, e, weights=False)
        e.set_contact_readout_gradients(1, S.wj[:T], S.ww[:T])
        e.clear_schedules()
        cleared2 = sweep(S, e, weights=False)
        for k in never:
            assert np.array_equal(never[k], zero[k]) and np.array_equal(never[k], cleared[k]) and np.array_equal(never[k], cleared2[k]), k
        # weights on SOME records only
        e.set_contact_readout_gradients(2, S.wj[1:2], S.ww[1:2])
        some = sweep(S, e, weights=False)
        assert not np.array_equal(some["dx"], never["dx"])
        e.set_contact_readout_gradients(1, None, None)
        # host form = device form in fp64; in fp32 up to the cast; an unaligned device view
        dev = torch.device("cuda", 0)
        e.sync()
        j64, w64 = torch.as_tensor(S.wj[:T], device=dev), torch.as_tensor(S.ww[:T], device=dev)
        d64 = sweep(S, e, dev=(j64, w64))
        for k in got:
            np.testing.assert_array_equal(got[k], d64[k], err_msg=k)
        d32 = sweep(S, e, dev=(j64.float(), w64.float()))          # (the weights are fp32 values already)
        pad = torch.zeros(j64.numel() + 1, dtype=torch.float32, device=dev)
        pad[1:] = j64.float().reshape(-1)
        view = sweep(S, e, dev=(pad[1:].reshape(j64.shape), w64.float()))
        for k in got:
            np.testing.assert_array_equal(got[k], d32[k], err_msg=k)
            np.testing.assert_array_equal(got[k], view[k], err_msg=k)
        e.set_contact_readout_gradients(1, None, None)
        # the fused 3-step sweep equals per-step calls handing dL_dx / dL_dv on, bit for bit: state gradients, the parameter rows and the force
        # gradients of every record (dL_dmu: the sweep accumulates it in fp32 on the device, the calls return it per step — the gate)
        for chain in ("step_backward", "one-step sweeps"):
            e.set_contact_readout_gradients(1, S.wj[:T], S.ww[:T])
            gx, gv = S.gx[T - 1], S.gv[T - 1]
            z = np.zeros((sc.nb, 3 * sc.N))
            dmu, par, fg = 0.0, [None] * T, [None] * T
            if chain != "step_backward":
                e.clear_schedules()
                e.set_contact_readout_gradients(1, S.wj[:T], S.ww[:T])
                e.set_seed_schedule(0, np.concatenate([z[None], S.ix[1:T]]), np.concatenate([z[None], S.iv[1:T]]))
                e.set_gradient(gx, gv)
            for s in range(T, 0, -1):
                if chain == "step_backward":
                    gb = e.step_backward(s, gx, gv, S.ix[s - 1] if s > 1 else z, S.iv[s - 1] if s > 1 else z, is_start=(s == 1))
                    gx, gv, dmu = gb["dL_dx"], gb["dL_dv"], dmu + gb["dL_dmu"]
                else:
                    e.rollout_backward(s, 1)
                    gx, gv, dmu = e.get_gradient()
                par[s - 1] = np.concatenate([v for v in e.get_param_gradients(s).values()], axis=None)
                fg[s - 1] = e.get_force_gradient()
            np.testing.assert_array_equal(gx, got["dx"], err_msg=chain)
            np.testing.assert_array_equal(gv, got["dv"], err_msg=chain)
            np.testing.assert_array_equal(np.stack(par), got["par"], err_msg=chain)
            np.testing.assert_array_equal(np.stack(fg), got["fg"], err_msg=chain)
            for b in range(sc.nb):
                assert records.mu_err(dmu[b], got["dmu"][b]) <= GATE, (chain, b)
            # a call that does NOT continue the chain adds its top record's part itself: the same step from a gradient set from outside
            if chain != "step_backward":
                e.set_gradient(S.gx[0], S.gv[0])
                e.rollout_backward(1, 1)
                fresh = e.get_gradient()[0]
                e.set_contact_readout_gradients(1, None, None)
                e.set_gradient(S.gx[0], S.gv[0])
                e.rollout_backward(1, 1)
                assert not np.array_equal(fresh, e.get_gradient()[0])
        lines.append("fused sweep = step_backward chain = one-step sweeps, bit for bit")
    finally:
        restore_oracle_records(S)
        print("\n" + "\n".join(lines))
    e.close()


# ---- split launches; a renumbered mesh ----
@pytest.mark.parametrize("K", [2, 4])
def test_split_launches(K):
    S, e1 = run_handed_in("split", steps=1)
    one = e1.step_backward(1, S.gx[0], S.gv[0], S.ix[0], S.iv[0], is_start=True)
    e1.close()
    S, e = run_handed_in("split", cluster=K, steps=1)
    got = e.step_backward(1, S.gx[0], S.gv[0], S.ix[0], S.iv[0], is_start=True)
    assert np.all(got["workgroups"] == K)
    for k in ("dL_dx", "dL_dv"):
        for b in range(S.sc.nb):
            assert rel(got[k][b], one[k][b]) <= GATE, (k, b)
    e.close()


def test_renumbered_mesh_with_an_odd_vertex_count():
    """the weights and the gradients are in the caller's numbering: the static scene with its vertices shuffled gives the shuffled gradients"""
    S = gs.scene("static")
    sc = S.sc
    assert sc.N % 2 == 1
    perm = np.random.default_rng(3).permutation(sc.N)          # new index k holds old vertex perm[k]
    inv = np.argsort(perm)
    e = cr.pv.make_engine(sc.V[perm], inv[sc.F], sc.prims, fabric=sc.fabric)
    assert e.layout()["renumbered"]
    cr.prepare(sc, e)
    p3 = (3 * perm[:, None] + np.arange(3)).reshape(-1)
    recs = S.oracle_records(0)
    for q in recs:
        for k in ("x", "v", "f", "r", "normal"):
            q[k] = q[k][p3]
        q["prim"] = q["prim"][perm]
    e.set_state(0, sc.Xe[0][:, p3], sc.Ve[0][:, p3])
    records.upload_oracle_records(e, 1, recs)
    e.set_contact_readout_gradients(1, S.wj[0][None][:, :, perm], S.ww[0][None])
    gb = e.step_backward(1, S.gx[0][:, p3], S.gv[0][:, p3], S.ix[0][:, p3], S.iv[0][:, p3], is_start=True)
    for b in range(sc.nb):
        want = S.backward(0, b, S.gx[0, b], S.gv[0, b], ix=S.ix[0, b], iv=S.iv[0, b], is_start=True)
        for k in ("dL_dx", "dL_dv"):
            assert rel(gb[k][b], want[k][p3]) <= GATE, (b, k, rel(gb[k][b], want[k][p3]))
        assert records.mu_err(gb["dL_dmu"][b], want["dL_dmu"]) <= GATE
    e.close()


# ---- sim_rollout(contact_readout=True) ----
def rollout_inputs(S, dev, dtype, T):
    sc = S.sc
    t = lambda a, g=True: torch.tensor(np.asarray(a), dtype=dtype, device=dev, requires_grad=g)
    return dict(x0=t(sc.Xe[0]), v0=t(sc.Ve[0]), mu=t(sc.mu), uniform_force=t(np.tile([0.01, 0.0, -0.02], (T, sc.nb, 1))),
                primitive_offsets=t(sc.D[:T], False), primitive_velocities=t(np.zeros((T, sc.nb, sc.G, 3))))


def rollout_loss(S, out, T, dev, dtype):
    xs, vs, jn, wr = out
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype, device=dev)
    return (xs * t(S.gx[:T])).sum() + (vs * t(S.gv[:T])).sum() + (jn * t(S.wj[:T])).sum() + (wr * t(S.ww[:T])).sum()


def test_sim_rollout_contact_readout_device_path_host_path_and_the_c_abi():
    S = gs.scene("static")
    sc = S.sc
    T = sc.steps
    grads, outs = {}, {}
    for path in ("cuda", "cpu", "stream"):
        e = cr.pv.make_engine(sc.V, sc.F, sc.prims, fabric=sc.fabric)
        e.alloc_batch(sc.nb, T)
        sim = BatchedSim(e, T)
        dev = torch.device("cpu") if path == "cpu" else torch.device("cuda", 0)
        dtype = torch.float64
        ctx = torch.cuda.stream(torch.cuda.Stream(dev)) if path == "stream" else contextlib.nullcontext()
        with ctx:
            inp = rollout_inputs(S, dev, dtype, T)
            out = sim_rollout(sim, inp["x0"], inp["v0"], steps=T, contact_readout=True, **{k: v for k, v in inp.items() if k not in ("x0", "v0")})
            assert len(out) == 4 and out[2].shape == (T, sc.nb, sc.N) and out[3].shape == (T, sc.nb, sc.G, 10) and out[2].dtype == dtype
            rollout_loss(S, out, T, dev, dtype).backward()
            if path != "cpu":
                torch.cuda.current_stream(dev).synchronize()
        ro = e.contact_readout(1, T)
        np.testing.assert_allclose(out[2].detach().cpu().numpy(), ro["normal_impulse"], rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(out[3].detach().cpu().numpy(), ro["wrench"], rtol=1e-6, atol=1e-12)
        grads[path] = {k: v.grad.detach().cpu().numpy() for k, v in inp.items() if v.requires_grad}
        outs[path] = [o.detach().cpu().numpy() for o in out]
        if path == "cuda":
            # the composition of C-ABI calls over the same tape
            e.set_seed_schedule(0, np.concatenate([np.zeros((1, sc.nb, 3 * sc.N)), S.gx[:T - 1]]), np.concatenate([np.zeros((1, sc.nb, 3 * sc.N)), S.gv[:T - 1]]))
            e.set_gradient(S.gx[T - 1], S.gv[T - 1])
            e.set_contact_readout_gradients(1, S.wj[:T], S.ww[:T])
            e.rollout_backward(T, T)
            dx, dv, dmu = e.get_gradient()
            np.testing.assert_array_equal(dx, grads[path]["x0"])
            np.testing.assert_array_equal(dv, grads[path]["v0"])
            np.testing.assert_array_equal(dmu, grads[path]["mu"])
            np.testing.assert_array_equal(np.stack([e.get_param_gradients(s)["sum_dfext"] for s in range(1, T + 1)]), grads[path]["uniform_force"])
            np.testing.assert_array_equal(e.get_primitive_velocity_gradients(1, T), grads[path]["primitive_velocities"])
            e.set_contact_readout_gradients(1, None, None)
            # the default call returns (xs, vs) as before
            e2 = cr.pv.make_engine(sc.V, sc.F, sc.prims, fabric=sc.fabric)
            e2.alloc_batch(sc.nb, T)
            inp2 = rollout_inputs(S, dev, dtype, T)
            plain = sim_rollout(BatchedSim(e2, T), inp2["x0"], inp2["v0"], steps=T, **{k: v for k, v in inp2.items() if k not in ("x0", "v0")})
            assert len(plain) == 2
            np.testing.assert_array_equal(plain[0].detach().cpu().numpy(), outs[path][0])
            (plain[0] * torch.tensor(S.gx[:T], device=dev)).sum().add((plain[1] * torch.tensor(S.gv[:T], device=dev)).sum()).backward()
            for k in ("x0", "v0", "mu", "uniform_force", "primitive_velocities"):          # the read-out's part is in every one of them
                assert rel(inp2[k].grad.cpu().numpy(), grads[path][k]) >= 100 * GATE, k
            e2.close()
        e.close()
    for k in grads["cuda"]:
        np.testing.assert_array_equal(grads["cuda"][k], grads["stream"][k], err_msg=k)
        assert rel(grads["cuda"][k], grads["cpu"][k]) <= 1e-6, (k, rel(grads["cuda"][k], grads["cpu"][k]))      # (the device path rounds its inputs on the device)


def test_sim_rollout_actions_receive_the_read_outs_part():
    """a scene with clipped corners: the action gradient is dL_dxfixed of every step, read-out's part included — the C-ABI composition bit for
    bit; and a loss on the read-out ALONE reaches the actions (without the feature that gradient is exactly zero)"""
    S = gs.scene("static")
    sc = S.sc
    T = 2
    att = (0, 16)
    dev, dtype = torch.device("cuda", 0), torch.float64
    acts = np.tile(sc.V[list(att)].reshape(-1), (T, sc.nb, 1)) + 0.01
    for state_loss in (True, False):
        e = cr.pv.make_engine(sc.V, sc.F, sc.prims, att=att, fabric=sc.fabric)
        e.alloc_batch(sc.nb, T)
        t = lambda a, g=True: torch.tensor(np.asarray(a), dtype=dtype, device=dev, requires_grad=g)
        x0, v0, a = t(sc.Xe[1]), t(sc.Ve[1]), t(acts)
        gx = S.gx[:T] if state_loss else np.zeros_like(S.gx[:T])
        out = sim_rollout(BatchedSim(e, T), x0, v0, a, contact_readout=True, primitive_offsets=t(sc.D[1:1 + T], False))
        assert out[3][:, :, 0, 7:10].sum() > 0          # there are contacts to weigh
        ((out[0] * t(gx, False)).sum() + (out[2] * t(S.wj[:T], False)).sum() + (out[3] * t(S.ww[:T], False)).sum()).backward()
        got = a.grad.cpu().numpy()
        e.set_seed_schedule(0, np.concatenate([np.zeros((1, sc.nb, 3 * sc.N)), gx[:T - 1]]))
        e.set_gradient(gx[T - 1], np.zeros_like(gx[T - 1]))
        e.set_contact_readout_gradients(1, S.wj[:T], S.ww[:T])
        e.rollout_backward(T, T)
        np.testing.assert_array_equal(e.get_dxfixed(1, T), got)
        if not state_loss:
            assert np.all(np.abs(got).reshape(T, sc.nb, -1).max(axis=2) > 0), got
            assert np.abs(x0.grad.cpu().numpy()).max() > 0 and np.abs(v0.grad.cpu().numpy()).max() > 0
        e.close()


def test_refusals_on_a_device_context():
    S = gs.scene("static")
    sc = S.sc
    e = cr.pv.make_engine(sc.V, sc.F, sc.prims, fabric=sc.fabric)
    e.alloc_batch(sc.nb, 2)
    j, w = np.zeros((1, sc.nb, sc.N)), np.zeros((1, sc.nb, sc.G, 10))
    for slot0, jj, msg in ((0, j, "slot 0"), (3, j, "past the tape"), (2, np.zeros((2, sc.nb, sc.N)), "past the tape")):
        with pytest.raises((capi.DcError, ValueError), match=msg):
            e.set_contact_readout_gradients(slot0, jj)
    e.set_contact_readout_gradients(2, j, w)
    e.set_contact_readout_gradients(1, None, None)
    e.close()
    e = cr.pv.make_engine(sc.V, sc.F, [], fabric=sc.fabric)
    e.alloc_batch(1, 2)
    with pytest.raises(capi.DcError, match="no primitive group"):
        e.set_contact_readout_gradients(1, None, np.zeros((1, 1, 1, 10)))
    e.set_contact_readout_gradients(1, np.zeros((1, 1, sc.N)))          # jn weights alone are accepted: there is no contact to weigh
    e.close()
