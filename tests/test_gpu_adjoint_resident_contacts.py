"""The adjoint operator's contact phase from step-resident tables (csrc/dc_adjoint.hip: build_contact_tables, contact_phase_resident; the list
ordered by vertex index, slot = rank among the set bits of the contact mask), through the C-ABI with one workgroup per rollout
(DC_CLUSTER=1), adjoint_mode 1, the diag(P) preconditioner (the instances whose correction solves are CG's) at the forward threshold of
tests/test_gpu_adjoint_own_slot.py, on the 48 x 48 grid (2 304 vertices, three element windows, bending rows on), two rollouts (the state and
a perturbation of it), ONE backward step per case:

  * the C4 cloth with a flap of 12 rows folded back and dropped 0.06 into the sphere: ~100 primitive contacts, 576 self contacts in two
    layers, ~90 vertices in both kinds of contact (asserted from the engine's record);
  * the same sheet unfolded with self collision off: primitive contacts only — on the 56 x 56 grid (4 windows), where the operator takes the
    list forms without self contacts, and on the 48 x 48 grid, where it forms y in the staging and no tables are built;
  * tests/selfdetect_cases.py's zigzag on this grid: 336 self contacts in 289 thin layers (past kWideLayers = 8: one wave walks them);
  * the flap scene over the oracle's rotating sphere, the engine's plain sphere given a velocity (zero) and the spin (0, 8 / radius, 0): the
    context has a motion table, so the step runs k_adjoint_step_moving;
  * three steps of the flap scene as one fused backward sweep: the contact sets of its steps differ (asserted), so tables left over from
    the step before would give other gradients than the three single-step launches do — bitwise equal.

Every case runs the backward step three times on one record: the default (tables resident: dc_get_adjoint_contact_path says so per
rollout), DC_ADJ_RESIDENT=0 (the path without them) and DC_TEST_YTAB_CAP=16 (tables refused by the fit rule: the fall-back inside the
same build, reported by the same counters). dL_dx, dL_dv, dL_dmu are bitwise equal and cg_iters, adjoint_iters, refine_cycles identical
across the three. The default run's gradient of rollout 0 is held to the fp64 oracle on the SAME record (the oracle adopts the engine's
record and solves it directly) at 1e-4, the same-record tolerance of tests/test_gpu_adjoint_own_slot.py. The rank arithmetic and the fit
rule are tests/test_resident_rank.py's."""
import numpy as np
import pytest

import orc
import records
import selfdetect_cases as sc
from diffcloth_amd import capi, workloads
from test_gpu_bend_rows import FWD_TOL, H, MU, f32

pytestmark = pytest.mark.gpu

B = 2
NX = 48
FOLD = 12
SAME_RECORD_TOL = 1e-4
RADIUS = workloads.C4_CLOTH["sphere_radius"]
MAT = {k: workloads.C4_CLOTH[k] for k in ("density", "k_stretch", "k_bend")}
STAT_KEYS = ("cg_iters", "adjoint_iters", "refine_cycles")
_cache = {}


def flap(fold, rotates=False, nx=NX):
    """the scene's mesh, sphere centre, fp64 oracle and the state after one settling step of the oracle (computed once, never changed)"""
    key = (fold, rotates, nx)
    if key not in _cache:
        V, F, V0, _, c = workloads.c4_scene(nx, fold, 0.05)
        o = orc.Oracle(V, F, h=H, fwd_tol=FWD_TOL, bwd_tol=1e-9, selfcollision=fold > 0, gradient_clipping=False, **MAT)
        o.add_sphere(c, RADIUS, MU, rotates=rotates)
        o.build()
        x = f32(V0.reshape(-1) + np.tile([0.0, -0.06, 0.0], V.shape[0]))
        out = o.step(x, np.zeros_like(x))
        assert out["converged"]
        _cache[key] = dict(V=V, F=F, c=c, o=o, x=f32(out["x"]), v=f32(out["v"]))
    return _cache[key]


def engine(V, F, c, selfcollision, min_windows=2):
    e = capi.Engine(0)
    e.set_mesh(V, F)
    e.set_params(time_step=H, forward_tol=FWD_TOL, backward_tol=1e-9, cg_rel_tol=1e-6, cg_max_iter=3000, gradient_clipping=0,
                 selfcollision_enabled=int(selfcollision), adjoint_mode=1, adjoint_rel_tol=1e-7, adjoint_block_precond=0, **MAT)
    e.set_primitives([dict(kind=capi.DC_PRIM_SPHERE, group=0, center=c, radius=RADIUS, mu=MU)])
    e.build()
    assert e.layout()["element_windows"] and e.bend_rows() and e.layout()["windows"] >= min_windows      # (48 x 48: 3 element windows)
    return e


def batch(x, v, seed):
    rng = np.random.default_rng(seed)
    X0 = np.stack([x, f32(x + 1e-4 * rng.standard_normal(x.size))])
    V0 = np.stack([v, f32(v + 1e-3 * rng.standard_normal(x.size))])
    gx = f32(rng.standard_normal(X0.shape)); gv = f32(0.01 * rng.standard_normal(X0.shape))
    return X0, V0, gx, gv


def switches(monkeypatch, resident, cap):
    for name, val in (("DC_ADJ_RESIDENT", resident), ("DC_TEST_YTAB_CAP", cap)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(val))


def three_ways(e, monkeypatch, run, steps=1, held=True):
    """run() under the default, with the tables switched off and with their room capped; the path counters of each; all three identical.
    held: the default run holds the tables (False: a step the operator never takes them for). Returns the default run's result."""
    out = []
    for tag, resident, cap, want in (("resident", None, None, steps if held else 0), ("switched off", 0, None, 0), ("room capped", None, 16, 0)):
        switches(monkeypatch, resident, cap)
        e.adjoint_contact_path(reset=True)
        g = run()
        path = e.adjoint_contact_path()
        assert np.all(path[:, 0] == steps), (tag, path)                  # an instance that can hold the tables ran every step
        assert np.all(path[:, 1] == want), (tag, path)                   # and held them exactly when it may
        out.append(g)
    switches(monkeypatch, None, None)
    for tag, g in zip(("switched off", "room capped"), out[1:]):
        for a, b in zip(out[0], g):
            for k in ("dL_dx", "dL_dv", "dL_dmu"):
                assert k == "dL_dmu" or np.abs(a[k]).max() > 0          # (dL_dmu is zero in a scene without a primitive)
                np.testing.assert_array_equal(a[k], b[k], err_msg=f"{tag}: {k}")
            for k in STAT_KEYS:
                np.testing.assert_array_equal(a[k], b[k], err_msg=f"{tag}: {k}")
    return out[0]


def same_record(o, e, X0, V0, gx, gv, g, tag, b=0, slot=1):
    """the oracle adopts the engine's record of rollout b at `slot` (X0, V0: the state of slot - 1) and differentiates it with its direct solve"""
    x1, v1 = e.get_state(slot)
    f = e.get_record(slot)[0]
    ref = o.step(X0[b], V0[b])
    assert ref["converged"]
    st = e.get_stats(slot)[0]
    assert st["prim_contacts"][b] == ref["nprim"] and st["self_contacts"][b] == ref["nself"], "the contact sets must agree for the adoption"
    matched = records.oracle_adopts_gpu_record(o, ref["id"], e, slot, b, X0[b], x1[b], v1[b], f[b], H, normals=e.get_contacts(slot)[1])
    assert matched == ref["nself"]
    rb = o.step_backward(ref["id"], gx[b], gv[b], is_start=False, direct=True)
    assert 0 <= rb["direct_residual"] <= 1e-10
    errs = dict(dx=records.rel(g["dL_dx"][b], rb["dL_dx"]), dv=records.rel(g["dL_dv"][b], rb["dL_dv"]),
                dmu=records.mu_err(g["dL_dmu"][b], rb["dL_dmu"][:g["dL_dmu"].shape[1]]) if o.nprim > 0 else 0.0)
    print(f"\n[resident contacts] {tag}: same record, oracle adopts: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items())
          + f"; CG iterations {g['cg_iters']} BiCGSTAB {g['adjoint_iters']} fp32 solves {g['refine_cycles']}")
    assert max(errs.values()) <= SAME_RECORD_TOL, errs
    return ref


def one_step(e, o, X0, V0, gx, gv, monkeypatch, tag, held=True):
    e.alloc_batch(B, 1)
    e.set_state(0, X0, V0)
    st = e.step_forward(0)
    assert np.all(st["converged"] == 1)
    g = three_ways(e, monkeypatch, lambda: [e.step_backward(1, gx, gv, is_start=False)], held=held)[0]
    assert np.all(g["converged"] == 1) and np.all(g["cg_iters"] > 0) and np.all(g["fp64_iters"] == 0)
    same_record(o, e, X0, V0, gx, gv, g, tag)
    return st


def both_kinds(e, b=0):
    """vertices of rollout b's record (slot 1) in contact with the sphere AND in a self contact"""
    prim = np.flatnonzero(e.get_contacts(1)[0][b] >= 0)
    pairs = e.get_self_contacts(1, rollout=b, cap=16384)["pairs"]
    return np.intersect1d(prim, np.unique(pairs))


def test_flap_on_the_sphere_self_and_primitive_contacts_on_the_same_vertices(monkeypatch):
    """cases 1 and 2: switch on = switch off = room capped, with both kinds of contact and vertices in both"""
    monkeypatch.setenv("DC_CLUSTER", "1")
    s = flap(FOLD)
    e = engine(s["V"], s["F"], s["c"], True)
    try:
        X0, V0, gx, gv = batch(s["x"], s["v"], 21)
        st = one_step(e, s["o"], X0, V0, gx, gv, monkeypatch, f"flap of {FOLD} rows")
        both = both_kinds(e)
        sl = e.get_self_contacts(1, rollout=0, cap=16384)
        print(f"[resident contacts] primitive contacts {st['prim_contacts']} self contacts {st['self_contacts']} in {sl['layers']} layers, vertices in both {len(both)}")
        assert np.all(st["prim_contacts"] >= 10) and np.all(st["self_contacts"] >= 100) and len(both) >= 1 and sl["layers"] <= 8
    finally:
        e.close()


@pytest.mark.parametrize("nx,windows,held", [(56, 4, True), (48, 3, False)], ids=["56x56-four-windows-tables", "48x48-three-windows-early-branch"])
def test_primitive_contacts_only(nx, windows, held, monkeypatch):
    """case 3: nself = 0 — the unfolded sheet on the sphere, self collision off. Without self contacts adjoint_operator forms y per vertex in the
    staging on a mesh of fewer than 4 windows and returns before either list form: the resident phase with an empty working set (no self
    tables, every primitive entry without a working-set slot, no layer walk) runs on the 56 x 56 grid (4 windows, as in
    tests/test_gpu_adjoint_own_slot.py); on the 48 x 48 grid the tables are not built and the counters say so."""
    monkeypatch.setenv("DC_CLUSTER", "1")
    s = flap(0, nx=nx)
    e = engine(s["V"], s["F"], s["c"], False, min_windows=windows)
    try:
        assert e.layout()["windows"] == windows
        X0, V0, gx, gv = batch(s["x"], s["v"], 22)
        st = one_step(e, s["o"], X0, V0, gx, gv, monkeypatch, f"unfolded sheet {nx} x {nx}", held=held)
        assert np.all(st["prim_contacts"] >= 10) and np.all(st["self_contacts"] == 0)
    finally:
        e.close()


def test_chain_of_thin_layers_walked_by_one_wave(monkeypatch):
    """case 4: hundreds of layers of one or two contacts (the zigzag fold on this grid)"""
    monkeypatch.setenv("DC_CLUSTER", "1")
    if "zigzag" not in _cache:
        case = sc.zigzag("zigzag48", nx=NX, rows=4, gap=0.06, seed=0)
        _cache["zigzag"] = (case, sc.oracle_of(case, threads=8))
    case, o = _cache["zigzag"]
    e = sc.engine_of(case, adjoint_mode=1, adjoint_block_precond=0)
    try:
        assert e.layout()["element_windows"] and e.bend_rows() and e.layout()["windows"] >= 2      # (more than one element window: 3 on this grid)
        X0, V0, gx, gv = batch(case["X"].reshape(-1), case["Vel"].reshape(-1), 23)
        X0[1], V0[1] = X0[0], V0[0]          # (the detection's margins hold for the case's own state: both rollouts run it)
        st = one_step(e, o, X0, V0, gx, gv, monkeypatch, "zigzag")
        sl = e.get_self_contacts(1, rollout=0, cap=16384)
        print(f"[resident contacts] zigzag: {sl['count']} self contacts in {sl['layers']} layers")
        assert sl["layers"] > 8 and np.all(st["self_contacts"] >= 100)
    finally:
        e.close()


def test_moving_instance_with_a_velocity_and_a_spin_set(monkeypatch):
    """case 5: the context has a motion table (velocity zero, spin that of the oracle's rotating sphere)"""
    monkeypatch.setenv("DC_CLUSTER", "1")
    s, rot = flap(FOLD), flap(FOLD, rotates=True)
    e = engine(s["V"], s["F"], s["c"], True)
    try:
        X0, V0, gx, gv = batch(s["x"], s["v"], 24)
        e.alloc_batch(B, 1)
        e.set_primitive_velocities(np.zeros((B, 1, 3)))
        e.set_primitive_spins(np.tile([0.0, 8.0 / RADIUS, 0.0], (B, 1, 1)))
        e.set_state(0, X0, V0)
        st = e.step_forward(0)
        assert np.all(st["converged"] == 1) and np.all(st["prim_contacts"] >= 10) and np.all(st["self_contacts"] >= 100)
        g = three_ways(e, monkeypatch, lambda: [e.step_backward(1, gx, gv, is_start=False)])[0]
        assert np.all(g["converged"] == 1) and np.all(g["cg_iters"] > 0)
        assert np.abs(e.get_primitive_spin_gradients(1, 1)).max() > 0          # (the moving kernel ran: only it writes dL/domega)
        same_record(rot["o"], e, X0, V0, gx, gv, g, "spinning sphere")
        assert len(both_kinds(e)) >= 1
    finally:
        e.close()


def test_fused_sweep_rebuilds_the_tables_every_step(monkeypatch):
    """case 6: three steps whose contact sets differ, as one launch and as three"""
    monkeypatch.setenv("DC_CLUSTER", "1")
    s = flap(FOLD)
    S = 3
    e = engine(s["V"], s["F"], s["c"], True)
    try:
        X0, V0, gx, gv = batch(s["x"], s["v"], 25)
        e.alloc_batch(B, S)
        e.set_state(0, X0, V0)
        e.rollout_forward(0, S)
        prim = [e.get_contacts(k)[0] >= 0 for k in range(1, S + 1)]
        assert all(p[0].sum() >= 10 for p in prim)
        assert any(np.any(prim[k] != prim[k + 1]) for k in range(S - 1)), "the steps' contact sets must differ"

        def sweep(nsteps):
            e.set_gradient(gx, gv)
            for k in range(S, 0, -nsteps):
                e.rollout_backward(k, nsteps)
            dx, dv, dmu = e.get_gradient()[:3]
            stats = [e.get_stats(k)[1] for k in range(1, S + 1)]
            assert all(np.all(q["converged"] == 1) and np.all(q["cg_iters"] > 0) for q in stats)
            return dict(dL_dx=dx, dL_dv=dv, dL_dmu=dmu, **{k: np.stack([q[k] for q in stats]) for k in STAT_KEYS})

        fused = three_ways(e, monkeypatch, lambda: [sweep(S)], steps=S)[0]
        single = three_ways(e, monkeypatch, lambda: [sweep(1)], steps=S)[0]
        for k in ("dL_dx", "dL_dv", "dL_dmu") + STAT_KEYS:
            np.testing.assert_array_equal(fused[k], single[k], err_msg=k)
        # the first step of the sweep (record S) as a launch of its own, from the state the engine reached at S - 1: held to the oracle on the same record
        e.set_gradient(gx, gv)
        e.rollout_backward(S, 1)
        dx, dv, dmu = e.get_gradient()[:3]
        g = dict(dL_dx=dx, dL_dv=dv, dL_dmu=dmu, **{k: e.get_stats(S)[1][k] for k in STAT_KEYS})
        xp, vp = e.get_state(S - 1)
        same_record(s["o"], e, xp, vp, gx, gv, g, "first step of the sweep", slot=S)
    finally:
        e.close()
