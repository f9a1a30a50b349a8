"""Moving obstacles: a velocity per rollout, primitive group and step (dc_set_primitive_velocities, dc_set_primitive_velocity_schedule, their
_dev forms, dc_get_primitive_velocities, dc_get_primitive_velocity_gradients; sim_rollout(primitive_velocities=...)).

The rule under test (include/diffcloth_hip.h): d = (f - v_rot m) - w m in the friction law, forward and adjoint, and detection samples
pos + (vel - w) h k / 2. With both the step is Galilean invariant: the engine stepping (x, v + w) under an obstacle of velocity w computes the
static step at (x, v) shifted by (w h, w) — so the fp64 oracle with its STATIC sphere is the parity partner, forward and backward.

Scene: the 17 x 17 base scene of tests/test_gpu_primitive_offsets.py (sphere of radius 2, h = 1/180, mu 0.4, its tight solver settings), four
steps from rest, B = 4, dyadic velocities
  b0  w = 0
  b1  w = (2, -1, -0.5)
  b2  w = (-4, 0, 2)
  b3  the sphere out of reach (centre offset (0, -4, 0)), w = (1, 1, 1)
|w| h exceeds 100 x the forward gate (5e-3) on b1 and b2, so a step that lacks the term cannot pass, and b1's vertical component points DOWN:
under an upward w the static law sees the cloth (at v + w) leaving a sphere it believes at rest, every contact takes off, and the step misses
the oracle by the free fall g h^2 = 3.0e-4 only, whatever |w|; a sphere moving down and sideways is what the static law gets wrong by |w| h.

Every step is compared at t_n = 0 (teacher-forced): the oracle steps (x, v) with its static sphere at the fp32 centre, the engine steps
(x, v + w) with the same centre and velocity w, and the next step starts again from the ORACLE's state (rounded to fp32, the engine's v being
f32(v + w) and the oracle's that value minus w), so rounding of a drifting frame never accumulates. The oracle's trajectory therefore does
not depend on the engine: it is computed once per scene and shared by the tests.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch          # before the engine's library: both must share ONE HIP runtime (torch's), see tests/test_gpu_functional.py

import meshes
import orc
import records
import test_gpu_primitive_offsets as po          # its scene builders (helpers, not tests)
from diffcloth_amd import capi, workloads
from diffcloth_amd.functional import BatchedSim, sim_rollout

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = po.H
B, S = 4, 4
FABRIC = po.FABRIC
f32, rel = po.f32, po.rel
GATE_X = 5e-5
W1 = np.array([[0.0, 0.0, 0.0], [2.0, -1.0, -0.5], [-4.0, 0.0, 2.0], [1.0, 1.0, 1.0]]).reshape(B, 1, 3)
D1 = np.array([[0.0, 0.125, 0.0], [0.25, 0.1875, 0.125], [0.0, 0.125, 0.0], [0.0, -4.0, 0.0]]).reshape(B, 1, 3)      # (b0, b1, b3: offsets of that scene)


def make_engine(V, F, prims, att=(), mode=1, selfcollision=0, fabric=FABRIC, tight=True, cg_max_iter=2000):
    e = capi.Engine(0)
    e.set_mesh(V, F)
    e.set_attachments(att)
    tol = dict(forward_tol=1e-9, backward_tol=1e-9, cg_rel_tol=1e-6, adjoint_rel_tol=1e-8) if tight else \
        dict(forward_tol=1e-7, backward_tol=1e-7, cg_rel_tol=1e-5, adjoint_rel_tol=1e-7)
    e.set_params(time_step=H, cg_max_iter=cg_max_iter, gradient_clipping=0, selfcollision_enabled=selfcollision, adjoint_mode=mode, **fabric, **tol)
    e.set_primitives(prims)
    e.build()
    return e


def sphere(c, group=0, rotates=0):
    return dict(kind=capi.DC_PRIM_SPHERE, group=group, center=c, radius=2.0, mu=0.4, rotates=rotates)


def mass3(e):
    return np.repeat(e.vertex_data()[0], 3)


class Scene:
    """Mesh, spheres [(centre, rotates)], per-rollout velocities W [B][G][3] and centre offsets D [B][G][3], attachments; and the oracle's
    teacher-forced trajectory in the static frame with everything the tests compare against, computed once (CPU, fp64)."""

    def __init__(self, spheres, W, D, att=(), steps=S, nx=17, threads=1):
        self.V, self.F = meshes.grid_cloth(nx, nx, 4.5, 4.5, "DOWN")
        self.V = f32(self.V)
        self.N = self.V.shape[0]
        self.c0 = f32(meshes.sphere_scene_center(self.V, 2.0))
        self.spheres = [(f32(self.c0 + np.asarray(d)), rot) for d, rot in spheres]
        self.G = len(self.spheres)
        self.W, self.D, self.att, self.steps = np.asarray(W, dtype=np.float64), np.asarray(D, dtype=np.float64), tuple(att), steps
        self.nb = self.W.shape[0]
        self.prims = [sphere(c, group=g, rotates=rot) for g, (c, rot) in enumerate(self.spheres)]
        N = self.N
        rng = np.random.default_rng(31)
        self.gx = f32(rng.standard_normal((steps, self.nb, 3 * N)))
        self.gv = f32(0.01 * rng.standard_normal((steps, self.nb, 3 * N)))
        # the frame velocity of a rollout: attachments tie the cloth to the frame, so with them every group of the rollout moves at one w
        self.wf = self.W[:, 0, :]
        self.oracles = []
        self.ref = [[None] * self.nb for _ in range(steps)]
        self.Xe = np.zeros((steps, self.nb, 3 * N)); self.Ve = np.zeros_like(self.Xe)
        self.XFe = np.zeros((steps, self.nb, 3 * len(self.att)))
        for b in range(self.nb):
            o = orc.Oracle(self.V, self.F, h=H, fwd_tol=1e-9, bwd_tol=1e-9, selfcollision=False, gradient_clipping=False,
                           attachments=list(self.att), threads=threads, **FABRIC)
            for g, (c, rot) in enumerate(self.spheres):
                o.add_sphere(f32(c + self.D[b, g]), 2.0, 0.4, rotates=bool(rot))
            o.build()
            self.oracles.append(o)
            wt = np.tile(self.wf[b], N)
            x = f32(self.V.reshape(-1)); ve = f32(wt)                          # from rest in the static frame
            xf_rest = self.V[list(self.att)].reshape(-1) if self.att else np.zeros(0)
            for s in range(steps):
                self.Xe[s, b], self.Ve[s, b] = x, ve
                xfe = f32(xf_rest + np.tile(self.wf[b], len(self.att)) * H) if self.att else np.zeros(0)      # the engine's targets: moved by w h
                self.XFe[s, b] = xfe
                xfo = xfe - np.tile(self.wf[b], len(self.att)) * H if self.att else None                    # the oracle's: exactly those minus w h
                r = o.step(x, ve - wt, xfo)
                r["pc"] = o.prim_contacts(r["id"])
                r["f"] = o.record_fr(r["id"])[0]
                r["bwd"] = {st: o.step_backward(r["id"], self.gx[s, b], self.gv[s, b], is_start=bool(st), direct=True) for st in (0, 1)}
                self.ref[s][b] = r
                x = f32(r["x"]); ve = f32(r["v"] + wt)

    def engine(self, mode=1, **kw):
        return make_engine(self.V, self.F, self.prims, att=self.att, mode=mode, **kw)

    def expected_dw(self, s, b):
        """per group: (sum of c_i over the vertices in contact with it, sum of |c_i|_2), c_i = h dL_dx_i + g_v,i - dL_dv_i from the oracle's
        is_start = 1 outputs (dx = u m - g_v / h, dv = y h m in finish_gradients, Simulation.cpp:1672-1764: c_i = -h m_i (y_i - u_i))"""
        r = self.ref[s][b]
        rb = r["bwd"][1]
        ci = (H * rb["dL_dx"] + self.gv[s, b] - rb["dL_dv"]).reshape(-1, 3)
        out = []
        for g in range(self.G):
            ids = r["pc"]["particle"][r["pc"]["prim"] == g]
            out.append((ci[ids].sum(axis=0), float(np.linalg.norm(ci[ids], axis=1).sum())))
        return out, ci


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "base":
        return Scene([((0, 0, 0), 0)], W1, D1)
    if name == "rotating":
        return Scene([((0, 0, 0), 1)], W1[:3], D1[:3], steps=2)
    if name == "two_one_reachable":          # group 1 far below: never in contact
        return Scene([((0, 0.125, 0), 0), ((0, -6, 0), 0)], np.concatenate([W1[:3], W1[:3][::-1]], axis=1), np.zeros((3, 2, 3)), steps=2)
    if name == "two_reachable":              # two spheres side by side under the cloth, both moving at the rollout's w
        return Scene([((-1.0, 0.125, 0), 0), ((1.0, 0.125, 0), 0)], np.concatenate([W1[:3], W1[:3]], axis=1), np.zeros((3, 2, 3)), steps=2)
    if name == "attached":
        return Scene([((0, 0, 0), 0)], W1[:3], D1[:3], att=(0, 16), steps=2)
    raise KeyError(name)


def contact_ids(grp_row):
    return np.nonzero(grp_row >= 0)[0]


def start_batch(sc, e, velocities=True):
    e.alloc_batch(sc.nb, sc.steps)
    if np.abs(sc.D).max() > 0:
        e.set_primitive_offsets(sc.D)
    if velocities:
        e.set_primitive_velocities(sc.W)


def forward_step(sc, e, s):
    """the engine's step s from the shared (oracle) state; everything the step leaves behind"""
    e.set_state(s, sc.Xe[s], sc.Ve[s])
    st = e.step_forward(s, fixed_pts=sc.XFe[s] if sc.att else None)
    x1, v1 = e.get_state(s + 1)
    grp, nrm = e.get_contacts(s + 1)
    f = e.get_record(s + 1)[0]
    return dict(st=st, x=x1, v=v1, grp=grp, nrm=nrm, f=f)


def check_forward(sc, got, s, lines, tag=""):
    m3 = None
    for b in range(sc.nb):
        ref, wt = sc.ref[s][b], np.tile(sc.wf[b], sc.N)
        assert got["st"]["converged"][b] == 1 and ref["converged"]
        assert got["st"]["prim_contacts"][b] == ref["nprim"], (s, b)
        ids = contact_ids(got["grp"][b])
        order = np.argsort(ref["pc"]["particle"])
        np.testing.assert_array_equal(ids, ref["pc"]["particle"][order])                                        # the same vertices are in contact
        np.testing.assert_allclose(got["nrm"][b].reshape(-1, 3)[ids], ref["pc"]["normal"][order], atol=2e-6)    # with the same normals
        dx = np.abs(got["x"][b] - wt * H - ref["x"]).max()
        dv = np.abs(got["v"][b] - wt - ref["v"]).max()
        xc = np.abs(got["x"][b] - (sc.Xe[s, b] + H * got["v"][b])).max()
        if m3 is None:
            m3 = sc.m3
        df = rel(got["f"][b] - m3 * wt, ref["f"])
        lines.append(f"{tag}step {s} rollout {b}: contacts {ref['nprim']}, PD iterations gpu {got['st']['pd_iters'][b]} / oracle {ref['iters']}, "
                     f"max|x - w h - x_oracle| {dx:.2e}, max|v - w - v_oracle| {dv:.2e}, f - m w vs oracle f {df:.2e}")
        assert dx <= GATE_X, lines[-1]
        assert xc <= 1e-6 and dv <= 2 * GATE_X / H, lines[-1]          # v_new is (x_new - x) / h: consistent with the x gate


def check_backward(sc, e, got, s, is_start, lines, gate=1e-4):
    """end to end, on the engine's record (the oracle adopts it, frame-shifted) and — separately, see check_injected — on the oracle's"""
    gb = e.step_backward(s + 1, sc.gx[s], sc.gv[s], is_start=bool(is_start))
    dw = e.get_primitive_velocity_gradients(s + 1, 1)[0]
    for b in range(sc.nb):
        ref, wt, o = sc.ref[s][b], np.tile(sc.wf[b], sc.N), sc.oracles[b]
        rb = ref["bwd"][int(bool(is_start))]
        ex, ev = rel(gb["dL_dx"][b], rb["dL_dx"]), rel(gb["dL_dv"][b], rb["dL_dv"])
        em = records.mu_err(gb["dL_dmu"][b], rb["dL_dmu"])
        records.oracle_adopts_gpu_record(o, ref["id"], e, s + 1, b, sc.Xe[s, b], got["x"][b] - wt * H, got["v"][b] - wt, got["f"][b] - sc.m3 * wt, H,
                                         normals=got["nrm"])
        rb3 = o.step_backward(ref["id"], sc.gx[s, b], sc.gv[s, b], is_start=bool(is_start), direct=True)
        ea = max(rel(gb["dL_dx"][b], rb3["dL_dx"]), rel(gb["dL_dv"][b], rb3["dL_dv"]), records.mu_err(gb["dL_dmu"][b], rb3["dL_dmu"]))
        o.override_record(ref["id"], x=ref["x"], f=ref["f"])           # (the shared record back to the oracle's own values; normals within 2e-6)
        lines.append(f"  backward step {s} rollout {b} is_start {int(is_start)}: dL_dx {ex:.2e} dL_dv {ev:.2e} dL_dmu {em:.2e}, same record (oracle adopts) {ea:.2e}")
        assert ex <= gate and ev <= gate and em <= gate, lines[-1]
        assert ea <= gate, lines[-1]
        if is_start:
            want, _ = sc.expected_dw(s, b)
            for g in range(sc.G):
                err = np.linalg.norm(dw[b, g] - want[g][0])
                lines.append(f"    dL/dw[{g}] engine {dw[b, g]} oracle {want[g][0]} |diff| {err:.2e} scale {want[g][1]:.2e}")
                assert err <= 1e-4 * want[g][1], lines[-1]
                if want[g][1] == 0.0:
                    assert np.all(dw[b, g] == 0.0), lines[-1]          # a group nothing touches: exactly zero
    return gb, dw


def check_injected(sc, e, s, is_start, lines):
    """the other direction: the oracle's record, transformed x + w h, v + w, f + m w, uploaded with dc_set_record; the backward step through
    it reads row s + 1 of the velocity table, set by a one-step schedule at s"""
    recs = []
    for b in range(sc.nb):
        ref, wt = sc.ref[s][b], np.tile(sc.wf[b], sc.N)
        q = records.oracle_record(sc.oracles[b], ref)
        q["x"] = q["x"] + wt * H; q["v"] = q["v"] + wt; q["f"] = q["f"] + sc.m3 * wt
        recs.append(q)
    e.set_state(s, sc.Xe[s], sc.Ve[s])
    records.upload_oracle_records(e, s + 1, recs, x_fixed=sc.XFe[s] if sc.att else None)
    e.set_primitive_velocity_schedule(s, sc.W[None])
    gb = e.step_backward(s + 1, sc.gx[s], sc.gv[s], is_start=bool(is_start))
    dw = e.get_primitive_velocity_gradients(s + 1, 1)[0]
    for b in range(sc.nb):
        rb = sc.ref[s][b]["bwd"][int(bool(is_start))]
        err = max(rel(gb["dL_dx"][b], rb["dL_dx"]), rel(gb["dL_dv"][b], rb["dL_dv"]), records.mu_err(gb["dL_dmu"][b], rb["dL_dmu"]))
        lines.append(f"  oracle's record injected, step {s} rollout {b} is_start {int(is_start)}: {err:.2e}")
        assert err <= 1e-4, lines[-1]
        if is_start:          # dL/dw through the fp64 record's branch (contact_JT_d on inj_f)
            want, _ = sc.expected_dw(s, b)
            for g in range(sc.G):
                edw = np.linalg.norm(dw[b, g] - want[g][0])
                lines.append(f"    injected dL/dw[{g}] |diff| {edw:.2e} scale {want[g][1]:.2e}")
                assert edw <= 1e-4 * want[g][1], lines[-1]
    e.clear_schedules()


def run_parity(name, mode=1, steps=None, backward=True, inject=True):
    sc = scene(name)
    e = sc.engine(mode=mode)
    sc.m3 = mass3(e)
    start_batch(sc, e)
    lines = []
    for s in range(sc.steps if steps is None else steps):
        got = forward_step(sc, e, s)
        np.testing.assert_array_equal(e.get_primitive_velocities(s + 1), f32(sc.W))
        check_forward(sc, got, s, lines)
        if backward:
            for is_start in (s % 2, 1 - s % 2):
                check_backward(sc, e, got, s, is_start, lines)
            if inject:
                check_injected(sc, e, s, s % 2, lines)
    print(f"\n[primitive velocities, scene {name}, adjoint_mode {mode}]\n" + "\n".join(lines))
    e.close()
    return sc


# ---- 1. forward parity, 3. backward parity (end to end, the engine's record adopted, the oracle's record injected), 4. dL/dw ----
def check_base_scene_is_not_vacuous():
    """>= 10 contacts per step on b0 .. b2, none on b3; b1 has sticking AND sliding contacts in at least one step (the oracle's contact types);
    out of contact |c_i| is at the oracle's solve tolerance, and dL/dw has something to measure on b0 .. b2"""
    sc = scene("base")
    both = False
    for s in range(S):
        for b in range(3):
            assert sc.ref[s][b]["nprim"] >= 10, (s, b, sc.ref[s][b]["nprim"])
        assert sc.ref[s][3]["nprim"] == 0
        ty = sc.ref[s][1]["pc"]["type"]
        both = both or ((ty == 1).sum() > 0 and (ty == 2).sum() > 0)
        for b in range(B):
            want, ci = sc.expected_dw(s, b)
            free = np.setdiff1d(np.arange(sc.N), sc.ref[s][b]["pc"]["particle"])
            scale = np.abs(H * sc.ref[s][b]["bwd"][1]["dL_dx"]).max()
            assert np.abs(ci[free]).max() <= 1e-6 * scale, (s, b, np.abs(ci[free]).max(), scale)
            assert (want[0][1] > 0) == (b < 3), (s, b, want)
    assert both


def test_forward_and_backward_parity_on_the_base_scene():
    run_parity("base", mode=1)


@pytest.mark.parametrize("mode", [2, 3])
def test_backward_parity_direct_adjoint_modes(mode):
    run_parity("base", mode=mode, steps=2)


def test_backward_parity_reference_iteration_one_step():
    run_parity("base", mode=0, steps=1)


def test_the_scene_can_see_the_term():
    """the same engine run with v + w but NO velocity set misses the oracle by more than 100 x the gate on b1 and b2 — on a scene that has
    something to see (check_base_scene_is_not_vacuous)"""
    check_base_scene_is_not_vacuous()
    sc = scene("base")
    e = sc.engine()
    start_batch(sc, e, velocities=False)
    lines = []
    for s in range(S):
        got = forward_step(sc, e, s)
        for b in range(B):
            miss = np.abs(got["x"][b] - np.tile(sc.wf[b], sc.N) * H - sc.ref[s][b]["x"]).max()
            lines.append(f"step {s} rollout {b}: without the term max|x - w h - x_oracle| {miss:.2e}")
            if b in (1, 2):
                assert miss > 100 * GATE_X, lines[-1]
            if b == 0:
                assert miss <= GATE_X, lines[-1]
    print("\n[primitive velocities unset]\n" + "\n".join(lines))
    with pytest.raises(capi.DcError, match="no primitive velocity has been set"):
        e.get_primitive_velocity_gradients(1, 1)
    e.close()


def test_rotating_sphere_spin_and_translation_add():
    run_parity("rotating", inject=False)


def test_two_groups_one_reachable_the_other_gradient_is_exactly_zero():
    sc = run_parity("two_one_reachable", inject=False)
    assert all(sc.expected_dw(s, b)[0][1][1] == 0.0 and sc.expected_dw(s, b)[0][0][1] > 0 for s in range(sc.steps) for b in range(sc.nb))


def total_identity(sc, s, b):
    """sum over the groups of dL/dw when every group moves at the rollout's w — the derivative along the frame velocity that is not already
    in dL_dv: h sum g_x - sum dL_dv (- h sum dL_dxfixed with attachments, whose targets move by w h), all from the oracle's is_start = 1 step.
    (g_x is the adjoint's carried gradient, which stands for dL/dx_new + g_v / h: dx = u m - g_v / h takes the g_v term out again, so no
    separate sum of g_v appears. On the oracle alone this expression equals the sum of c_i over ALL vertices to rounding, in every scene of this
    file; with a further + sum g_v it does not, by the size of sum g_v. Since it holds to rounding on the oracle alone, gating the engine's sum
    over the groups against it asks nothing the per-group gates do not already ask: it is kept as the statement of what the sum MEANS.)"""
    rb = sc.ref[s][b]["bwd"][1]
    t = H * sc.gx[s, b].reshape(-1, 3).sum(axis=0) - rb["dL_dv"].reshape(-1, 3).sum(axis=0)
    if sc.att:
        t = t - H * rb["dL_dxfixed"].reshape(-1, 3).sum(axis=0)
    return t


@pytest.mark.parametrize("name", ["two_reachable", "attached"])
def test_groups_moving_together_sum_to_the_frame_derivative(name):
    sc = scene(name)
    e = sc.engine()
    sc.m3 = mass3(e)
    start_batch(sc, e)
    lines = []
    for s in range(sc.steps):
        got = forward_step(sc, e, s)
        check_forward(sc, got, s, lines)
        check_backward(sc, e, got, s, 0, lines)
        _, dw = check_backward(sc, e, got, s, 1, lines)
        for b in range(sc.nb):
            want, _ = sc.expected_dw(s, b)
            assert all(q[1] > 0 for q in want), (s, b, want)               # every group is touched
            tot, scale = total_identity(sc, s, b), sum(q[1] for q in want)
            err = np.linalg.norm(dw[b].sum(axis=0) - tot)
            lines.append(f"    sum over groups {dw[b].sum(axis=0)} frame derivative {tot} |diff| {err:.2e} scale {scale:.2e}")
            assert err <= 1e-4 * scale, lines[-1]
    print(f"\n[primitive velocities, scene {name}]\n" + "\n".join(lines))
    e.close()


# ---- 5. bit-for-bit statements on the engine alone ----
def collect(e, nsteps, grads=True):
    x, v = e.get_states(0, nsteps + 1)
    out = dict(x=x, v=v, grp=[], nrm=[], f=[], r=[])
    for s in range(nsteps):
        g, n = e.get_contacts(s + 1)
        f, r = e.get_record(s + 1)
        out["grp"].append(g); out["nrm"].append(n); out["f"].append(f); out["r"].append(r)
    return out


def same(a, b):
    for k in ("x", "v"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for k in ("grp", "nrm", "f", "r"):
        for p, q in zip(a[k], b[k]):
            np.testing.assert_array_equal(p, q, err_msg=k)
    for k in ("dx", "dv", "dmu", "dw"):
        if k in a and k in b:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def lowered_state(V, nb):
    N = V.shape[0]
    X0 = np.stack([f32(V.reshape(-1) + np.tile([0.0, -0.03 * b, 0.0], N)) for b in range(nb)])      # (lowered: contacts from the first step)
    return X0


def check_zero_unset_schedule_and_reset(nx, cluster, monkeypatch):
    """all-zero velocities = never-set velocities (states, records, gradients); a schedule = per-step calls with dc_set_primitive_velocities,
    fused and per step; NULL, dc_clear_schedules and dc_alloc_batch put the never-set result back"""
    if cluster:
        monkeypatch.setenv("DC_CLUSTER", str(cluster))
    V, F, c, e = po.base_scene(nx, tight=(nx == 17))
    N = V.shape[0]
    e.alloc_batch(B, S)
    assert e.cluster() == (cluster if cluster else 1)
    rng = np.random.default_rng(5)
    X0 = lowered_state(V, B)
    Ws = np.stack([W1 * (0.25 * (s + 1)) for s in range(S)])             # [S][B][1][3], another velocity in every step
    V0 = np.zeros_like(X0)
    gx = f32(rng.standard_normal((B, 3 * N))); gv = f32(0.01 * rng.standard_normal((B, 3 * N)))

    def run(fused, per_step_w=None, grads=False):
        e.set_state(0, X0, V0)
        if fused:
            e.rollout_forward(0, S)
        else:
            for s in range(S):
                if per_step_w is not None:
                    e.set_primitive_velocities(per_step_w[s])
                e.step_forward(s)
        out = collect(e, S)
        if grads:
            if fused:
                e.set_gradient(gx, gv)
                e.rollout_backward(S, S)
                out["dx"], out["dv"], out["dmu"] = e.get_gradient()
            else:
                cx, cv, dmu = gx, gv, np.zeros((B, 1))
                for s in range(S, 0, -1):
                    o = e.step_backward(s, cx, cv, is_start=(s == 1))
                    cx, cv = o["dL_dx"], o["dL_dv"]
                out["dx"], out["dv"] = cx, cv
        return out

    never_f, never_s = run(True, grads=True), run(False, grads=True)
    assert all((g >= 0).sum() > 10 for g in never_s["grp"])
    with pytest.raises(capi.DcError, match="no primitive velocity has been set"):
        e.get_primitive_velocity_gradients(1, S)
    # zeros = never set
    e.set_primitive_velocities(np.zeros((B, 1, 3)))
    same(run(True, grads=True), never_f); same(run(False, grads=True), never_s)
    assert np.all(e.get_primitive_velocities(S) == 0)
    # a schedule = per-step calls
    a = run(False, per_step_w=Ws, grads=True)
    a["dw"] = e.get_primitive_velocity_gradients(1, S)
    for s in range(S):
        np.testing.assert_array_equal(e.get_primitive_velocities(s + 1), f32(Ws[s]))
    assert np.abs(a["x"][S] - never_s["x"][S]).max() > 1e-4 and np.abs(a["dw"]).max() > 0
    e.set_primitive_velocities(None)
    e.set_primitive_velocity_schedule(0, Ws)
    b_s = run(False, grads=True)
    b_s["dw"] = e.get_primitive_velocity_gradients(1, S)
    same(b_s, a)
    b_f = run(True, grads=True)
    same(b_f, dict(x=a["x"], v=a["v"], grp=a["grp"], nrm=a["nrm"], f=a["f"], r=a["r"]))
    dwf = e.get_primitive_velocity_gradients(1, S)
    print(f"\n[primitive velocity schedule nx={nx} K={e.cluster()}] backward sweep vs per-step calls: dL_dx {rel(b_f['dx'], a['dx']):.2e} "
          f"dL_dv {rel(b_f['dv'], a['dv']):.2e} dL_dw {rel(dwf, a['dw']):.2e}")
    assert rel(b_f["dx"], a["dx"]) <= 2e-6 and rel(b_f["dv"], a["dv"]) <= 2e-6 and rel(dwf, a["dw"]) <= 2e-6
    same(dict(run(True, grads=True), dw=e.get_primitive_velocity_gradients(1, S)), dict(b_f, dw=dwf))      # the sweep is bit-reproducible
    # a schedule over part of a fused sweep is an error
    e.clear_schedules()
    e.set_primitive_velocity_schedule(0, Ws[:2])
    with pytest.raises(capi.DcError, match="covers only part"):
        e.rollout_forward(0, S)
    # clear_schedules, NULL: the never-set result
    e.clear_schedules()
    same(run(True, grads=True), never_f); same(run(False, grads=True), never_s)
    e.set_primitive_velocities(Ws[1])
    assert np.abs(run(True)["x"][S] - never_f["x"][S]).max() > 1e-4
    e.set_primitive_velocities(None)
    same(run(True), never_f)
    # a fresh alloc_batch drops velocities and schedule, and the table itself
    e.set_primitive_velocities(Ws[1]); e.set_primitive_velocity_schedule(0, Ws[:2])
    e.alloc_batch(B, S)
    same(run(False), never_s); same(run(True), never_f)
    with pytest.raises(capi.DcError, match="no primitive velocity has been set"):
        e.get_primitive_velocity_gradients(1, S)
    e.close()


@pytest.mark.parametrize("nx,cluster", [(17, 0), (48, 4)])
def test_zero_unset_schedule_and_reset(nx, cluster, monkeypatch):
    check_zero_unset_schedule_and_reset(nx, cluster, monkeypatch)


def test_no_primitives_nothing_to_move():
    V, F = meshes.grid_cloth(5, 5, 4.5, 4.5, "DOWN")
    e = make_engine(f32(V), F, [])
    e.alloc_batch(1, 1)
    with pytest.raises(capi.DcError, match="no primitives"):
        e.set_primitive_velocities(np.zeros((1, 1, 3)))
    e.close()


@pytest.mark.parametrize("name", ["DC_DENSE_MAX_N", "DC_WINDOWS"])
def test_kernel_families_selected_at_build(name, monkeypatch):
    """DC_DENSE_MAX_N=0: the packet kernel's PCG instead of the explicit inverse small meshes get; DC_WINDOWS=0: the global-memory corner passes
    (resident kernel). Both are read at dc_build."""
    monkeypatch.setenv(name, "0")
    sc = scene("base")
    e = sc.engine()
    lay = e.layout()
    assert not (lay["dense_inverse"] if name == "DC_DENSE_MAX_N" else lay["element_windows"])
    e.close()
    run_parity("base", backward=False)


@pytest.mark.parametrize("name", ["DC_DENSE_MAX_N", "DC_WINDOWS"])
def test_gradients_under_the_kernel_families_selected_at_build(name, monkeypatch):
    """the records those forward kernels leave, differentiated: two steps, backward and injected checks. DC_WINDOWS=0 also puts the one adjoint
    instance without element windows under a velocity table."""
    monkeypatch.setenv(name, "0")
    run_parity("base", steps=2, backward=True)


@pytest.mark.parametrize("variant", ["global", "0", "1"])
def test_kernel_families_selected_per_process(variant):
    """DC_FWD_VARIANT is read once per process by the launchers: the forward parity in a child process per value"""
    env = dict(os.environ)
    env["DC_FWD_VARIANT"] = variant
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k",
                        "test_forward_parity_alone or test_the_scene_can_see_the_term"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0, f"DC_FWD_VARIANT={variant}:\n{tail}\n{r.stderr[-2000:]}"
    assert "2 passed" in tail and "failed" not in tail, tail


def test_forward_parity_alone():
    run_parity("base", backward=False)


def test_device_pointer_setters_and_getters_match_the_host_ones():
    V, F, c, e = po.base_scene(tight=False)
    N = V.shape[0]
    e.alloc_batch(B, S)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(8)
    X0 = lowered_state(V, B)
    gx = f32(rng.standard_normal((B, 3 * N))); gv = f32(0.01 * rng.standard_normal((B, 3 * N)))
    for Ws in (np.stack([W1 * (0.25 * (s + 1)) for s in range(S)]), 0.7 * rng.standard_normal((S, B, 1, 3))):      # dyadic, and no fp32 numbers
        for dtype in (torch.float32, torch.float64):
            Wh = f32(Ws) if dtype == torch.float32 else Ws
            V0 = np.stack([f32(np.tile(Wh[0, b, 0], N)) for b in range(B)])
            e.alloc_batch(B, S)
            e.set_state(0, X0, V0)
            e.set_primitive_velocity_schedule(0, Wh)
            e.rollout_forward(0, S)
            host = collect(e, S)
            hw = np.stack([e.get_primitive_velocities(s + 1) for s in range(S)])
            np.testing.assert_array_equal(hw, f32(Wh))
            e.set_gradient(gx, gv); e.rollout_backward(S, S)
            hdw = e.get_primitive_velocity_gradients(1, S)
            assert np.abs(hdw).max() > 0
            wide = torch.zeros((S, B, 1, 6), dtype=dtype, device=dev)
            wide[..., :3] = torch.as_tensor(Wh, dtype=dtype)
            for t in (torch.as_tensor(Wh, dtype=dtype).to(dev), wide[..., :3]):    # contiguous, and a strided view the wrapper copies
                e.alloc_batch(B, S)
                e.set_state(0, X0, V0)
                e.set_primitive_velocity_schedule_dev(0, S, t)
                e.rollout_forward(0, S)
                same(collect(e, S), host)
                np.testing.assert_array_equal(np.stack([e.get_primitive_velocities(s + 1) for s in range(S)]), hw)
                e.set_gradient(gx, gv); e.rollout_backward(S, S)
                out = torch.full((S, B, 1, 3), 7.0, dtype=dtype, device=dev)
                e.get_primitive_velocity_gradients_dev(1, S, out)
                e.sync()
                np.testing.assert_array_equal(out.cpu().numpy().astype(np.float64), hdw)      # (fp32 values: exact in either dtype)
            # the velocities of the NEXT steps
            e.clear_schedules()
            e.set_state(0, X0, V0)
            e.set_primitive_velocities_dev(torch.as_tensor(Wh[1], dtype=dtype).to(dev))
            e.step_forward(0)
            np.testing.assert_array_equal(e.get_primitive_velocities(1), hw[1])
            xa, _ = e.get_state(1)
            e.set_primitive_velocities_dev(None)
            e.step_forward(0)
            assert np.all(e.get_primitive_velocities(1) == 0) and np.abs(e.get_state(1)[0] - xa).max() > 1e-6
            e.set_primitive_velocities(Wh[1])
            e.step_forward(0)
            np.testing.assert_array_equal(e.get_state(1)[0], xa)
    e.close()


def test_self_collision_layers_under_a_moving_sphere(monkeypatch):
    """the flap scene of tests/test_gpu_primitive_offsets.py, frame-shifted: cloth at (x, v + w), sphere moving at w. The primitive contacts seed
    the layering, so the self-contact lists (pairs, layers) equal the static run's only when detection and step kernel saw the same velocity row;
    per-step path and fused sweep (detection inlined)."""
    monkeypatch.setenv("DC_CLUSTER", "1")
    cfg = workloads.C4_CLOTH
    V, F, Vf, flap, c = workloads.c4_scene(grid=16, fold_rows=3, fold_gap=0.02)
    N = V.shape[0]
    fabric = dict(density=cfg["density"], k_stretch=cfg["k_stretch"], k_bend=cfg["k_bend"])
    prim = dict(kind=capi.DC_PRIM_SPHERE, group=0, center=c, radius=cfg["sphere_radius"], mu=cfg["sphere_mu"])
    to_flap = Vf[flap].mean(axis=0) - c
    nb = 2
    D = np.zeros((nb, 1, 3))
    D[:, 0] = np.round(np.array([to_flap[0], 0.0, to_flap[2]]) * 32) / 32 + np.array([0.0, 0.125, 0.0])        # the sphere's top under the flap
    W = np.array([[[0.0, 0.0, 0.0]], [[0.5, 0.25, -0.125]]])
    X0 = np.tile(f32(Vf.reshape(-1)), (nb, 1))
    V0 = np.stack([f32(np.tile(W[b, 0], N)) for b in range(nb)])
    e = make_engine(V, F, [prim], selfcollision=1, fabric=fabric)
    e.alloc_batch(nb, 1)
    e.set_primitive_offsets(D)
    e.set_primitive_velocities(W)
    lists = []
    for fused in (False, True):
        e.set_state(0, X0, V0)
        if fused:
            e.set_primitive_velocity_schedule(0, W[None])
            e.rollout_forward(0, 1)
        else:
            e.step_forward(0)
        grp, _ = e.get_contacts(1)
        x, _ = e.get_state(1)
        sc = [e.get_self_contacts(1, rollout=b) for b in range(nb)]
        lists.append((grp.copy(), sc, x))
    for grp, sc, x in lists:
        np.testing.assert_array_equal(grp[1], grp[0])                                   # the same primitive contacts in both frames
        assert sc[0]["count"] == sc[1]["count"] >= 10 and sc[0]["layers"] == sc[1]["layers"]
        np.testing.assert_array_equal(sc[0]["pairs"], sc[1]["pairs"]); np.testing.assert_array_equal(sc[0]["layer"], sc[1]["layer"])
        assert (grp[0] >= 0).sum() >= 5
        assert np.abs(x[1] - np.tile(W[1, 0], N) * H - x[0]).max() <= GATE_X             # and the same step, shifted by w h
    np.testing.assert_array_equal(lists[0][0], lists[1][0])
    e.close()


# ---- 6. sim_rollout ----
def test_sim_rollout_takes_primitive_velocities_on_both_paths():
    """device path = host path; [B, G, 3] = [T, B, G, 3] repeated; primitive_velocities.grad = Engine.get_primitive_velocity_gradients (summed over
    the steps for the short form)"""
    V, F, c, e = po.base_scene(tight=False)
    N = V.shape[0]
    e.alloc_batch(B, S)
    sim = BatchedSim(e, S)
    rng = np.random.default_rng(4)
    x0 = lowered_state(V, B)
    Wc = W1 * 0.25
    v0 = np.stack([f32(np.tile(Wc[b, 0], N)) for b in range(B)])
    w = f32(1e-3 * rng.standard_normal((S, B, 3 * N)))

    def run(device, pv):
        t = lambda a, grad=False: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(device).requires_grad_(grad)
        tx, tw = t(x0, True), (None if pv is None else t(pv, True))
        xs, vs = sim_rollout(sim, tx, t(v0), None, steps=S, primitive_velocities=tw)
        (xs * t(w)).sum().backward()
        dw = e.get_primitive_velocity_gradients(1, S) if pv is not None else None
        return xs.detach().cpu().numpy(), vs.detach().cpu().numpy(), tx.grad.cpu().numpy(), (None if tw is None else tw.grad.cpu().numpy()), dw

    long = np.broadcast_to(Wc, (S, B, 1, 3)).copy()
    host, devc = run("cpu", long), run("cuda", long)
    np.testing.assert_array_equal(devc[0], host[0]); np.testing.assert_array_equal(devc[1], host[1])
    assert rel(devc[2], host[2]) <= 2e-6 and rel(devc[3], host[3]) <= 2e-6 and np.abs(host[3][:, :3]).max() > 0
    np.testing.assert_array_equal(host[3], host[4].astype(np.float32)); np.testing.assert_array_equal(devc[3], devc[4].astype(np.float32))
    short_h, short_d = run("cpu", Wc), run("cuda", Wc)
    np.testing.assert_array_equal(short_d[0], devc[0]); np.testing.assert_array_equal(short_h[0], host[0])
    assert rel(short_h[3], short_h[4].sum(axis=0)) <= 2e-6 and rel(short_d[3], short_d[4].sum(axis=0)) <= 2e-6      # (fp32 tensors: one rounding of the sum)
    none_d = run("cuda", None)                                                         # omitted: the schedule is cleared, the current velocities (zeros) apply
    assert np.abs(none_d[0] - devc[0]).max() > 1e-5
    e.close()


def test_sim_rollout_drags_the_cloth_with_offsets_and_velocities():
    """a sphere dragged under the cloth for four steps: offsets[s] = c(t_s) - c_built, velocities[s] = (c(t_{s+1}) - c(t_s)) / h. The contacts the
    oracle calls sticking are carried along — their mean tangential velocity is the sphere's — while the same run without velocities lets them slide
    over a sphere it believes at rest and brakes them by Coulomb friction."""
    V, F, c, e = po.base_scene(tight=False)
    N = V.shape[0]
    nb = 1
    e.alloc_batch(nb, S)
    sim = BatchedSim(e, S)
    wdrag = np.array([1.0, 0.0, 0.5])
    offs = np.stack([np.broadcast_to(np.array([0.0, 0.125, 0.0]) + wdrag * H * s, (nb, 1, 3)) for s in range(S)])      # c(t_s) - c_built
    vels = np.broadcast_to(wdrag, (S, nb, 1, 3)).copy()
    x0 = f32(V.reshape(1, -1)); v0 = f32(np.tile(wdrag, N).reshape(1, -1))            # the cloth rides on the sphere: at rest in ITS frame
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()
    xs_w, vs_w = sim_rollout(sim, t(x0), t(v0), None, steps=S, primitive_offsets=t(offs), primitive_velocities=t(vels))
    sim.check_episode()
    grp = e.get_contacts(S)[0][0]
    np.testing.assert_array_equal(np.stack([e.get_primitive_centers(s + 1)[:, 0] for s in range(S)]), f32(c + offs[:, :, 0]))
    xs_0, vs_0 = sim_rollout(sim, t(x0), t(v0), None, steps=S, primitive_offsets=t(offs))
    sim.check_episode()
    # the oracle's contact types of the last step, from the engine's state before it, in the sphere's frame
    o = orc.Oracle(V, F, h=H, fwd_tol=1e-7, bwd_tol=1e-7, selfcollision=False, gradient_clipping=False, **FABRIC)
    o.add_sphere(f32(c + offs[S - 1, 0, 0]), 2.0, 0.4)
    o.build()
    ref = o.step(xs_w[S - 2, 0].cpu().numpy(), vs_w[S - 2, 0].cpu().numpy() - np.tile(wdrag, N))
    pc = o.prim_contacts(ref["id"])
    stick = pc["particle"][pc["type"] == 1]
    assert len(stick) >= 3 and set(stick.tolist()) <= set(contact_ids(grp).tolist())
    nrm = pc["normal"][pc["type"] == 1]

    def tangential(vs):
        v = vs[S - 1, 0].cpu().numpy().reshape(-1, 3)[stick]
        return (v - nrm * (v * nrm).sum(axis=1)[:, None]).mean(axis=0)

    wt = (wdrag - nrm * (nrm @ wdrag)[:, None]).mean(axis=0)
    with_w, without = tangential(vs_w), tangential(vs_0)
    print(f"\n[dragged sphere] {len(stick)} sticking contacts: mean tangential velocity with velocities {with_w}, without {without}, the sphere's {wt}")
    # a sticking contact has no velocity relative to the obstacle: carried along to the forward gate (5e-5 in x is 5e-5 / h in v). Under the static
    # law the same vertices pass over a sphere believed at rest at |w|, far above mu |d_N| / m: they SLIDE (they are not braked to rest), and a
    # sliding contact that carries the cloth's weight loses at least mu g h of tangential velocity in one step — more than twice the gate above
    assert np.linalg.norm(with_w - wt) <= GATE_X / H
    assert np.dot(wt - without, wt) / np.linalg.norm(wt) >= 0.4 * 9.8 * H
    e.close()
