"""Spinning obstacles: an angular velocity per rollout, primitive group and step (dc_set_primitive_spins, dc_set_primitive_spin_schedule, their
_dev forms, dc_get_primitive_spins, dc_get_primitive_spin_gradients; sim_rollout(primitive_spins=...)).

The rule under test (include/diffcloth_hip.h): a DC_PRIM_SPHERE of a group with omega != 0 adds v_spin = radius (omega x n) to the obstacle's
velocity in the friction law, d = ((f - v_rot m) - w m) - v_spin m, forward and adjoint, and every backward step leaves
dL/domega = -h sum m_i radius (n_i x g_i). The fp64 oracle's `rotates` sphere — surface velocity 8 (y^ x n) whatever its radius — is the exact
partner of a PLAIN engine sphere with omega = (0, 8 / radius, 0): the scenes, the teacher forcing from the oracle's state, the Galilean partner
in w and the gates are those of tests/test_gpu_primitive_velocities.py, whose helpers this file imports.
The cloth LANDS on the sphere (LandingScene below says why a cloth at rest cannot show the term to 100 gates).
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
import test_gpu_primitive_offsets as po
import test_gpu_primitive_velocities as pv          # its Scene, make_engine, step helpers and gates (helpers, not tests)
from diffcloth_amd import capi, workloads
from diffcloth_amd.functional import BatchedSim, sim_rollout

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, GATE_X, f32, rel = pv.H, pv.GATE_X, pv.f32, pv.rel
GATE_B = 1e-4          # the backward gate of pv.check_backward / pv.check_injected (BASELINE.json's flat 1e-4)
DW_RTOL = 1e-4         # pv.check_backward's rule for dL/dw, applied to dL/domega as it stands there: |diff| <= 1e-4 * sum_i |c_i|
SURFACE_SPEED = 8.0    # the reference's rotating sphere: v_rot = 8 (y^ x n), Primitive.cpp:254-257


def spin_of(radius):
    return np.array([0.0, SURFACE_SPEED / radius, 0.0])


def plain_prims(sc):
    """the scene's spheres WITHOUT the reference's rotates flag: the engine gets the spin through the new entries"""
    return [pv.sphere(c, group=g, rotates=0) for g, (c, rot) in enumerate(sc.spheres)]


def spins_for(sc, idle=(0.0, 0.0, 0.0)):
    """[B][G][3]: omega = (0, 8 / radius, 0) for every sphere the ORACLE rotates, `idle` for the others"""
    om = np.zeros((sc.nb, sc.G, 3))
    for g, (c, rot) in enumerate(sc.spheres):
        om[:, g] = spin_of(sc.prims[g]["radius"]) if rot else idle
    return om


FALL = np.array([0.0, -6.0, 0.0])


class LandingScene(pv.Scene):
    """pv.Scene with the cloth LANDING on the spheres at `fall` (in the static frame) instead of starting from rest; everything else — the
    teacher forcing from the oracle's state, the Galilean partner w, the attributes the helpers of that file read — is that class's. A cloth that
    rests on a sphere is pressed on by its weight alone: Coulomb friction then moves it by at most mu g h^2 = 1.2e-4 per step whatever the
    surface does, and a step without the spin misses by just that. A cloth that lands at 6 is stopped by the normal impulse m (6 + g h), friction
    may take mu times that, and the oracle's static and rotating spheres are 7.9e-3 ... 1.0e-2 apart after ONE step from the same state
    (measured on the oracle alone, every rollout and step of this scene): more than 100 forward gates."""

    def __init__(self, spheres, W, D, steps=2, fall=FALL, nx=17, threads=1):
        self.V, self.F = meshes.grid_cloth(nx, nx, 4.5, 4.5, "DOWN")
        self.V = f32(self.V)
        self.N = N = self.V.shape[0]
        self.c0 = f32(meshes.sphere_scene_center(self.V, 2.0))
        self.spheres = [(f32(self.c0 + np.asarray(d)), rot) for d, rot in spheres]
        self.G = len(self.spheres)
        self.W, self.D, self.att, self.steps = np.asarray(W, dtype=np.float64), np.asarray(D, dtype=np.float64), (), steps
        self.nb = self.W.shape[0]
        self.prims = [pv.sphere(c, group=g, rotates=rot) for g, (c, rot) in enumerate(self.spheres)]
        rng = np.random.default_rng(31)
        self.gx = f32(rng.standard_normal((steps, self.nb, 3 * N)))
        self.gv = f32(0.01 * rng.standard_normal((steps, self.nb, 3 * N)))
        self.wf = self.W[:, 0, :]
        self.oracles = []
        self.ref = [[None] * self.nb for _ in range(steps)]
        self.Xe = np.zeros((steps, self.nb, 3 * N)); self.Ve = np.zeros_like(self.Xe)
        self.XFe = np.zeros((steps, self.nb, 0))
        for b in range(self.nb):
            o = orc.Oracle(self.V, self.F, h=H, fwd_tol=1e-9, bwd_tol=1e-9, selfcollision=False, gradient_clipping=False, threads=threads, **pv.FABRIC)
            for g, (c, rot) in enumerate(self.spheres):
                o.add_sphere(f32(c + self.D[b, g]), self.prims[g]["radius"], self.prims[g]["mu"], rotates=bool(rot))
            o.build()
            self.oracles.append(o)
            wt = np.tile(self.wf[b], N)
            x = f32(self.V.reshape(-1)); ve = f32(np.tile(fall, N) + wt)          # landing at `fall` in the static frame
            for s in range(steps):
                self.Xe[s, b], self.Ve[s, b] = x, ve
                r = o.step(x, ve - wt, None)
                r["pc"] = o.prim_contacts(r["id"])
                r["f"] = o.record_fr(r["id"])[0]
                r["bwd"] = {st: o.step_backward(r["id"], self.gx[s, b], self.gv[s, b], is_start=bool(st), direct=True) for st in (0, 1)}
                self.ref[s][b] = r
                x = f32(r["x"]); ve = f32(r["v"] + wt)


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "rotating":                    # one rotating sphere, three rollouts with their own centre offset and w (those of that file)
        return LandingScene([((0, 0, 0), 1)], pv.W1[:3], pv.D1[:3])
    if name == "static":
        return pv.scene("base")
    if name == "two_one_reachable":           # group 0 rotates under the cloth, group 1 far below: never in contact
        return LandingScene([((0, 0.125, 0), 1), ((0, -6, 0), 0)], np.concatenate([pv.W1[:3], pv.W1[:3][::-1]], axis=1), np.zeros((3, 2, 3)))
    raise KeyError(name)


def start(sc, e, om, velocities=True):
    e.alloc_batch(sc.nb, sc.steps)
    if np.abs(sc.D).max() > 0:
        e.set_primitive_offsets(sc.D)
    if velocities:
        e.set_primitive_velocities(sc.W)
    if om is not None:
        e.set_primitive_spins(om)


def expected_dom(sc, s, b):
    """per group: (sum_i radius (n_i x c_i) over the oracle's contacts with it, sum_i |c_i|), c_i and n_i the oracle's (pv.Scene.expected_dw)"""
    want, ci = sc.expected_dw(s, b)
    pc = sc.ref[s][b]["pc"]
    out = []
    for g in range(sc.G):
        sel = pc["prim"] == g
        out.append((sc.prims[g]["radius"] * np.cross(pc["normal"][sel], ci[pc["particle"][sel]]).sum(axis=0), want[g][1]))
    return out


def check_dom(sc, dom, s, lines, tag=""):
    for b in range(sc.nb):
        want = expected_dom(sc, s, b)
        for g in range(sc.G):
            err = np.linalg.norm(dom[b, g] - want[g][0])
            lines.append(f"    {tag}dL/domega[{g}] rollout {b} engine {dom[b, g]} oracle {want[g][0]} |diff| {err:.2e} scale {want[g][1]:.2e}")
            assert err <= DW_RTOL * want[g][1], lines[-1]
            if want[g][1] == 0.0:
                assert np.all(dom[b, g] == 0.0), lines[-1]          # a group nothing touches: exactly zero


def run_parity(name, mode=1, steps=None, backward=True, inject=True, prims=None, om=None):
    sc = scene(name)
    om = spins_for(sc) if om is None else om
    e = pv.make_engine(sc.V, sc.F, plain_prims(sc) if prims is None else prims, att=sc.att, mode=mode)
    sc.m3 = pv.mass3(e)
    start(sc, e, om)
    lines = []
    for s in range(sc.steps if steps is None else steps):
        got = pv.forward_step(sc, e, s)
        np.testing.assert_array_equal(e.get_primitive_spins(s + 1), f32(om))
        np.testing.assert_array_equal(e.get_primitive_velocities(s + 1), f32(sc.W))
        pv.check_forward(sc, got, s, lines)
        for b in range(sc.nb):                                       # PD iteration counts, per rollout and step
            assert abs(int(got["st"]["pd_iters"][b]) - sc.ref[s][b]["iters"]) <= 1, lines[-sc.nb + b]
        if backward:
            for is_start in (s % 2, 1 - s % 2):
                pv.check_backward(sc, e, got, s, is_start, lines, gate=GATE_B)      # dL_dx, dL_dv, dL_dmu, dL/dw: end to end and on the engine's record
                if is_start:
                    check_dom(sc, e.get_primitive_spin_gradients(s + 1, 1)[0], s, lines)
            if inject:                                               # the oracle's record handed in: its spin row from a one-step schedule at s
                e.set_primitive_spin_schedule(s, om[None])
                pv.check_injected(sc, e, s, s % 2, lines)
                if s % 2:
                    check_dom(sc, e.get_primitive_spin_gradients(s + 1, 1)[0], s, lines, tag="injected ")
    print(f"\n[primitive spins, scene {name}, adjoint_mode {mode}]\n" + "\n".join(lines))
    e.close()
    return sc


# ---- 1. forward parity against the oracle's rotating sphere; 4. backward parity; 5. dL/domega ----
def test_forward_and_backward_parity_with_the_oracles_rotating_sphere():
    sc = run_parity("rotating", mode=1)
    assert all(sc.ref[s][b]["nprim"] >= 10 for s in range(sc.steps) for b in range(sc.nb))
    assert all(expected_dom(sc, s, b)[0][1] > 0 for s in range(sc.steps) for b in range(sc.nb))


@pytest.mark.parametrize("mode", [0, 2, 3])
def test_backward_parity_other_adjoint_modes(mode):
    run_parity("rotating", mode=mode, steps=1 if mode == 0 else None)


def test_forward_parity_alone():
    run_parity("rotating", backward=False)


def test_without_the_spin_the_step_misses_the_oracle():
    """the same plain sphere with no spin set: every rollout is in contact and misses the oracle's rotating sphere by more than 100 gates in
    every step (LandingScene says why the cloth has to land: a surface speed of 8 is 8 h = 0.044 per step only for a contact that sticks)"""
    sc = scene("rotating")
    e = pv.make_engine(sc.V, sc.F, plain_prims(sc))
    start(sc, e, None)
    lines = []
    for s in range(sc.steps):
        got = pv.forward_step(sc, e, s)
        for b in range(sc.nb):
            assert sc.ref[s][b]["nprim"] >= 10
            miss = np.abs(got["x"][b] - np.tile(sc.wf[b], sc.N) * H - sc.ref[s][b]["x"]).max()
            lines.append(f"step {s} rollout {b}: without the spin max|x - w h - x_oracle| {miss:.2e}")
            assert miss > 100 * GATE_X, lines[-1]
    print("\n[primitive spins unset]\n" + "\n".join(lines))
    with pytest.raises(capi.DcError, match="no primitive spin has been set"):
        e.get_primitive_spin_gradients(1, 1)
    e.close()


def test_two_groups_one_out_of_reach_its_gradient_is_exactly_zero():
    sc = scene("two_one_reachable")
    run_parity("two_one_reachable", inject=False, om=spins_for(sc, idle=(1.0, -2.0, 3.0)))
    assert all(expected_dom(sc, s, b)[1][1] == 0.0 and expected_dom(sc, s, b)[0][1] > 0 for s in range(sc.steps) for b in range(sc.nb))


# ---- 3. another magnitude: rotates and omega add ----
def test_rotates_flag_and_opposite_spin_cancel_to_the_static_sphere():
    """an engine sphere with rotates = 1 and omega = (0, -8 / radius, 0) against the oracle's STATIC sphere"""
    sc = scene("static")
    om = np.broadcast_to(-spin_of(2.0), (sc.nb, 1, 3)).copy()
    run_parity("static", steps=2, inject=False, prims=[pv.sphere(c, group=g, rotates=1) for g, (c, rot) in enumerate(sc.spheres)], om=om)


# ---- 2. other axes by turning the world; 3. radius 2.5 ----
CYC = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
TURNS = {"identity_r25": (np.eye(3), 2.5), "cyclic": (CYC, 2.0), "cyclic2": (CYC @ CYC, 2.0), "half_turn": (np.diag([1.0, -1.0, -1.0]), 2.0),
         "rot345": (np.array([[1.0, 0.0, 0.0], [0.0, 0.6, -0.8], [0.0, 0.8, 0.6]]), 2.0)}
GRAVITY = np.array([0.0, -9.8, 0.0])
TSTEPS = 2


@functools.lru_cache(maxsize=None)
def turned(name):
    """The engine's world is Q . the oracle's. The engine's inputs are fp32 (mesh, centre, omega, states, incoming gradients); the oracle
    receives Q^T . those, in fp64 — for the permutations and the half turn that is its own unturned world exactly, so they share one run."""
    Q, radius = TURNS[name]
    exact = bool(np.all(np.isin(Q, (-1.0, 0.0, 1.0))))
    if exact and name != "cyclic" and radius == 2.0:
        base = turned("cyclic")
        return dict(base, Q=Q)
    V0, F = meshes.grid_cloth(17, 17, 4.5, 4.5, "DOWN")
    V0 = f32(V0)
    N = V0.shape[0]
    c0 = f32(f32(meshes.sphere_scene_center(V0, radius)) + pv.D1[0, 0])
    Qo = np.eye(3) if exact else Q                       # what the oracle's world is turned by to give the engine's fp32 inputs
    Ve, ce = f32(V0 @ Qo.T), f32(Qo @ c0)
    Vo, co = Ve @ Qo, Qo.T @ ce
    o = orc.Oracle(Vo, F, h=H, fwd_tol=1e-9, bwd_tol=1e-9, selfcollision=False, gradient_clipping=False, **pv.FABRIC)
    o.add_sphere(co, radius, 0.4, rotates=True)
    o.build()
    rng = np.random.default_rng(17)
    tq = lambda a, M: (a.reshape(-1, 3) @ M.T).reshape(-1)          # rows turned by M
    gxe = [f32(tq(f32(rng.standard_normal(3 * N)), Qo)) for _ in range(TSTEPS)]
    gve = [f32(tq(f32(0.01 * rng.standard_normal(3 * N)), Qo)) for _ in range(TSTEPS)]
    xe, ve = f32(Ve.reshape(-1)), f32(tq(np.tile(FALL, N), Qo))      # landing, as in LandingScene
    ref = []
    for s in range(TSTEPS):
        r = o.step(tq(xe, Qo.T), tq(ve, Qo.T))
        r["pc"] = o.prim_contacts(r["id"])
        r["xe"], r["ve"] = xe, ve                                    # the engine's state before the step, in ITS (Qo) world
        r["gx"], r["gv"] = tq(gxe[s], Qo.T), tq(gve[s], Qo.T)
        r["bwd"] = o.step_backward(r["id"], r["gx"], r["gv"], is_start=True, direct=True)
        ref.append(r)
        xe, ve = f32(tq(r["x"], Qo)), f32(tq(r["v"], Qo))
    return dict(Q=Q, Qo=Qo, radius=radius, V0=V0, F=F, c0=c0, N=N, ref=ref, exact=exact)


@pytest.mark.parametrize("name", sorted(TURNS))
def test_other_axes_by_turning_the_world(name):
    t = turned(name)
    Q, N, radius = t["Q"], t["N"], t["radius"]
    # for an exact Q the shared oracle run is the unturned world (Qo = 1): the engine's inputs are Q . fp32 values, still fp32 exactly
    R = Q if t["exact"] else np.eye(3)                   # what is still to be applied to the stored (Qo-world) engine inputs
    tq = lambda a, M: (np.asarray(a).reshape(-1, 3) @ M.T).reshape(-1)
    Qfull = R @ t["Qo"]
    Ve, ce = f32(t["V0"] @ Qfull.T), f32(Qfull @ t["c0"])
    om = f32(Qfull @ spin_of(radius))
    e = capi.Engine(0)
    e.set_mesh(Ve, t["F"])
    e.set_attachments(())
    e.set_params(time_step=H, cg_max_iter=2000, gradient_clipping=0, selfcollision_enabled=0, adjoint_mode=1, gravity=tuple(Qfull @ GRAVITY),
                 forward_tol=1e-9, backward_tol=1e-9, cg_rel_tol=1e-6, adjoint_rel_tol=1e-8, **pv.FABRIC)
    e.set_primitives([dict(kind=capi.DC_PRIM_SPHERE, group=0, center=ce, radius=radius, mu=0.4, rotates=0)])
    e.build()
    e.alloc_batch(1, TSTEPS)
    e.set_primitive_spins(om.reshape(1, 1, 3))
    lines = []
    for s, r in enumerate(t["ref"]):
        e.set_state(s, tq(r["xe"], R)[None], tq(r["ve"], R)[None])
        st = e.step_forward(s)
        x1, v1 = e.get_state(s + 1)
        grp, nrm = e.get_contacts(s + 1)
        ids = pv.contact_ids(grp[0])
        order = np.argsort(r["pc"]["particle"])
        assert st["converged"][0] == 1 and r["converged"] and r["nprim"] >= 10
        np.testing.assert_array_equal(ids, r["pc"]["particle"][order])
        np.testing.assert_allclose(tq(nrm[0], Qfull.T).reshape(-1, 3)[ids], r["pc"]["normal"][order], atol=2e-6)
        dx = np.abs(tq(x1[0], Qfull.T) - r["x"]).max()
        dv = np.abs(tq(v1[0], Qfull.T) - r["v"]).max()
        lines.append(f"{name} step {s}: contacts {r['nprim']}, PD iterations gpu {st['pd_iters'][0]} / oracle {r['iters']}, max|Q^T x - x_oracle| {dx:.2e}, "
                     f"max|Q^T v - v_oracle| {dv:.2e}")
        assert dx <= GATE_X and dv <= 2 * GATE_X / H, lines[-1]
        assert abs(int(st["pd_iters"][0]) - r["iters"]) <= 1, lines[-1]
        gb = e.step_backward(s + 1, tq(r["gx"], Qfull)[None], tq(r["gv"], Qfull)[None], is_start=True)
        rb = r["bwd"]
        ex, ev = rel(tq(gb["dL_dx"][0], Qfull.T), rb["dL_dx"]), rel(tq(gb["dL_dv"][0], Qfull.T), rb["dL_dv"])
        em = records.mu_err(gb["dL_dmu"][0], rb["dL_dmu"])
        ci = (H * rb["dL_dx"] + r["gv"] - rb["dL_dv"]).reshape(-1, 3)
        pc = r["pc"]
        want = Qfull @ (radius * np.cross(pc["normal"], ci[pc["particle"]]).sum(axis=0))
        scale = float(np.linalg.norm(ci[pc["particle"]], axis=1).sum())
        dom = e.get_primitive_spin_gradients(s + 1, 1)[0, 0, 0]
        err = np.linalg.norm(dom - want)
        lines.append(f"  backward: dL_dx {ex:.2e} dL_dv {ev:.2e} dL_dmu {em:.2e}; dL/domega engine {dom} oracle (turned) {want} |diff| {err:.2e} scale {scale:.2e}")
        assert ex <= GATE_B and ev <= GATE_B and em <= GATE_B, lines[-1]
        assert err <= DW_RTOL * scale, lines[-1]
    print("\n[primitive spins, turned world]\n" + "\n".join(lines))
    e.close()


# ---- 5. a LowerLeg group: the capsule children contribute nothing, the sphere child does ----
def test_lower_leg_group_only_its_sphere_child_spins():
    """the LowerLeg of po.leg_scene (joint sphere, foot capsule, leg capsule: one group, one omega) under a sheet around the foot capsule
    (rollout 0) and at the joint (rollout 1). Children are tested in order and the sphere is the first, so a vertex within the sphere's contact
    shell is the sphere's contact and every other contact a capsule's. With c_i = h dL_dx_i + g_v,i - dL_dv_i of the SAME backward step
    (= -h m_i g_i, pv.Scene.expected_dw), dL/domega is radius sum (n_i x c_i) over the sphere's contacts alone; a rollout whose contacts are all
    on capsules takes the never-set step bit for bit and has dL/domega exactly zero."""
    V, F, center, prims = po.leg_scene()
    N = V.shape[0]
    mid = V.mean(axis=0)
    X0 = np.stack([f32((V + (center + np.array([0.0, height, 0.0]) - mid)).reshape(-1)) for height in (2.0, 4.1)])
    V0 = np.zeros_like(X0)
    om = np.broadcast_to(np.array([0.5, 2.0, -1.0]), (2, 1, 3)).copy()
    rng = np.random.default_rng(3)
    gx = f32(rng.standard_normal((2, 3 * N))); gv = f32(0.01 * rng.standard_normal((2, 3 * N)))
    assert prims[0]["kind"] == capi.DC_PRIM_SPHERE and all(p["kind"] == capi.DC_PRIM_CAPSULE for p in prims[1:])
    radius, cs = float(prims[0]["radius"]), np.asarray(prims[0]["center"], dtype=np.float64)

    def run(spin):
        e = pv.make_engine(V, F, prims)
        e.alloc_batch(2, 1)
        if spin is not None:
            e.set_primitive_spins(spin)
        e.set_state(0, X0, V0)
        e.step_forward(0)
        grp, nrm = e.get_contacts(1)
        gb = e.step_backward(1, gx, gv, is_start=True)
        out = dict(x=e.get_state(1)[0], grp=grp, nrm=nrm, dx=gb["dL_dx"], dv=gb["dL_dv"],
                   dom=None if spin is None else e.get_primitive_spin_gradients(1, 1)[0])
        e.close()
        return out

    plain, spun = run(None), run(om)
    n_sphere = n_capsule = 0
    for b in range(2):
        np.testing.assert_array_equal(spun["grp"][b], plain["grp"][b])               # detection does not see the spin
        ids = pv.contact_ids(spun["grp"][b])
        assert len(ids) >= 8
        dist = np.linalg.norm(X0[b].reshape(-1, 3)[ids] - cs, axis=1) - radius      # (v = 0: all three samples are the vertex itself)
        assert np.all(np.abs(dist - 0.1) > 1e-4)                                    # nobody on the shell's edge: the classification is safe
        sph = ids[dist < 0.1]
        ci = (H * spun["dx"][b] + gv[b] - spun["dv"][b]).reshape(-1, 3)
        nb = spun["nrm"][b].reshape(-1, 3)
        want = radius * np.cross(nb[sph], ci[sph]).sum(axis=0)
        scale = float(np.linalg.norm(ci[ids], axis=1).sum())
        err = np.linalg.norm(spun["dom"][b, 0] - want)
        print(f"[LowerLeg] rollout {b}: {len(ids)} contacts, {len(sph)} on the joint sphere; dL/domega {spun['dom'][b, 0]} expected {want} "
              f"|diff| {err:.2e} scale {scale:.2e}")
        assert err <= DW_RTOL * scale
        n_sphere += len(sph); n_capsule += len(ids) - len(sph)
        if len(sph) == 0:
            np.testing.assert_array_equal(spun["x"][b], plain["x"][b])
            assert np.all(spun["dom"][b] == 0.0)
        else:
            assert np.abs(spun["x"][b] - plain["x"][b]).max() > 1e-6 and np.linalg.norm(want) > DW_RTOL * scale      # (there is something to see)
        if len(sph) < len(ids):                                                     # (what counting the capsule contacts too would have given)
            allc = radius * np.cross(nb[ids], ci[ids]).sum(axis=0)
            print(f"           with the capsule children's contacts counted: {allc}, {np.linalg.norm(allc - want):.2e} away")
    assert n_sphere > 0 and n_capsule > 0, (n_sphere, n_capsule)


# ---- 6. bit-for-bit statements on the engine alone ----
def check_zero_unset_schedule_and_reset(nx, cluster, monkeypatch):
    """all-zero spins = never-set spins, with and without a velocity table; a schedule = per-step calls, fused and per step; NULL,
    dc_clear_schedules and dc_alloc_batch put the never-set result back; a partial schedule refuses a fused sweep; two runs give one dL/domega"""
    if cluster:
        monkeypatch.setenv("DC_CLUSTER", str(cluster))
    B, S = pv.B, pv.S
    V, F, c, e = po.base_scene(nx, tight=(nx == 17))
    N = V.shape[0]
    e.alloc_batch(B, S)
    assert e.cluster() == (cluster if cluster else 1)
    rng = np.random.default_rng(5)
    X0 = pv.lowered_state(V, B)
    V0 = np.zeros_like(X0)
    OMs = np.stack([pv.W1 * (0.5 * (s + 1)) for s in range(S)])            # [S][B][1][3], another spin in every step (rollout 0: none)
    Ws = np.stack([pv.W1 * (0.25 * (s + 1)) for s in range(S)])
    gx = f32(rng.standard_normal((B, 3 * N))); gv = f32(0.01 * rng.standard_normal((B, 3 * N)))

    def run(fused, per_step_om=None, grads=True):
        e.set_state(0, X0, V0)
        if fused:
            e.rollout_forward(0, S)
        else:
            for s in range(S):
                if per_step_om is not None:
                    e.set_primitive_spins(per_step_om[s])
                e.step_forward(s)
        out = pv.collect(e, S)
        if grads:
            if fused:
                e.set_gradient(gx, gv)
                e.rollout_backward(S, S)
                out["dx"], out["dv"], out["dmu"] = e.get_gradient()
            else:
                cx, cv = gx, gv
                for s in range(S, 0, -1):
                    o = e.step_backward(s, cx, cv, is_start=(s == 1))
                    cx, cv = o["dL_dx"], o["dL_dv"]
                out["dx"], out["dv"] = cx, cv
        return out

    never_f, never_s = run(True), run(False)
    assert all((g >= 0).sum() > 10 for g in never_s["grp"])
    with pytest.raises(capi.DcError, match="no primitive spin has been set"):
        e.get_primitive_spin_gradients(1, S)
    # zeros = never set (the table exists from here on: the moving adjoint instances and the forward kernels' table branch run)
    e.set_primitive_spins(np.zeros((B, 1, 3)))
    pv.same(run(True), never_f); pv.same(run(False), never_s)
    assert np.all(e.get_primitive_spins(S) == 0) and np.all(e.get_primitive_velocities(S) == 0)
    with pytest.raises(capi.DcError, match="no primitive velocity has been set"):          # the two kinds are tracked separately
        e.get_primitive_velocity_gradients(1, S)
    e.set_primitive_spins(-np.zeros((B, 1, 3)))                                            # -0 is zero too
    pv.same(run(True), never_f)
    # ... and with velocities: zero spins = no spins
    e.alloc_batch(B, S)
    e.set_primitive_velocity_schedule(0, Ws)
    vel_f, vel_s = run(True), run(False)
    vel_f["dw"] = e.get_primitive_velocity_gradients(1, S)
    e.set_primitive_spins(np.zeros((B, 1, 3)))
    pv.same(dict(run(True), dw=e.get_primitive_velocity_gradients(1, S)), vel_f); pv.same(run(False), vel_s)
    e.alloc_batch(B, S)
    # a schedule = per-step calls
    a = run(False, per_step_om=OMs)
    a["dom"] = e.get_primitive_spin_gradients(1, S)
    for s in range(S):
        np.testing.assert_array_equal(e.get_primitive_spins(s + 1), f32(OMs[s]))
    assert np.abs(a["x"][S] - never_s["x"][S]).max() > 1e-4 and np.abs(a["dom"]).max() > 0
    np.testing.assert_array_equal(a["x"][:, 0], never_s["x"][:, 0])                        # rollout 0 has omega = 0: its own never-set run
    e.set_primitive_spins(None)
    e.set_primitive_spin_schedule(0, OMs)
    b_s = run(False)
    pv.same(b_s, a)
    np.testing.assert_array_equal(e.get_primitive_spin_gradients(1, S), a["dom"])
    b_f = run(True)
    pv.same(b_f, dict(x=a["x"], v=a["v"], grp=a["grp"], nrm=a["nrm"], f=a["f"], r=a["r"]))
    domf = e.get_primitive_spin_gradients(1, S)
    print(f"\n[primitive spin schedule nx={nx} K={e.cluster()}] backward sweep vs per-step calls: dL_dx {rel(b_f['dx'], a['dx']):.2e} "
          f"dL_dv {rel(b_f['dv'], a['dv']):.2e} dL_domega {rel(domf, a['dom']):.2e}")
    assert rel(b_f["dx"], a["dx"]) <= 2e-6 and rel(b_f["dv"], a["dv"]) <= 2e-6 and rel(domf, a["dom"]) <= 2e-6
    again = run(True)
    pv.same(again, b_f)                                                                    # the sweep is bit-reproducible,
    np.testing.assert_array_equal(e.get_primitive_spin_gradients(1, S), domf)              # dL/domega included
    # a schedule over part of a fused sweep is an error; a velocity schedule over all of it does not make up for it
    e.clear_schedules()
    e.set_primitive_spin_schedule(0, OMs[:2])
    e.set_primitive_velocity_schedule(0, Ws)
    with pytest.raises(capi.DcError, match="covers only part"):
        e.rollout_forward(0, S)
    # clear_schedules, NULL: the never-set result
    e.clear_schedules()
    e.set_primitive_velocities(None)
    pv.same(run(True), never_f); pv.same(run(False), never_s)
    e.set_primitive_spins(OMs[1])
    assert np.abs(run(True, grads=False)["x"][S] - never_f["x"][S]).max() > 1e-4
    e.set_primitive_spins(None)
    pv.same(run(True, grads=False), never_f)
    # a fresh alloc_batch drops spins and schedule, and the table itself
    e.set_primitive_spins(OMs[1]); e.set_primitive_spin_schedule(0, OMs[:2])
    e.alloc_batch(B, S)
    pv.same(run(False, grads=False), never_s); pv.same(run(True, grads=False), never_f)
    with pytest.raises(capi.DcError, match="no primitive spin has been set"):
        e.get_primitive_spin_gradients(1, S)
    e.close()


@pytest.mark.parametrize("nx,cluster", [(17, 0), (48, 4)])
def test_zero_unset_schedule_and_reset(nx, cluster, monkeypatch):
    check_zero_unset_schedule_and_reset(nx, cluster, monkeypatch)


@pytest.mark.parametrize("name", ["DC_DENSE_MAX_N", "DC_WINDOWS"])
def test_kernel_families_selected_at_build(name, monkeypatch):
    """DC_DENSE_MAX_N=0: the packet kernel's PCG instead of the explicit inverse small meshes get; DC_WINDOWS=0: the global-memory corner passes
    (resident kernel). Both are read at dc_build (the mechanism of tests/test_gpu_primitive_velocities.py)."""
    monkeypatch.setenv(name, "0")
    sc = scene("rotating")
    e = pv.make_engine(sc.V, sc.F, plain_prims(sc))
    lay = e.layout()
    assert not (lay["dense_inverse"] if name == "DC_DENSE_MAX_N" else lay["element_windows"])
    e.close()
    run_parity("rotating", backward=False)


@pytest.mark.parametrize("name", ["DC_DENSE_MAX_N", "DC_WINDOWS"])
def test_gradients_under_the_kernel_families_selected_at_build(name, monkeypatch):
    """the records those forward kernels leave, differentiated: two steps, backward and injected checks. DC_WINDOWS=0 also puts the one adjoint
    instance without element windows under a velocity and spin table."""
    monkeypatch.setenv(name, "0")
    run_parity("rotating", steps=2, backward=True)


@pytest.mark.parametrize("variant", ["global", "0", "1"])
def test_kernel_families_selected_per_process(variant):
    """DC_FWD_VARIANT is read once per process by the launchers: the forward parity in a child process per value"""
    env = dict(os.environ)
    env["DC_FWD_VARIANT"] = variant
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k",
                        "test_forward_parity_alone or test_without_the_spin_the_step_misses_the_oracle"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0, f"DC_FWD_VARIANT={variant}:\n{tail}\n{r.stderr[-2000:]}"
    assert "2 passed" in tail and "failed" not in tail, tail


def test_device_pointer_setters_and_getters_match_the_host_ones():
    B, S = pv.B, pv.S
    V, F, c, e = po.base_scene(tight=False)
    N = V.shape[0]
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(8)
    X0 = pv.lowered_state(V, B)
    V0 = np.zeros_like(X0)
    Wc = pv.W1 * 0.25
    gx = f32(rng.standard_normal((B, 3 * N))); gv = f32(0.01 * rng.standard_normal((B, 3 * N)))
    for OMs in (np.stack([pv.W1 * (0.5 * (s + 1)) for s in range(S)]), 1.3 * rng.standard_normal((S, B, 1, 3))):      # dyadic, and no fp32 numbers
        for dtype in (torch.float32, torch.float64):
            Oh = f32(OMs) if dtype == torch.float32 else OMs
            e.alloc_batch(B, S)
            e.set_state(0, X0, V0)
            e.set_primitive_velocities(Wc)                       # the other half of the rows stays what it is
            e.set_primitive_spin_schedule(0, Oh)
            e.rollout_forward(0, S)
            host = pv.collect(e, S)
            ho = np.stack([e.get_primitive_spins(s + 1) for s in range(S)])
            np.testing.assert_array_equal(ho, f32(Oh))
            e.set_gradient(gx, gv); e.rollout_backward(S, S)
            hdom, hdw = e.get_primitive_spin_gradients(1, S), e.get_primitive_velocity_gradients(1, S)
            assert np.abs(hdom).max() > 0 and np.abs(hdw).max() > 0
            wide = torch.zeros((S, B, 1, 6), dtype=dtype, device=dev)
            wide[..., :3] = torch.as_tensor(Oh, dtype=dtype)
            for t in (torch.as_tensor(Oh, dtype=dtype).to(dev), wide[..., :3]):    # contiguous, and a strided view the wrapper copies
                e.alloc_batch(B, S)
                e.set_state(0, X0, V0)
                e.set_primitive_velocities_dev(torch.as_tensor(Wc, dtype=dtype).to(dev))
                e.set_primitive_spin_schedule_dev(0, S, t)
                e.rollout_forward(0, S)
                pv.same(pv.collect(e, S), host)
                np.testing.assert_array_equal(np.stack([e.get_primitive_spins(s + 1) for s in range(S)]), ho)
                np.testing.assert_array_equal(e.get_primitive_velocities(S), f32(Wc))
                e.set_gradient(gx, gv); e.rollout_backward(S, S)
                out = torch.full((S, B, 1, 3), 7.0, dtype=dtype, device=dev)
                outw = torch.full((S, B, 1, 3), 7.0, dtype=dtype, device=dev)
                e.get_primitive_spin_gradients_dev(1, S, out)
                e.get_primitive_velocity_gradients_dev(1, S, outw)
                e.sync()
                np.testing.assert_array_equal(out.cpu().numpy().astype(np.float64), hdom)      # (fp32 values: exact in either dtype)
                np.testing.assert_array_equal(outw.cpu().numpy().astype(np.float64), hdw)
            # the spins of the NEXT steps
            e.clear_schedules()
            e.set_state(0, X0, V0)
            e.set_primitive_spins_dev(torch.as_tensor(Oh[1], dtype=dtype).to(dev))
            e.step_forward(0)
            np.testing.assert_array_equal(e.get_primitive_spins(1), ho[1])
            xa, _ = e.get_state(1)
            e.set_primitive_spins_dev(None)
            e.step_forward(0)
            assert np.all(e.get_primitive_spins(1) == 0) and np.abs(e.get_state(1)[0] - xa).max() > 1e-6
            np.testing.assert_array_equal(e.get_primitive_velocities(1), f32(Wc))
            e.set_primitive_spins(Oh[1])
            e.step_forward(0)
            np.testing.assert_array_equal(e.get_state(1)[0], xa)
    e.close()


# ---- 7. refusals ----
def test_refusals():
    """a non-zero omega for a plane-only group and non-finite values (DC_ERR_INVALID), no primitives at all; the fused sweep over a partial spin
    schedule is refused in check_zero_unset_schedule_and_reset, on the scene whose sweeps are known to be fused"""
    V, F = meshes.grid_cloth(5, 5, 4.5, 4.5, "DOWN")
    V = f32(V)
    c = f32(meshes.sphere_scene_center(V, 2.0))
    plane = dict(kind=capi.DC_PRIM_PLANE, group=1, center=c + np.array([0.0, -3.0, 0.0]), top_offset=(-4.0, 0.0, -4.0), corner2=(4.0, 0.0, -4.0), radius=0.0, mu=0.2)
    e = pv.make_engine(V, F, [pv.sphere(c), plane], tight=False)
    e.alloc_batch(2, 4)
    ok = np.zeros((2, 2, 3)); ok[:, 0] = (0.0, 4.0, 0.0)
    e.set_primitive_spins(ok)
    e.set_primitive_spin_schedule(0, ok[None])
    bad = ok.copy(); bad[1, 1, 2] = 0.5
    for call in (lambda a: e.set_primitive_spins(a), lambda a: e.set_primitive_spin_schedule(1, a[None])):
        with pytest.raises(capi.DcError, match="holds no DC_PRIM_SPHERE"):
            call(bad)
        for v in (np.nan, np.inf):
            nf = ok.copy(); nf[0, 0, 1] = v
            with pytest.raises(capi.DcError, match="not finite"):
                call(nf)
    np.testing.assert_array_equal(e.get_primitive_spins(1), ok)                           # the accepted schedule entry is in its row,
    np.testing.assert_array_equal(e.get_primitive_spins(2), np.zeros((2, 2, 3)))          # nothing of a refused one was stored
    e.set_primitive_spins_dev(torch.as_tensor(bad).cuda())                                # the _dev forms cannot look: accepted, the term is zero there
    e.sync()
    e.close()
    e = pv.make_engine(V, F, [], tight=False)
    e.alloc_batch(1, 1)
    with pytest.raises(capi.DcError, match="no primitives"):
        e.set_primitive_spins(np.zeros((1, 1, 3)))
    e.close()


# ---- 8. self-contact layers under a spinning sphere ----
def test_self_collision_layers_under_a_spinning_sphere(monkeypatch):
    """the flap scene of tests/test_gpu_primitive_velocities.py, the sphere's top under the flap, spinning: pairs, layers and primitive contacts are
    those of the oracle's rotating sphere from the same state; per-step path and fused sweep (detection inlined) agree bit for bit"""
    monkeypatch.setenv("DC_CLUSTER", "1")
    cfg = workloads.C4_CLOTH
    V, F, Vf, flap, c = workloads.c4_scene(grid=16, fold_rows=3, fold_gap=0.02)
    N = V.shape[0]
    fabric = dict(density=cfg["density"], k_stretch=cfg["k_stretch"], k_bend=cfg["k_bend"])
    radius = cfg["sphere_radius"]
    to_flap = Vf[flap].mean(axis=0) - c
    cm = f32(c + np.round(np.array([to_flap[0], 0.0, to_flap[2]]) * 32) / 32 + np.array([0.0, 0.125, 0.0]))
    prim = dict(kind=capi.DC_PRIM_SPHERE, group=0, center=cm, radius=radius, mu=cfg["sphere_mu"])
    nsteps = 2
    X0 = f32(Vf.reshape(1, -1)); V0 = np.zeros_like(X0)
    e = pv.make_engine(V, F, [prim], selfcollision=1, fabric=fabric)
    e.alloc_batch(1, nsteps)
    e.set_primitive_spins(spin_of(radius).reshape(1, 1, 3))
    runs = []
    for fused in (False, True):
        e.set_state(0, X0, V0)
        if fused:
            e.rollout_forward(0, nsteps)
        else:
            for s in range(nsteps):
                e.step_forward(s)
        runs.append([dict(x=e.get_state(s + 1)[0], v=e.get_state(s + 1)[1], grp=e.get_contacts(s + 1)[0], sc=e.get_self_contacts(s + 1, rollout=0))
                     for s in range(nsteps)])
    for p, q in zip(*runs):
        np.testing.assert_array_equal(p["x"], q["x"]); np.testing.assert_array_equal(p["grp"], q["grp"])
        np.testing.assert_array_equal(p["sc"]["pairs"], q["sc"]["pairs"]); np.testing.assert_array_equal(p["sc"]["layer"], q["sc"]["layer"])
    o = orc.Oracle(V, F, h=H, fwd_tol=1e-9, bwd_tol=1e-9, selfcollision=True, contact=True, gradient_clipping=False, **fabric)
    o.add_sphere(cm, radius, cfg["sphere_mu"], rotates=True)
    o.build()
    x, v = X0[0], V0[0]
    for s in range(nsteps):
        ref = o.step(x, v)
        sc = o.self_contacts(ref["id"])
        got = runs[0][s]["sc"]
        want = sorted((int(l), int(p), int(q)) for l, p, q in zip(sc["layer"], sc["p1"], sc["p2"]))
        have = sorted((int(l), int(p), int(q)) for l, (p, q) in zip(got["layer"], got["pairs"]))
        assert have == want, f"step {s}"
        assert got["layers"] == ref["nlayers"] and got["count"] == ref["nself"] >= 10
        ids = pv.contact_ids(runs[0][s]["grp"][0])
        np.testing.assert_array_equal(ids, np.sort(o.prim_contacts(ref["id"])["particle"]))
        assert len(ids) >= 5
        dx = np.abs(runs[0][s]["x"][0] - ref["x"]).max()
        print(f"[spinning sphere under the flap] step {s}: {got['count']} self contacts in {got['layers']} layers, {len(ids)} primitive contacts, "
              f"max|x - x_oracle| {dx:.2e}")
        x, v = runs[0][s]["x"][0], runs[0][s]["v"][0]              # the oracle goes on from the engine's state
    e.close()


# ---- 9. sim_rollout ----
def test_sim_rollout_takes_primitive_spins_on_both_paths():
    """device path = host path; [B, G, 3] = [T, B, G, 3] repeated; primitive_spins.grad = Engine.get_primitive_spin_gradients (summed over the steps
    for the short form); the other gradients of the call do not depend on whether the spin requires grad; spin, velocity, offset and shape
    together through sim_rollout = the same through the engine's entries"""
    B, S = pv.B, pv.S
    V, F, c, e = po.base_scene(tight=False)
    N = V.shape[0]
    e.alloc_batch(B, S)
    sim = BatchedSim(e, S)
    rng = np.random.default_rng(4)
    x0 = pv.lowered_state(V, B)
    Wc = pv.W1 * 0.25
    OMc = pv.W1[::-1] * 0.5
    Dc = np.broadcast_to(np.array([0.0, 0.03125, 0.0]), (B, 1, 3)).copy()
    SH = np.tile(e.built_primitive_shapes()[None], (B, 1, 1))            # [B][P][8]: the built shapes, given explicitly
    v0 = np.stack([f32(np.tile(Wc[b, 0], N)) for b in range(B)])
    w = f32(1e-3 * rng.standard_normal((S, B, 3 * N)))

    def run(device, om, om_grad=True, extras=False):
        t = lambda a, grad=False: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(device).requires_grad_(grad)
        tx, tv, tw, to = t(x0, True), t(v0, True), t(Wc, True), t(om, om_grad)
        kw = dict(primitive_offsets=t(Dc), primitive_shapes=t(SH)) if extras else {}
        xs, vs = sim_rollout(sim, tx, tv, None, steps=S, primitive_velocities=tw, primitive_spins=to, **kw)
        (xs * t(w)).sum().backward()
        g = lambda q: None if q.grad is None else q.grad.cpu().numpy()
        return dict(xs=xs.detach().cpu().numpy(), vs=vs.detach().cpu().numpy(), dx=g(tx), dv=g(tv), dw=g(tw), dom=g(to),
                    getter=e.get_primitive_spin_gradients(1, S))

    long = np.broadcast_to(OMc, (S, B, 1, 3)).copy()
    host, devc = run("cpu", long), run("cuda", long)
    np.testing.assert_array_equal(devc["xs"], host["xs"]); np.testing.assert_array_equal(devc["vs"], host["vs"])
    assert rel(devc["dx"], host["dx"]) <= 2e-6 and rel(devc["dom"], host["dom"]) <= 2e-6 and np.abs(host["dom"]).max() > 0
    for r in (host, devc):
        np.testing.assert_array_equal(r["dom"], r["getter"].astype(np.float32))
    for device, full in (("cpu", host), ("cuda", devc)):
        short = run(device, OMc)
        np.testing.assert_array_equal(short["xs"], full["xs"])
        assert rel(short["dom"], short["getter"].sum(axis=0)) <= 2e-6          # (fp32 tensors: one rounding of the sum)
        const = run(device, long, om_grad=False)                             # the spin as a constant: the other gradients are unchanged
        assert const["dom"] is None
        for k in ("xs", "vs", "dx", "dv", "dw"):
            np.testing.assert_array_equal(const[k], full[k], err_msg=k)
    # everything together through sim_rollout = the engine's own entries, on both paths
    both = [run(device, long, extras=True) for device in ("cpu", "cuda")]
    np.testing.assert_array_equal(both[0]["xs"], both[1]["xs"])
    e.clear_schedules()
    e.set_primitive_offset_schedule(0, np.broadcast_to(Dc, (S, B, 1, 3)).copy())
    e.set_primitive_velocity_schedule(0, np.broadcast_to(f32(Wc), (S, B, 1, 3)).copy())
    e.set_primitive_shape_schedule(0, np.broadcast_to(f32(SH), (S,) + SH.shape).copy())
    e.set_primitive_spin_schedule(0, f32(long))
    e.set_state(0, x0, v0)
    e.rollout_forward(0, S)
    xs, vs = e.get_states(1, S)
    np.testing.assert_array_equal(xs.astype(np.float32), both[0]["xs"])
    none = run("cuda", np.zeros_like(long))
    assert np.abs(none["xs"] - devc["xs"]).max() > 1e-5
    e.close()
