"""Movable obstacles: per-rollout, per-step offsets of the primitive groups' centres (dc_set_primitive_offsets, dc_set_primitive_offset_schedule,
their _dev forms, dc_get_primitive_centers; sim_rollout(primitive_offsets=...); diffcloth_py's writable Primitive.center).

The reference reads Primitive::center at every step (isInContactWithObstacle, Simulation.cpp:153-191). The rule under test (csrc/dc_primoffset.h):
every flattened primitive of group g of rollout b is tested at fp32((double) center + d[b][g]) — so a context GIVEN an offset and a context
BUILT at the moved centre compute the same step bit for bit, and the fp64 oracle with its obstacle at that fp32 centre is the parity partner.

Base scene: the 17 x 17 cloth of tests/test_gpu_schedules.py (sphere of radius 2 at c = f32(sphere_scene_center), h = 1/180, mu = 0.4), four steps
from rest, B = 4; dyadic offsets, so f32(c + d) is what both sides see:
  b0 (0, 0.125, 0)               oracle contacts per step 21 / 21 / 22 / 21 of 289 vertices
  b1 (0.25, 0.1875, 0.125)       30 / 30 / 31 / 30, a different contact set in every step
  b2 (0, -4, 0)                  none: the obstacle is out of reach
  b3 moving, (0.03125 (s + 1), 0.0625 + 0.03125 (s + 1), 0) at step s: 15 / 20 / 27 / 31
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch          # before the engine's library: both must share ONE HIP runtime (torch's), see tests/test_gpu_functional.py

import meshes
import orc
import records
from diffcloth_amd import capi, workloads
from diffcloth_amd.functional import BatchedSim, sim_rollout

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 1.0 / 180
B, S = 4, 4
FABRIC = dict(density=0.3, k_stretch=150.0, k_bend=0.05)


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-30)


def base_offsets():
    """[S][B][G = 1][3], all dyadic"""
    D = np.zeros((S, B, 1, 3))
    D[:, 0, 0] = (0.0, 0.125, 0.0)
    D[:, 1, 0] = (0.25, 0.1875, 0.125)
    D[:, 2, 0] = (0.0, -4.0, 0.0)
    for s in range(S):
        D[s, 3, 0] = (0.03125 * (s + 1), 0.0625 + 0.03125 * (s + 1), 0.0)
    return D


def engine(V, F, prims, att=(), tight=True, selfcollision=0, h=H, fabric=FABRIC, fwd_tol=None):
    """tight: the solver settings of tests/test_gpu_primitives.py::pair (oracle parity); else those of tests/test_gpu_schedules.py::scene"""
    e = capi.Engine(0)
    e.set_mesh(V, F)
    e.set_attachments(att)
    tol = dict(forward_tol=1e-9, backward_tol=1e-9, cg_rel_tol=1e-6, adjoint_rel_tol=1e-8) if tight else \
        dict(forward_tol=1e-7, backward_tol=1e-7, cg_rel_tol=1e-5, adjoint_rel_tol=1e-7)
    if fwd_tol is not None:
        tol["forward_tol"] = fwd_tol
    e.set_params(time_step=h, cg_max_iter=2000, gradient_clipping=0, selfcollision_enabled=selfcollision, adjoint_mode=1, **fabric, **tol)
    e.set_primitives(prims)
    e.build()
    return e


def base_scene(nx=17, tight=True, att=()):
    V, F = meshes.grid_cloth(nx, nx, 4.5, 4.5, "DOWN")
    V = f32(V)
    c = f32(meshes.sphere_scene_center(V, 2.0))
    e = engine(V, F, [dict(kind=capi.DC_PRIM_SPHERE, group=0, center=c, radius=2.0, mu=0.4)], att=att, tight=tight)
    return V, F, c, e


def sphere_oracle(V, F):
    o = orc.Oracle(V, F, h=H, fwd_tol=1e-9, bwd_tol=1e-9, selfcollision=False, gradient_clipping=False, **FABRIC)
    o.build()
    return o


def oracle_sphere_at(o, centre, radius=2.0, mu=0.4):
    """the oracle's single obstacle, cleared and re-added at `centre` (it reads its primitives at every step: no rebuild)"""
    orc.lib().orc_clear_primitives(o.h)
    o.nprim = 0
    o.add_sphere(centre, radius, mu)


def contact_ids(grp_row):
    return np.nonzero(grp_row >= 0)[0]


# ---- 1. oracle parity on the base scene: the statements and gates of tests/test_gpu_primitives.py::check_step, per rollout and per step ----
def check_base_scene_against_oracle(backward=True):
    V, F, c, e = base_scene()
    N = V.shape[0]
    D = base_offsets()
    e.alloc_batch(B, S)
    X0 = np.tile(f32(V.reshape(-1)), (B, 1))
    e.set_state(0, X0, np.zeros_like(X0))
    e.set_primitive_offset_schedule(0, D)
    oracles = [sphere_oracle(V, F) for _ in range(B)]
    rng = np.random.default_rng(31)
    sets = [[None] * B for _ in range(S)]
    lines = []
    for s in range(S):
        xs, vs = e.get_state(s)
        st = e.step_forward(s)                        # the per-step call honours the schedule entry of its slot
        x1, v1 = e.get_state(s + 1)
        grp, nrm = e.get_contacts(s + 1)
        fr = e.get_record(s + 1)[0]
        np.testing.assert_array_equal(e.get_primitive_centers(s + 1)[:, 0], f32(c + D[s, :, 0]))
        gx = f32(rng.standard_normal((B, 3 * N))); gv = f32(0.01 * rng.standard_normal((B, 3 * N)))
        gb = e.step_backward(s + 1, gx, gv) if backward else None
        for b in range(B):
            o = oracles[b]
            oracle_sphere_at(o, f32(c + D[s, b, 0]))
            ref = o.step(xs[b], vs[b])
            assert st["converged"][b] == 1 and ref["converged"]
            assert st["prim_contacts"][b] == ref["nprim"]
            pc = o.prim_contacts(ref["id"])
            ids = contact_ids(grp[b])
            order = np.argsort(pc["particle"])
            np.testing.assert_array_equal(ids, pc["particle"][order])                                   # the same vertices are in contact
            np.testing.assert_allclose(nrm[b].reshape(-1, 3)[ids], pc["normal"][order], atol=2e-6)      # with the same normals
            sets[s][b] = set(ids.tolist())
            dx = np.abs(x1[b] - ref["x"]).max()
            line = f"step {s} rollout {b}: contacts {ref['nprim']}, PD iterations gpu {st['pd_iters'][b]} / oracle {ref['iters']}, max|dx| {dx:.2e}"
            assert dx <= 5e-5, line
            if backward:
                rb = o.step_backward(ref["id"], gx[b], gv[b], is_start=False, direct=True)
                ex, ev = rel(gb["dL_dx"][b], rb["dL_dx"]), rel(gb["dL_dv"][b], rb["dL_dv"])
                records.oracle_adopts_gpu_record(o, ref["id"], e, s + 1, b, xs[b], x1[b], v1[b], fr[b], H, normals=nrm)
                rb3 = o.step_backward(ref["id"], gx[b], gv[b], is_start=False, direct=True)
                ea = max(rel(gb["dL_dx"][b], rb3["dL_dx"]), rel(gb["dL_dv"][b], rb3["dL_dv"]), records.mu_err(gb["dL_dmu"][b], rb3["dL_dmu"]))
                line += f", gradient rel err dx {ex:.2e} dv {ev:.2e}, same record (oracle adopts) {ea:.2e}"
                lines.append(line)
                assert ex <= 1e-4 and ev <= 1e-4, line
                assert ea <= 1e-4, line
            else:
                lines.append(line)
    print("\n[primitive offsets, base scene]\n" + "\n".join(lines))
    # what keeps the test from being vacuous
    for s in range(S):
        assert all(len(sets[s][b]) >= 10 for b in (0, 1, 3)), [len(q) for q in sets[s]]
        assert len(sets[s][2]) == 0
        assert sets[s][1] != sets[s][0] and sets[s][3] != sets[s][0]
    e.close()


def test_oracle_parity_on_the_base_scene():
    check_base_scene_against_oracle()


# ---- 2. bitwise against a context built at the moved centre, every primitive kind ----
def run_steps(e, X0, V0, nsteps, offsets=None):
    """nsteps per-step calls from (X0, V0); everything a step leaves behind"""
    nb = X0.shape[0]
    e.alloc_batch(nb, nsteps)
    if offsets is not None:
        e.set_primitive_offsets(offsets)
    e.set_state(0, X0, V0)
    out = []
    for s in range(nsteps):
        st = e.step_forward(s)
        x, v = e.get_state(s + 1)
        grp, nrm = e.get_contacts(s + 1)
        f, r = e.get_record(s + 1)
        out.append(dict(x=x, v=v, grp=grp, nrm=nrm, f=f, r=r, contacts=st["prim_contacts"].copy(), centres=e.get_primitive_centers(s + 1)))
    return out


def check_offsets_equal_moved_builds(V, F, prims, Doff, X0, V0, monkeypatch, nsteps=2, min_contacts=5, fabric=FABRIC, h=H):
    """prims: engine primitive dicts (fp64 centres); Doff: [nb][G][3]; rollout b of the context given Doff against rollout b of a context whose
    primitives were built at center + Doff[b][group] (the sum formed in fp64 by the caller), same batch size, one workgroup per rollout"""
    monkeypatch.setenv("DC_CLUSTER", "1")
    nb = X0.shape[0]
    groups = []
    for p in prims:
        if p["group"] not in groups:
            groups.append(p["group"])
    e = engine(V, F, prims, fwd_tol=1e-7, fabric=fabric, h=h)
    got = run_steps(e, X0, V0, nsteps, offsets=Doff)
    assert e.cluster() == 1
    e.close()
    for b in range(nb):
        moved = [dict(p, center=np.asarray(p["center"], dtype=np.float64) + Doff[b, groups.index(p["group"])]) for p in prims]
        em = engine(V, F, moved, fwd_tol=1e-7, fabric=fabric, h=h)
        want = run_steps(em, X0, V0, nsteps)
        em.close()
        for s in range(nsteps):
            for key in ("x", "v", "grp", "nrm", "f", "r", "centres"):
                np.testing.assert_array_equal(got[s][key][b], want[s][key][b], err_msg=f"rollout {b} step {s} {key}")
            np.testing.assert_array_equal(want[s]["centres"][b], np.stack([f32(q["center"]) for q in moved]))
            assert got[s]["contacts"][b] >= min_contacts, (b, s, got[s]["contacts"])
    return got


def test_offset_equals_build_at_the_moved_centre_sphere(monkeypatch):
    V, F = meshes.grid_cloth(17, 17, 4.5, 4.5, "DOWN")
    V = f32(V)
    c = f32(meshes.sphere_scene_center(V, 2.0)) + 1e-9            # an fp64 centre that is no fp32 number: the sum is rounded once
    D = np.array([[[0.0, 0.125, 0.0]], [[0.25, 0.1875, 0.125]], [[1e-3, 0.2, -0.3]]])
    X0 = np.tile(f32(V.reshape(-1)), (3, 1))
    got = check_offsets_equal_moved_builds(V, F, [dict(kind=capi.DC_PRIM_SPHERE, group=0, center=c, radius=2.0, mu=0.4)], D, X0, np.zeros_like(X0), monkeypatch)
    assert set(contact_ids(got[0]["grp"][0])) != set(contact_ids(got[0]["grp"][1]))


def test_offset_equals_build_at_the_moved_centre_tilted_plane(monkeypatch):
    """the rectangle of tests/test_gpu_primitives.py::test_finite_tilted_plane: its corners are relative to the centre and move with it"""
    V, F = meshes.grid_cloth(22, 22, 4.5, 4.5, "DOWN")
    V = f32(V)
    c = f32(V.mean(axis=0) + np.array([0.13, -0.25, 0.07]))
    ul, ur = f32([-1.5, 0.3, -1.5]), f32([1.5, 0.3, -1.5])
    D = np.array([[[0.0625, 0.125, 0.0]], [[-0.625, -0.0625, 0.75]]])
    X0 = np.tile(f32(V.reshape(-1)), (2, 1))
    got = check_offsets_equal_moved_builds(V, F, [dict(kind=capi.DC_PRIM_PLANE, group=0, center=c, top_offset=ul, corner2=ur, radius=0.0, mu=0.2)], D, X0,
                                           np.zeros_like(X0), monkeypatch, min_contacts=50)
    a, b = set(contact_ids(got[0]["grp"][0])), set(contact_ids(got[0]["grp"][1]))
    assert a != b and len(a) < V.shape[0] and len(b) < V.shape[0]      # the rim hangs free, and the rectangle covers other vertices after the move


def test_offset_equals_build_at_the_moved_centre_bowl(monkeypatch):
    """Bowl::isInContact tests pos.y > center.y (Primitive.cpp:362-381): a sheet laid on the MOVED shell across its equator — the half above the
    moved centre is free, the half below in contact; with the built centre in that test the split would sit elsewhere."""
    V, F = meshes.grid_cloth(14, 14, 1.3, 1.3, "DOWN")
    V = f32(V)
    R = 1.2
    c = f32(np.array([V[:, 0].mean(), 0.0, V[:, 2].mean()]))
    D = np.array([[[0.125, 0.25, 0.0]], [[0.0, -0.8125, 0.0625]]])
    u, w = (V[:, 0] - V[:, 0].mean()) / R, (V[:, 2] - V[:, 2].mean()) / R           # elevation / azimuth of the sheet's vertices on the shell
    unit = np.stack([np.cos(u) * np.cos(w), np.sin(u), np.cos(u) * np.sin(w)], axis=1)
    X0 = np.stack([f32((c + D[b, 0] + R * unit).reshape(-1)) for b in range(2)])
    V0 = np.tile(f32((0.3 * unit).reshape(-1)), (2, 1))                                # moving outwards, onto the shell
    got = check_offsets_equal_moved_builds(V, F, [dict(kind=capi.DC_PRIM_BOWL, group=0, center=c, radius=R, mu=0.4)], D, X0, V0, monkeypatch, nsteps=1, min_contacts=40)
    for b in range(2):
        ids = contact_ids(got[0]["grp"][b])
        y = X0[b].reshape(-1, 3)[:, 1]
        cy = f32(c + D[b, 0])[1]
        assert (y[ids] <= cy).all() and (y > cy).sum() >= 40 and len(ids) < V.shape[0]
    assert (X0[1].reshape(-1, 3)[:, 1] < c[1]).all()               # rollout 1: the whole sheet is below the BUILT centre, yet half of it is free


def leg_scene(nx=12):
    V, F = meshes.grid_cloth(nx, nx, 4.5, 4.5, "DOWN")
    V = f32(V)
    center, children = workloads.sock_leg(V.min(axis=0), V.max(axis=0))
    center = f32(center)
    prims = [dict(kind=capi.DC_PRIM_SPHERE if k == 0 else capi.DC_PRIM_CAPSULE, group=7, center=center + f32(c0), radius=float(np.float32(r)), mu=0.4,
                  top_offset=f32(t), length=float(np.float32(ln))) for k, c0, t, r, ln in children]
    return V, F, center, prims


def test_offset_equals_build_at_the_moved_centre_lower_leg(monkeypatch):
    """a LowerLeg (joint sphere, foot capsule, leg capsule of workloads.sock_leg: one group) — ONE offset per rollout moves all three children. A
    horizontal sheet threaded by the leg: around the foot capsule (rollout 0) and at the joint, where sphere and both capsules meet (rollout 1)."""
    V, F, center, prims = leg_scene()
    D = np.array([[[0.25, 0.5, -0.125]], [[-0.375, 0.0625, 0.25]]])
    mid = V.mean(axis=0)
    X0 = np.stack([f32((V + (center + D[b, 0] + np.array([0.0, height, 0.0]) - mid)).reshape(-1)) for b, height in ((0, 2.0), (1, 4.1))])
    V0 = np.zeros_like(X0)
    got = check_offsets_equal_moved_builds(V, F, prims, D, X0, V0, monkeypatch, min_contacts=8)
    built = np.stack([np.asarray(p["center"], dtype=np.float64) for p in prims])
    for b in range(2):
        np.testing.assert_array_equal(got[0]["centres"][b], f32(built + D[b, 0]))         # every child moved by the group's offset
        assert set(got[0]["grp"][b][contact_ids(got[0]["grp"][b])].tolist()) == {7}       # contacts report the caller's group id


def test_offset_equals_build_at_the_moved_centre_discretised_sphere(monkeypatch):
    """the BIG_SPHERE of tests/test_gpu_primitives.py::test_discretised_sphere (radius 15): its face table is stored relative to the centre, the
    sample point is re-formed in fp64 against the MOVED centre. Also against the oracle's add_discretized_sphere at the moved centre."""
    V, F = meshes.grid_cloth(22, 22, 4.5, 4.5, "DOWN")
    V = f32(V)
    R = 15.0
    c = np.array([-0.5, -16.0, 0.0])
    D = np.array([[[0.375, 0.25, -0.125]], [[-1.0, 0.5, 2.0]]])
    rows = []
    for b in range(2):
        cb = c + D[b, 0]
        X = V.copy()
        X[:, 0] += cb[0] - V[:, 0].mean() + 0.37; X[:, 2] += cb[2] - V[:, 2].mean() - 0.21      # (off the mesh's symmetry lines)
        X[:, 1] = cb[1] + np.sqrt(R * R - (X[:, 0] - cb[0]) ** 2 - (X[:, 2] - cb[2]) ** 2) + 0.02
        rows.append(f32(X.reshape(-1)))
    X0 = np.stack(rows)
    vel = np.zeros_like(V); vel[:, 1] = -0.3; vel[:, 0] = 0.2
    V0 = np.tile(f32(vel.reshape(-1)), (2, 1))
    got = check_offsets_equal_moved_builds(V, F, [dict(kind=capi.DC_PRIM_SPHERE_DISCRETIZED, group=0, center=c, radius=R, mu=0.3)], D, X0, V0, monkeypatch,
                                           nsteps=1, min_contacts=400)
    for b in range(2):
        o = orc.Oracle(V, F, h=H, fwd_tol=1e-9, bwd_tol=1e-9, selfcollision=False, gradient_clipping=False, **FABRIC)
        o.add_discretized_sphere(f32(c + D[b, 0]), R, 0.3)
        o.build()
        ref = o.step(X0[b], V0[b])
        pc = o.prim_contacts(ref["id"])
        ids = contact_ids(got[0]["grp"][b])
        order = np.argsort(pc["particle"])
        np.testing.assert_array_equal(ids, pc["particle"][order])
        np.testing.assert_allclose(got[0]["nrm"][b].reshape(-1, 3)[ids], pc["normal"][order], atol=2e-6)
        radial = (X0[b].reshape(-1, 3)[ids] - (c + D[b, 0])) / np.linalg.norm(X0[b].reshape(-1, 3)[ids] - (c + D[b, 0]), axis=1)[:, None]
        assert np.abs(pc["normal"][order] - radial).max() > 1e-2            # face normals, not radial ones


# ---- 3. self collision: detection (which seeds the layering with the primitive contacts) and the step kernel see the same centres ----
def test_self_collision_layers_follow_the_moved_sphere(monkeypatch):
    """workloads.c4_scene on a 16 x 16 grid (flap of 3 rows folded onto the cloth), the sphere moved per rollout under the flap: the primitive
    contacts seed the layering frontier of contactSorting (Simulation.cpp:455-460), so pairs, layers and normals equal the oracle's only when the
    detection saw the step's centres; per-step path and fused sweep (detection inlined), and a context built at the moved centre."""
    monkeypatch.setenv("DC_CLUSTER", "1")
    cfg = workloads.C4_CLOTH
    V, F, Vf, flap, c = workloads.c4_scene(grid=16, fold_rows=3, fold_gap=0.02)
    N = V.shape[0]
    fabric = dict(density=cfg["density"], k_stretch=cfg["k_stretch"], k_bend=cfg["k_bend"])
    prim = dict(kind=capi.DC_PRIM_SPHERE, group=0, center=c, radius=cfg["sphere_radius"], mu=cfg["sphere_mu"])
    to_flap = Vf[flap].mean(axis=0) - c
    nb, nsteps = 2, 2
    D = np.zeros((nb, 1, 3))
    for b, frac in enumerate((1.0, 0.5)):          # the sphere's top under the flap / half-way there; 1/32 steps
        D[b, 0] = np.round(np.array([to_flap[0] * frac, 0.0, to_flap[2] * frac]) * 32) / 32 + np.array([0.0, 0.125 + 0.03125 * b, 0.0])
    X0 = np.tile(f32(Vf.reshape(-1)), (nb, 1))
    V0 = np.zeros_like(X0)

    def collect(e):
        out = []
        for s in range(nsteps):
            grp, nrm = e.get_contacts(s + 1)
            x, v = e.get_state(s + 1)
            out.append(dict(x=x, v=v, grp=grp, nrm=nrm, selfc=[e.get_self_contacts(s + 1, rollout=b) for b in range(nb)]))
        return out

    def same(a, b_, rollouts):
        for s in range(nsteps):
            for b in rollouts:
                for key in ("x", "v", "grp", "nrm"):
                    np.testing.assert_array_equal(a[s][key][b], b_[s][key][b], err_msg=f"step {s} rollout {b} {key}")
                p, q = a[s]["selfc"][b], b_[s]["selfc"][b]
                assert p["count"] == q["count"] and p["layers"] == q["layers"]
                for key in ("pairs", "layer", "normal"):
                    np.testing.assert_array_equal(p[key], q[key])

    e = engine(V, F, [prim], selfcollision=1, fabric=fabric)
    e.alloc_batch(nb, nsteps)
    e.set_primitive_offsets(D)
    e.set_state(0, X0, V0)
    states = [e.get_state(0)]
    for s in range(nsteps):
        e.step_forward(s)
        states.append(e.get_state(s + 1))
    stepwise = collect(e)
    e.set_state(0, X0, V0)
    e.rollout_forward(0, nsteps)                    # fused: the detection of every step runs inside the step kernel's launch
    same(collect(e), stepwise, range(nb))
    e.close()
    for b in range(nb):
        em = engine(V, F, [dict(prim, center=c + D[b, 0])], selfcollision=1, fabric=fabric)
        em.alloc_batch(nb, nsteps)
        em.set_state(0, X0, V0)
        em.rollout_forward(0, nsteps)
        same(collect(em), stepwise, [b])
        em.close()
    # the oracle, teacher-forced from the engine's state of every step
    for b in range(nb):
        o = orc.Oracle(V, F, h=H, fwd_tol=1e-9, bwd_tol=1e-9, selfcollision=True, contact=True, gradient_clipping=False, **fabric)
        o.build()
        for s in range(nsteps):
            oracle_sphere_at(o, f32(c + D[b, 0]), cfg["sphere_radius"], cfg["sphere_mu"])
            ref = o.step(states[s][0][b], states[s][1][b])
            sc = o.self_contacts(ref["id"])
            got = stepwise[s]["selfc"][b]
            want = sorted((int(l), int(p), int(q)) for l, p, q in zip(sc["layer"], sc["p1"], sc["p2"]))
            have = sorted((int(l), int(p), int(q)) for l, (p, q) in zip(got["layer"], got["pairs"]))
            assert have == want, f"rollout {b} step {s}"
            assert got["layers"] == ref["nlayers"] and got["count"] == ref["nself"] >= 10
            nmap = {(int(p), int(q)): n for p, q, n in zip(sc["p1"], sc["p2"], sc["normal"])}
            for (p, q), n in zip(got["pairs"], got["normal"]):
                np.testing.assert_allclose(n, nmap[(int(p), int(q))], atol=5e-6)
            pc = o.prim_contacts(ref["id"])
            ids = contact_ids(stepwise[s]["grp"][b])
            np.testing.assert_array_equal(ids, np.sort(pc["particle"]))
            assert len(ids) >= 5
            # the frontier matters here: vertices in primitive contact take part in self contacts
            assert len(set(ids.tolist()) & set(got["pairs"].reshape(-1).tolist())) > 0, f"rollout {b} step {s}: no vertex in both kinds of contact"
    assert set(contact_ids(stepwise[0]["grp"][0])) != set(contact_ids(stepwise[0]["grp"][1]))


# ---- 4. schedule = per-step calls, bitwise; the backward sweep over the moved record ----
def check_schedule_equals_per_step_calls(nx, cluster, monkeypatch, oracle=True):
    if cluster:
        monkeypatch.setenv("DC_CLUSTER", str(cluster))
    V, F, c, e = base_scene(nx, tight=(nx == 17))
    N = V.shape[0]
    D = base_offsets()
    e.alloc_batch(B, S)
    assert e.cluster() == (cluster if cluster else 1)
    rng = np.random.default_rng(5)
    X0 = np.tile(f32(V.reshape(-1)), (B, 1))
    V0 = np.zeros_like(X0)
    centres = np.stack([f32(c + D[s, :, 0]) for s in range(S)])
    # ---- (a) per-step calls: the offsets of a step set before it
    e.set_state(0, X0, V0)
    for s in range(S):
        e.set_primitive_offsets(D[s])
        e.step_forward(s)
        np.testing.assert_array_equal(e.get_primitive_centers(s + 1)[:, 0], centres[s])
    xa, va = e.get_states(0, S + 1)
    ca = [e.get_contacts(s + 1) for s in range(S)]
    assert all((ca[s][0][b] >= 0).sum() >= 10 for s in range(S) for b in (0, 1, 3)) and all((ca[s][0][2] >= 0).sum() == 0 for s in range(S))
    gx = f32(rng.standard_normal((B, 3 * N))); gv = f32(0.01 * rng.standard_normal((B, 3 * N)))
    cx, cv = gx, gv
    for s in range(S, 0, -1):
        out = e.step_backward(s, cx, cv, is_start=(s == 1))
        cx, cv = out["dL_dx"], out["dL_dv"]
    # ---- (b) the schedule + one launch per direction
    e.set_primitive_offsets(None)
    e.set_state(0, X0, V0)
    e.set_primitive_offset_schedule(0, D)
    e.rollout_forward(0, S)
    xb, vb = e.get_states(0, S + 1)
    np.testing.assert_array_equal(xa, xb)
    np.testing.assert_array_equal(va, vb)
    for s in range(S):
        np.testing.assert_array_equal(e.get_primitive_centers(s + 1)[:, 0], centres[s])
        cb = e.get_contacts(s + 1)
        np.testing.assert_array_equal(ca[s][0], cb[0]); np.testing.assert_array_equal(ca[s][1], cb[1])
    e.set_gradient(gx, gv)
    e.rollout_backward(S, S)
    dx, dv, _ = e.get_gradient()
    print(f"\n[primitive offset schedule nx={nx} K={e.cluster()}] backward sweep vs per-step calls: dL_dx {rel(dx, cx):.2e} dL_dv {rel(dv, cv):.2e}")
    assert rel(dx, cx) <= 2e-6 and rel(dv, cv) <= 2e-6
    if oracle:      # the moving obstacle of rollout 3: the oracle's steps from the engine's states, its backward steps chained
        o = sphere_oracle(V, F)
        rids = []
        for s in range(S):
            oracle_sphere_at(o, centres[s, 3])
            rids.append(o.step(xa[s, 3], va[s, 3])["id"])
        ox, ov = gx[3], gv[3]
        for s in range(S, 0, -1):
            rb = o.step_backward(rids[s - 1], ox, ov, is_start=(s == 1), direct=True)
            ox, ov = rb["dL_dx"], rb["dL_dv"]
        print(f"[primitive offset schedule nx={nx}] rollout 3 (moving obstacle), sweep vs the oracle's chained backward steps: dL_dx {rel(dx[3], ox):.2e} dL_dv {rel(dv[3], ov):.2e}")
        assert rel(dx[3], ox) <= 1e-4 and rel(dv[3], ov) <= 1e-4
    # ---- a schedule that covers only part of a FUSED sweep is an error, not a silent mix (the split kernels and the packet kernels fuse; the
    # resident / global-memory families of DC_FWD_VARIANT run a rollout step by step, where every step takes its own entry or the current offsets)
    e.clear_schedules()
    e.set_primitive_offset_schedule(0, D[:2])
    if cluster or os.environ.get("DC_FWD_VARIANT") is None:
        with pytest.raises(capi.DcError, match="covers only part"):
            e.rollout_forward(0, S)
    else:
        e.set_state(0, X0, V0)
        e.rollout_forward(0, S)
        for s in range(S):
            np.testing.assert_array_equal(e.get_primitive_centers(s + 1)[:, 0], centres[s] if s < 2 else np.broadcast_to(c, (B, 3)))
    e.clear_schedules()
    e.set_state(0, X0, V0)
    e.rollout_forward(0, S)                          # and without a schedule the current offsets (none) apply again
    xc, _ = e.get_states(S, 1)
    assert np.abs(xc[0] - xa[S]).max() > 1e-6
    e.close()


@pytest.mark.parametrize("nx,cluster", [(17, 0), (48, 4)])
def test_schedule_equals_per_step_calls(nx, cluster, monkeypatch):
    check_schedule_equals_per_step_calls(nx, cluster, monkeypatch, oracle=(nx == 17))


# ---- 5. the other kernel families ----
@pytest.mark.parametrize("name", ["DC_DENSE_MAX_N", "DC_WINDOWS"])
def test_kernel_families_selected_at_build(name, monkeypatch):
    """DC_DENSE_MAX_N=0: the packet kernel's PCG instead of the explicit inverse small meshes get; DC_WINDOWS=0: the global-memory corner passes
    (resident kernel). Both are read at dc_build."""
    monkeypatch.setenv(name, "0")
    _, _, _, e = base_scene()
    lay = e.layout()
    assert not (lay["dense_inverse"] if name == "DC_DENSE_MAX_N" else lay["element_windows"])
    e.close()
    check_base_scene_against_oracle(backward=False)
    check_schedule_equals_per_step_calls(17, 0, monkeypatch, oracle=False)


@pytest.mark.parametrize("variant", ["global", "0", "1"])
def test_kernel_families_selected_per_process(variant):
    """DC_FWD_VARIANT is read once per process by the launchers: tests 1 and 4 in a child process per value"""
    env = dict(os.environ)
    env["DC_FWD_VARIANT"] = variant
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k",
                        "test_oracle_parity_on_the_base_scene or test_schedule_equals_per_step_calls"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0, f"DC_FWD_VARIANT={variant}:\n{tail}\n{r.stderr[-2000:]}"
    assert "3 passed" in tail and "failed" not in tail, tail


# ---- 6. unset and reset ----
def test_unset_and_reset_give_the_never_set_result():
    V, F, c, e = base_scene(tight=False)
    N = V.shape[0]
    D = base_offsets()
    X0 = np.stack([f32(V.reshape(-1) + np.tile([0.0, -0.03 * b, 0.0], N)) for b in range(B)])      # (lowered: contacts without any offset)
    V0 = np.zeros_like(X0)

    def run(fused):
        e.set_state(0, X0, V0)
        if fused:
            e.rollout_forward(0, S)
        else:
            for s in range(S):
                e.step_forward(s)
        x, v = e.get_states(0, S + 1)
        return x, v, [e.get_contacts(s + 1) for s in range(S)], np.stack([e.get_primitive_centers(s + 1) for s in range(S)])

    def same(a, b):
        np.testing.assert_array_equal(a[0], b[0]); np.testing.assert_array_equal(a[1], b[1]); np.testing.assert_array_equal(a[3], b[3])
        for p, q in zip(a[2], b[2]):
            np.testing.assert_array_equal(p[0], q[0]); np.testing.assert_array_equal(p[1], q[1])

    e.alloc_batch(B, S)
    never = run(False)
    assert (never[2][-1][0] >= 0).sum() > 10
    np.testing.assert_array_equal(never[3], np.broadcast_to(c, (S, B, 1, 3)))
    same(run(True), never)
    # set_primitive_offsets(None)
    e.set_primitive_offsets(D[0])
    moved = run(False)
    assert np.abs(moved[0][S] - never[0][S]).max() > 1e-6
    e.set_primitive_offsets(None)
    same(run(False), never); same(run(True), never)
    # clear_schedules
    e.set_primitive_offset_schedule(0, D)
    assert np.abs(run(True)[0][S] - never[0][S]).max() > 1e-6
    e.clear_schedules()
    same(run(True), never); same(run(False), never)
    # a fresh alloc_batch drops offsets and schedule
    e.set_primitive_offsets(D[1]); e.set_primitive_offset_schedule(0, D[:2])
    e.alloc_batch(B, S)
    same(run(False), never); same(run(True), never)
    # no primitives: nothing to move
    e2 = engine(V, F, [])
    e2.alloc_batch(1, 1)
    with pytest.raises(capi.DcError, match="no primitives"):
        e2.set_primitive_offsets(np.zeros((1, 1, 3)))
    e2.close(); e.close()


# ---- 7. device pointers ----
def test_device_pointer_setters_fill_the_host_paths_table():
    V, F, c, e = base_scene(tight=False)
    e.alloc_batch(B, S)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(8)
    for D in (base_offsets(), 0.3 * rng.standard_normal((S, B, 1, 3))):           # dyadic, and offsets that are no fp32 numbers
        for dtype in (torch.float32, torch.float64):
            Dh = f32(D) if dtype == torch.float32 else D                           # what the tensor holds
            e.clear_schedules()
            e.set_primitive_offset_schedule(0, Dh)
            host = np.stack([e.get_primitive_centers(s + 1) for s in range(S)])
            np.testing.assert_array_equal(host[:, :, 0], f32(c + Dh[:, :, 0]))
            wide = torch.zeros((S, B, 1, 6), dtype=dtype, device=dev)
            wide[..., :3] = torch.as_tensor(Dh, dtype=dtype)
            for t in (torch.as_tensor(Dh, dtype=dtype).to(dev), wide[..., :3]):    # contiguous, and a strided view the wrapper copies
                e.alloc_batch(B, S)                                                # (every row back to the built centres)
                e.set_primitive_offset_schedule_dev(0, S, t)
                e.sync()
                np.testing.assert_array_equal(np.stack([e.get_primitive_centers(s + 1) for s in range(S)]), host)
            assert not wide[..., :3].is_contiguous()
            # the offsets of the NEXT steps (a schedule entry of the slot would win): the step's row says what it used
            e.clear_schedules()
            X0 = np.tile(f32(V.reshape(-1)), (B, 1))
            e.set_state(0, X0, np.zeros_like(X0))
            e.set_primitive_offsets_dev(torch.as_tensor(Dh[1], dtype=dtype).to(dev))
            e.step_forward(0)
            np.testing.assert_array_equal(e.get_primitive_centers(1), host[1])
            xa, _ = e.get_state(1)
            e.set_primitive_offsets_dev(None)
            e.set_primitive_offsets(Dh[1])
            e.step_forward(0)
            np.testing.assert_array_equal(e.get_state(1)[0], xa)
    e.close()


def test_sim_rollout_takes_primitive_offsets_on_both_paths():
    """sim_rollout(primitive_offsets=...) on CUDA tensors = on CPU tensors (host calls) = per-step calls, bit for bit, with gradients to the
    other inputs over the moved record; [B, G, 3] = the same entry in every step"""
    att = (0, 16)
    V, F, c, e = base_scene(tight=False, att=att)
    N = V.shape[0]
    e.alloc_batch(B, S)
    sim = BatchedSim(e, S)
    D = base_offsets()
    rng = np.random.default_rng(4)
    x0 = np.stack([f32(V.reshape(-1) + np.tile([0.01 * b, 0.0, 0.0], N)) for b in range(B)])
    actions = np.stack([np.stack([f32((V[list(att)] + np.array([0.0, 0.01 * (s + 1), 0.002 * b])).reshape(-1)) for b in range(B)]) for s in range(S)])
    w = f32(1e-3 * rng.standard_normal((S, B, 3 * N)))

    def run(device, po):
        t = lambda a, grad=False: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(device).requires_grad_(grad)
        tx, ta = t(x0, True), t(actions, True)
        xs, vs = sim_rollout(sim, tx, t(np.zeros_like(x0)), ta, primitive_offsets=None if po is None else t(po))
        (xs * t(w)).sum().backward()
        centres = np.stack([e.get_primitive_centers(s + 1) for s in range(S)])
        return xs.detach().cpu().numpy(), vs.detach().cpu().numpy(), tx.grad.cpu().numpy(), ta.grad.cpu().numpy(), centres

    host, devc = run("cpu", D), run("cuda", D)
    np.testing.assert_array_equal(devc[0], host[0]); np.testing.assert_array_equal(devc[1], host[1]); np.testing.assert_array_equal(devc[4], host[4])
    np.testing.assert_array_equal(host[4][:, :, 0], f32(c + D[:, :, 0]))
    assert rel(devc[2], host[2]) <= 2e-6 and rel(devc[3], host[3]) <= 2e-6 and np.abs(host[2]).max() > 0
    # per-step calls
    e.clear_schedules()
    e.set_state(0, x0, np.zeros_like(x0))
    for s in range(S):
        e.set_primitive_offsets(D[s])
        e.step_forward(s, fixed_pts=actions[s])
    xs, vs = e.get_states(1, S)
    np.testing.assert_array_equal(xs.astype(np.float32), devc[0]); np.testing.assert_array_equal(vs.astype(np.float32), devc[1])
    e.set_primitive_offsets(None)
    # constant over the episode, and omitted: the schedule is cleared like the others
    const_h, const_d = run("cpu", D[0]), run("cuda", D[0])
    np.testing.assert_array_equal(const_d[0], const_h[0])
    np.testing.assert_array_equal(const_d[4], np.broadcast_to(f32(c + D[0, :, 0])[None, :, None, :], (S, B, 1, 3)))
    none_d = run("cuda", None)
    np.testing.assert_array_equal(none_d[4], np.broadcast_to(c, (S, B, 1, 3)))
    assert np.abs(none_d[0] - const_d[0]).max() > 1e-6 and np.abs(const_d[0] - devc[0]).max() > 1e-6
    with pytest.raises(ValueError, match="normals.*constant.*reference"):
        sim_rollout(sim, torch.zeros(B, 3 * N), torch.zeros(B, 3 * N), None, steps=S, primitive_offsets=torch.zeros(B, 1, 3, requires_grad=True))
    e.close()


# ---- 8. diffcloth_py: the reference's callers move an obstacle by writing Primitive.center ----
def test_writing_primitive_center_between_steps_moves_the_obstacle(monkeypatch):
    """sim.primitives[0].center = c on the sphere demo (python_interface.cpp:285): the next step equals the C-ABI step with that offset and
    differs from the unmoved one; resetSystem puts the obstacle back (Primitive::reset, Primitive.h:164-166)."""
    sys.path.insert(0, os.path.join(ROOT, "diffcloth_amd", "lib"))
    import diffcloth_py as d
    sim = d.makeSim("sphere")
    monkeypatch.setattr(d.Simulation, "forwardConvergenceThreshold", 1e-7)          # (a static of the module: put back for the tests that follow)
    nsteps = 3
    c0 = np.array(sim.primitives[0].center)
    np.testing.assert_array_equal(c0, np.array(sim.primitives[0].centerInit))
    moves = [np.array([0.0, 0.125, 0.0]), np.array([0.0625, 0.1875, 0.0]), np.array([0.0625, 0.25, -0.03125])]

    def rollout(move):
        sim.resetSystem()
        np.testing.assert_array_equal(np.array(sim.primitives[0].center), c0)          # reset restored the built centre
        out = []
        for s in range(nsteps):
            if move:
                sim.primitives[0].center = c0 + moves[s]
            sim.step()
            rec = sim.getStateInfo()
            out.append((np.array(rec.x), np.array(rec.v)))
        return out

    unmoved, moved, unmoved2 = rollout(False), rollout(True), rollout(False)
    for s in range(nsteps):
        np.testing.assert_array_equal(unmoved[s][0], unmoved2[s][0])                    # ... on the device too
    assert np.abs(moved[0][0] - unmoved[0][0]).max() > 1e-6                             # the write reaches the device: the behavioural gap of the parent
    # the C-ABI path: the same system, the offsets set before every step
    rest = np.array(sim.getRestPositions()).reshape(-1, 3)
    _, F = meshes.grid_cloth(25, 25, 4.5, 4.5, "DOWN")
    e = capi.Engine(0)
    e.set_mesh(rest, F)
    e.set_params(time_step=1.0 / 180, density=0.3, k_stretch=150.0, k_bend=0.00001, forward_tol=1e-7, selfcollision_enabled=1)
    e.set_primitives([dict(kind=capi.DC_PRIM_SPHERE, group=0, center=c0, radius=2.0, mu=0.9)])
    e.build()
    e.alloc_batch(1, nsteps)
    for move, want in ((False, unmoved), (True, moved)):
        e.set_state(0, rest.reshape(1, -1), np.zeros((1, rest.size)))
        for s in range(nsteps):
            e.set_primitive_offsets(moves[s].reshape(1, 1, 3) if move else None)
            e.step_forward(s)
            x, v = e.get_state(s + 1)
            np.testing.assert_array_equal(x[0], want[s][0], err_msg=f"moved {move} step {s}")
            np.testing.assert_array_equal(v[0], want[s][1], err_msg=f"moved {move} step {s}")
    e.close()
