"""Per-rollout obstacle shapes: radius, capsule axis and length, plane corners per rollout and step (dc_set_primitive_shapes,
dc_set_primitive_shape_schedule, their _dev forms, dc_get_primitive_shapes; sim_rollout(primitive_shapes=...), rotated_primitive_shapes).

The rule under test (csrc/dc_primshape.h): a shape row {top_offset[3], corner2[3], radius, length} per rollout and flattened primitive, stored
as fp32 of each value and read by the kernels in place of the built values — so a context GIVEN a shape and a context BUILT with that shape
compute the same step bit for bit, and the fp64 oracle with its obstacle re-added in that fp32 shape is the parity partner. The helpers,
solver settings and gates are those of tests/test_gpu_primitive_offsets.py.

Oracle contact counts of the three parity scenes (free-running from rest; asserted as lower bounds) are in the tests' docstrings.
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
import test_gpu_primitive_offsets as po          # its scene builders and helpers (not its tests)
from diffcloth_amd import capi, workloads
from diffcloth_amd.functional import BatchedSim, rotated_primitive_shapes, sim_rollout

pytestmark = pytest.mark.gpu
ROOT = po.ROOT
H, FABRIC = po.H, po.FABRIC
B, S = 4, 4
f32, rel, contact_ids = po.f32, po.rel, po.contact_ids


def Rx(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def Ry(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def Rz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def clear(o):
    orc.lib().orc_clear_primitives(o.h)
    o.nprim = 0


def rest_state(V, nb):
    X0 = np.tile(f32(V.reshape(-1)), (nb, 1))
    return X0, np.zeros_like(X0)


# ---- 1-3. oracle parity per rollout and step: the statements and gates of po.check_base_scene_against_oracle ----
def check_against_oracle(tag, V, F, prims, SH, readd, want_counts, D=None, backward=True):
    """prims: the built primitive dicts; SH: [steps][nb][P][8] fp64 shape schedule; readd(o, s, b): puts rollout b's obstacle of step s into the
    cleared oracle o, in the fp32 shape and at the fp32 centre the device uses; want_counts[b]: the oracle's contact counts per step (an int:
    the same in every step), lower bounds — 0 means none at all; D: [steps][nb][G][3] offset schedule or None. Returns the contact sets."""
    nsteps, nb = SH.shape[0], SH.shape[1]
    N = V.shape[0]
    e = po.engine(V, F, prims)
    e.alloc_batch(nb, nsteps)
    X0, V0 = rest_state(V, nb)
    e.set_state(0, X0, V0)
    e.set_primitive_shape_schedule(0, SH)
    if D is not None:
        e.set_primitive_offset_schedule(0, D)
    oracles = [po.sphere_oracle(V, F) for _ in range(nb)]
    rng = np.random.default_rng(31)
    sets = [[None] * nb for _ in range(nsteps)]
    lines = []
    for s in range(nsteps):
        xs, vs = e.get_state(s)
        st = e.step_forward(s)                        # the per-step call honours the schedule entry of its slot
        x1, v1 = e.get_state(s + 1)
        grp, nrm = e.get_contacts(s + 1)
        fr = e.get_record(s + 1)[0]
        np.testing.assert_array_equal(e.get_primitive_shapes(s + 1), f32(SH[s]))            # the fp32-rounded schedule
        gx = f32(rng.standard_normal((nb, 3 * N))); gv = f32(0.01 * rng.standard_normal((nb, 3 * N)))
        gb = e.step_backward(s + 1, gx, gv) if backward else None
        for b in range(nb):
            o = oracles[b]
            clear(o)
            readd(o, s, b)
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
                assert ex <= 1e-4 and ev <= 1e-4, line
                assert ea <= 1e-4, line
            lines.append(line)
    print(f"\n[primitive shapes, {tag}]\n" + "\n".join(lines))
    # what keeps the test from being vacuous: the oracle's own counts as lower bounds
    for b in range(nb):
        for s in range(nsteps):
            want = want_counts[b] if np.isscalar(want_counts[b]) else want_counts[b][s]
            if want == 0:
                assert len(sets[s][b]) == 0, (b, s, len(sets[s][b]))
            else:
                assert len(sets[s][b]) >= want, (b, s, len(sets[s][b]), want)
    e.close()
    return sets


def base_radii():
    """[S][B] radius of the base scene's sphere (built with 2.0)"""
    r = np.zeros((S, B))
    r[:, 0], r[:, 1], r[:, 2] = 2.125, 2.375, 0.5
    for s in range(S):
        r[s, 3] = 2.0 + 0.0625 * (s + 1)
    return r


def radius_schedule(e, radii):
    """[steps][nb][P = 1][8]: the built row with the radius replaced"""
    SH = np.tile(e.built_primitive_shapes(), radii.shape + (1, 1))
    SH[..., 0, 6] = radii
    return SH


def check_sphere_radius_against_oracle(backward=True):
    V, F, c, e = po.base_scene()
    radii = base_radii()
    SH = radius_schedule(e, radii)
    e.close()
    prims = [dict(kind=capi.DC_PRIM_SPHERE, group=0, center=c, radius=2.0, mu=0.4)]
    sets = check_against_oracle("sphere radius", V, F, prims, SH, lambda o, s, b: o.add_sphere(c, float(f32(radii[s, b])), 0.4),
                                [22, 66, 0, (10, 22, 33, 43)], backward=backward)
    for s in range(S):
        assert sets[s][1] != sets[s][0] and sets[s][3] != sets[s][1]


def test_oracle_parity_sphere_radius_per_rollout_and_step():
    """the 17 x 17 cloth over the sphere built with radius 2.0 (which alone gives 0 / 0 / 0 / 1 contacts: a run that ignores the table fails on the
    contact sets); radius 2.125: 22 contacts in every step, 2.375: 66, 0.5: none, growing 2.0 + 0.0625 (s + 1): 10 / 22 / 33 / 43"""
    check_sphere_radius_against_oracle()


def test_oracle_parity_tilted_plane():
    """the 22 x 22 cloth on the rectangle ul = (-1.5, 0, -1.5), ur = (1.5, 0, -1.5), corners rotated per rollout with rotated_primitive_shapes:
    identity 196 contacts in every step, Rx(-0.2) 140, Rz(0.15) 168, Ry(0.6) 196 (another set), Rx(-0.05 (s + 1)) 196 / 196 / 154 / 140"""
    V, F = meshes.grid_cloth(22, 22, 4.5, 4.5, "DOWN")
    V = f32(V)
    c = f32(V.mean(axis=0) + np.array([0.13, -0.25, 0.07]))
    ul, ur = np.array([-1.5, 0.0, -1.5]), np.array([1.5, 0.0, -1.5])
    prims = [dict(kind=capi.DC_PRIM_PLANE, group=0, center=c, top_offset=ul, corner2=ur, radius=0.0, mu=0.2)]
    nb = 5
    R = np.zeros((S, nb, 1, 3, 3))
    for s in range(S):
        R[s, :, 0] = [np.eye(3), Rx(-0.2), Rz(0.15), Ry(0.6), Rx(-0.05 * (s + 1))]
    built = np.array([[*ul, *ur, 0.0, 0.0]])
    SH = rotated_primitive_shapes(torch.as_tensor(built), torch.as_tensor(R)).numpy()
    assert SH.shape == (S, nb, 1, 8) and SH.dtype == np.float64
    np.testing.assert_allclose(SH[2, 1, 0, 0:3], Rx(-0.2) @ ul, atol=1e-15)
    sets = check_against_oracle("tilted plane", V, F, prims, SH, lambda o, s, b: o.add_plane(c, f32(SH[s, b, 0, 0:3]), f32(SH[s, b, 0, 3:6]), 0.2),
                                [196, 140, 168, 196, (196, 196, 154, 140)])
    for s in range(S):
        assert sets[s][3] != sets[s][0] and sets[s][1] != sets[s][0] and sets[s][2] != sets[s][1]


def test_oracle_parity_capsule_axis_radius_and_centre():
    """the 17 x 17 cloth on a capsule of length 3 lying under it, top = f32(R (0, 3, 0)), centre f32(mid - (0, 0.65, 0) - top / 2): the centre
    depends on the axis, so it goes through the offset schedule (offsets and shapes set together). Axis along x, radius 0.5: 12 contacts; along z:
    12, another set; diagonal: 24; along x with radius 0.75: 69; Rz(-pi/2 + 0.2): 28"""
    V, F = meshes.grid_cloth(17, 17, 4.5, 4.5, "DOWN")
    V = f32(V)
    mid = V.mean(axis=0)
    rots = [Rz(-np.pi / 2), Rx(np.pi / 2), Ry(np.pi / 4) @ Rz(-np.pi / 2), Rz(-np.pi / 2), Rz(-np.pi / 2 + 0.2)]
    radii = [0.5, 0.5, 0.5, 0.75, 0.5]
    nb, nsteps = len(rots), 2
    tops = np.stack([f32(Rm @ np.array([0.0, 3.0, 0.0])) for Rm in rots])
    centres = np.stack([f32(mid - np.array([0.0, 0.65, 0.0]) - tops[b] / 2) for b in range(nb)])
    prims = [dict(kind=capi.DC_PRIM_CAPSULE, group=0, center=centres[0], top_offset=tops[0], radius=0.5, length=3.0, mu=0.4)]
    SH = np.zeros((nsteps, nb, 1, 8))
    SH[:, :, 0, 0:3] = tops
    SH[:, :, 0, 6] = radii
    SH[:, :, 0, 7] = 3.0
    D = np.zeros((nsteps, nb, 1, 3))
    D[:, :, 0] = centres - centres[0]                  # (a difference of fp32 numbers: exact in fp64, so fp32(built + d) is the wanted centre)
    np.testing.assert_array_equal(f32(centres[0] + D[0, :, 0]), centres)
    sets = check_against_oracle("capsule", V, F, prims, SH, lambda o, s, b: o.add_capsule(centres[b], tops[b], radii[b], 3.0, 0.4),
                                [12, 12, 24, 69, 28], D=D)
    for s in range(nsteps):
        assert sets[s][1] != sets[s][0] and sets[s][3] != sets[s][0] and sets[s][4] != sets[s][0]


# ---- 4. bit for bit against a context built with the shape, every primitive kind ----
def run_steps(e, X0, V0, nsteps, shapes=None, offsets=None, velocities=None):
    """nsteps per-step calls from (X0, V0); everything a step leaves behind"""
    nb = X0.shape[0]
    e.alloc_batch(nb, nsteps)
    if shapes is not None:
        e.set_primitive_shapes(shapes)
    if offsets is not None:
        e.set_primitive_offsets(offsets)
    if velocities is not None:
        e.set_primitive_velocities(velocities)
    e.set_state(0, X0, V0)
    out = []
    for s in range(nsteps):
        st = e.step_forward(s)
        x, v = e.get_state(s + 1)
        grp, nrm = e.get_contacts(s + 1)
        f, r = e.get_record(s + 1)
        out.append(dict(x=x, v=v, grp=grp, nrm=nrm, f=f, r=r, contacts=st["prim_contacts"].copy(), shapes=e.get_primitive_shapes(s + 1),
                        centres=e.get_primitive_centers(s + 1)))
    return out


def with_shape(p, row):
    """the primitive dict p built with the fp64 shape row"""
    return dict(p, top_offset=row[0:3].copy(), corner2=row[3:6].copy(), radius=float(row[6]), length=float(row[7]))


def check_shapes_equal_built(V, F, prims, SH, X0, V0, monkeypatch, nsteps=2, min_contacts=5, fabric=FABRIC, h=H, Doff=None, W=None):
    """prims: engine primitive dicts; SH: [nb][P][8] fp64 rows; rollout b of the context given SH against rollout b of a context whose primitives
    were BUILT with row b (same batch size, one workgroup per rollout). Doff [nb][G][3] / W [nb][G][3]: offsets and velocities set as well — the
    built context then stands at center + Doff[b] (the sum formed in fp64 by the caller) and is given the same velocities."""
    monkeypatch.setenv("DC_CLUSTER", "1")
    nb = X0.shape[0]
    groups = []
    for p in prims:
        if p["group"] not in groups:
            groups.append(p["group"])
    assert any(float(np.float32(v)) != v for v in SH.reshape(-1)), "at least one value that is no fp32 number: the rounding happens once"
    e = po.engine(V, F, prims, fwd_tol=1e-7, fabric=fabric, h=h)
    got = run_steps(e, X0, V0, nsteps, shapes=SH, offsets=Doff, velocities=W)
    assert e.cluster() == 1
    e.close()
    for b in range(nb):
        built = [with_shape(p, SH[b, k]) for k, p in enumerate(prims)]
        if Doff is not None:
            built = [dict(p, center=np.asarray(p["center"], dtype=np.float64) + Doff[b, groups.index(p["group"])]) for p in built]
        em = po.engine(V, F, built, fwd_tol=1e-7, fabric=fabric, h=h)
        want = run_steps(em, X0, V0, nsteps, velocities=W)
        em.close()
        for s in range(nsteps):
            for key in ("x", "v", "grp", "nrm", "f", "r", "shapes", "centres"):
                np.testing.assert_array_equal(got[s][key][b], want[s][key][b], err_msg=f"rollout {b} step {s} {key}")
            np.testing.assert_array_equal(got[s]["shapes"][b], f32(SH[b]))
            assert got[s]["contacts"][b] >= min_contacts, (b, s, got[s]["contacts"])
    return got


def sphere_case():
    V, F = meshes.grid_cloth(17, 17, 4.5, 4.5, "DOWN")
    V = f32(V)
    c = f32(meshes.sphere_scene_center(V, 2.0))
    prims = [dict(kind=capi.DC_PRIM_SPHERE, group=0, center=c, radius=2.0, mu=0.4)]
    SH = np.zeros((3, 1, 8))
    SH[:, 0, 6] = (2.125 + 1e-9, 2.375, 2.25 + 1e-3)
    return V, F, prims, SH


def test_shape_equals_build_sphere(monkeypatch):
    V, F, prims, SH = sphere_case()
    X0, V0 = rest_state(V, 3)
    got = check_shapes_equal_built(V, F, prims, SH, X0, V0, monkeypatch, min_contacts=20)
    assert set(contact_ids(got[0]["grp"][0])) != set(contact_ids(got[0]["grp"][1]))


def test_shape_equals_build_tilted_plane(monkeypatch):
    V, F = meshes.grid_cloth(22, 22, 4.5, 4.5, "DOWN")
    V = f32(V)
    c = f32(V.mean(axis=0) + np.array([0.13, -0.25, 0.07]))
    ul, ur = np.array([-1.5, 0.0, -1.5]), np.array([1.5, 0.0, -1.5])
    prims = [dict(kind=capi.DC_PRIM_PLANE, group=0, center=c, top_offset=ul, corner2=ur, radius=0.0, mu=0.2)]
    R = np.stack([Rx(-0.2), Rz(0.15), Ry(0.6) @ Rx(-0.1)])[:, None]
    SH = rotated_primitive_shapes(torch.as_tensor(np.array([[*ul, *ur, 0.0, 0.0]])), torch.as_tensor(R)).numpy()       # fp64 rotations: no fp32 numbers
    X0, V0 = rest_state(V, 3)
    got = check_shapes_equal_built(V, F, prims, SH, X0, V0, monkeypatch, min_contacts=50)
    a, b = set(contact_ids(got[0]["grp"][0])), set(contact_ids(got[0]["grp"][1]))
    assert a != b and len(a) < V.shape[0] and len(b) < V.shape[0]


def test_shape_equals_build_bowl_radius(monkeypatch):
    """the sheet of po's bowl test laid on the shell of the GIVEN radius across its equator (built radius 1.0: out of reach of either sheet)"""
    V, F = meshes.grid_cloth(14, 14, 1.3, 1.3, "DOWN")
    V = f32(V)
    c = f32(np.array([V[:, 0].mean(), 0.0, V[:, 2].mean()]))
    radii = (1.2 + 1e-9, 1.3125)
    X0, V0 = [], []
    for Rb in radii:
        u, w = (V[:, 0] - V[:, 0].mean()) / Rb, (V[:, 2] - V[:, 2].mean()) / Rb           # elevation / azimuth of the sheet's vertices on the shell
        unit = np.stack([np.cos(u) * np.cos(w), np.sin(u), np.cos(u) * np.sin(w)], axis=1)
        X0.append(f32((c + Rb * unit).reshape(-1)))
        V0.append(f32((0.3 * unit).reshape(-1)))                                           # moving outwards, onto the shell
    X0, V0 = np.stack(X0), np.stack(V0)
    SH = np.zeros((2, 1, 8))
    SH[:, 0, 6] = radii
    got = check_shapes_equal_built(V, F, [dict(kind=capi.DC_PRIM_BOWL, group=0, center=c, radius=1.0, mu=0.4)], SH, X0, V0, monkeypatch, nsteps=1, min_contacts=40)
    for b in range(2):
        ids = contact_ids(got[0]["grp"][b])
        y = X0[b].reshape(-1, 3)[:, 1]
        assert (y[ids] <= c[1]).all() and (y > c[1]).sum() >= 40 and len(ids) < V.shape[0]      # "below the centre" stays world-up


def test_shape_equals_build_lower_leg_children(monkeypatch):
    """the LowerLeg of po.leg_scene (joint sphere, foot capsule, leg capsule: one group, three flattened primitives) — every child has its own row:
    its own radius, and the capsules their own axis and length"""
    V, F, center, prims = po.leg_scene()
    built = np.array([[*p["top_offset"], 0.0, 0.0, 0.0, p["radius"], p["length"]] for p in prims], dtype=np.float64)
    SH = np.stack([built, built])
    # rollout 0: thicker joint and foot, the foot capsule swung by 0.1 about z and 1/8 longer, the leg capsule thinner
    SH[0, 0, 6] = built[0, 6] * 1.125 + 1e-9
    SH[0, 1, 0:3] = Rz(0.1) @ built[1, 0:3] * (1 + 1 / 32)
    SH[0, 1, 6], SH[0, 1, 7] = built[1, 6] * 1.25, built[1, 7] * (1 + 1 / 32)
    SH[0, 2, 6] = built[2, 6] * 0.875
    # rollout 1: thicker leg capsule swung by -0.15 about x, thinner foot, the joint 1/16 larger
    SH[1, 0, 6] = built[0, 6] + 0.0625
    SH[1, 1, 6] = built[1, 6] * 0.9375
    SH[1, 2, 0:3] = Rx(-0.15) @ built[2, 0:3]
    SH[1, 2, 6] = built[2, 6] * 1.125 + 1e-9
    mid = V.mean(axis=0)
    X0 = np.stack([f32((V + (center + np.array([0.0, height, 0.0]) - mid)).reshape(-1)) for height in (2.0, 4.1)])     # around the foot / at the joint
    V0 = np.zeros_like(X0)
    got = check_shapes_equal_built(V, F, prims, SH, X0, V0, monkeypatch, min_contacts=8)
    for b in range(2):
        assert set(got[0]["grp"][b][contact_ids(got[0]["grp"][b])].tolist()) == {7}       # contacts report the caller's group id
    # the table is what made the difference: the built shapes give another step
    e = po.engine(V, F, prims, fwd_tol=1e-7)
    plain = run_steps(e, X0, V0, 1)
    e.close()
    assert all(np.abs(plain[0]["x"][b] - got[0]["x"][b]).max() > 1e-6 for b in range(2))


def test_shape_with_a_discretised_sphere_in_the_context(monkeypatch):
    """po's BIG_SPHERE scene (radius 15, face normals) with a small plain sphere above the sheet, first in the list: the discretised sphere's own
    row, equal to the built one, is accepted by the host form — the kernels do not read it —, another row for it is refused, and the small
    sphere's row is honoured: given radius 1.25 it reaches the sheet (built 0.5: out of reach)"""
    V, F = meshes.grid_cloth(22, 22, 4.5, 4.5, "DOWN")
    V = f32(V)
    Rbig = 15.0
    c = np.array([-0.5, -16.0, 0.0])
    X = V.copy()
    X[:, 0] += c[0] - V[:, 0].mean() + 0.37; X[:, 2] += c[2] - V[:, 2].mean() - 0.21      # (off the mesh's symmetry lines)
    X[:, 1] = c[1] + np.sqrt(Rbig * Rbig - (X[:, 0] - c[0]) ** 2 - (X[:, 2] - c[2]) ** 2) + 0.02
    X0 = np.tile(f32(X.reshape(-1)), (2, 1))
    vel = np.zeros_like(V); vel[:, 1] = -0.3; vel[:, 0] = 0.2
    V0 = np.tile(f32(vel.reshape(-1)), (2, 1))
    apex = X[np.argmax(X[:, 1])]
    small = f32(apex + np.array([0.0, 1.3, 0.0]))
    prims = [dict(kind=capi.DC_PRIM_SPHERE, group=5, center=small, radius=0.5, mu=0.4),
             dict(kind=capi.DC_PRIM_SPHERE_DISCRETIZED, group=2, center=c, radius=Rbig, mu=0.3)]
    SH = np.zeros((2, 2, 8))
    SH[:, 1, 6] = Rbig                                  # the discretised sphere's own row (length 0 = the default resolution, as built)
    SH[:, 0, 6] = (1.25 + 1e-9, 1.3125)
    got = check_shapes_equal_built(V, F, prims, SH, X0, V0, monkeypatch, nsteps=1, min_contacts=400)
    for b in range(2):
        g = got[0]["grp"][b]
        assert (g == 5).sum() >= 3 and (g == 2).sum() >= 300, ((g == 5).sum(), (g == 2).sum())
    e = po.engine(V, F, prims, fwd_tol=1e-7)
    e.alloc_batch(2, 1)
    plain = run_steps(e, X0, V0, 1)
    assert (plain[0]["grp"] == 5).sum() == 0            # the built small sphere touches nothing
    bad = SH.copy()
    bad[1, 1, 6] = Rbig + 0.5
    with pytest.raises(capi.DcError, match="discretised"):
        e.set_primitive_shapes(bad)
    with pytest.raises(capi.DcError, match="discretised"):
        e.set_primitive_shape_schedule(0, bad[None])
    e.set_primitive_shapes(SH)                          # and the refusals left nothing behind
    e.close()


def test_offset_velocity_and_shape_together_equal_the_moved_build(monkeypatch):
    """all three per-rollout tables at once, against a context built at the moved centre with the shape and given the same velocity"""
    V, F, prims, SH = sphere_case()
    SH = SH[:2]
    D = np.array([[[0.0, 0.0625, 0.0]], [[0.125, 0.03125 + 1e-9, -0.0625]]])
    W = np.array([[[0.5, 0.0, 0.25]], [[-0.25, 0.125, 0.0]]])
    X0, V0 = rest_state(V, 2)
    got = check_shapes_equal_built(V, F, prims, SH, X0, V0, monkeypatch, min_contacts=20, Doff=D, W=W)
    c = np.asarray(prims[0]["center"])
    for b in range(2):
        np.testing.assert_array_equal(got[0]["centres"][b, 0], f32(c + D[b, 0]))
    # each of the three matters here
    e = po.engine(V, F, prims, fwd_tol=1e-7)
    for drop in ("shapes", "offsets", "velocities"):
        kw = dict(shapes=SH, offsets=D, velocities=W)
        kw[drop] = None
        other = run_steps(e, X0, V0, 2, **kw)
        assert np.abs(other[1]["x"] - got[1]["x"]).max() > 1e-6, drop
    e.close()


# ---- 5. self collision: detection (which seeds the layering with the primitive contacts) and the step kernel see the same shape ----
def test_self_collision_layers_follow_the_radius(monkeypatch):
    """the scene of po.test_self_collision_layers_follow_the_moved_sphere with the per-rollout difference in the RADIUS: the sphere is built
    under the flap (at po's moved centre of rollout 0) with a radius that keeps it out of reach, and the table gives rollout 0 the scene's
    radius — po's rollout 0 — and rollout 1 one 1/16 smaller. Layers, pairs and primitive contacts of the per-step path and of the fused
    sweep (detection inlined) are those of a context built with that radius."""
    monkeypatch.setenv("DC_CLUSTER", "1")
    cfg = workloads.C4_CLOTH
    V, F, Vf, flap, c = workloads.c4_scene(grid=16, fold_rows=3, fold_gap=0.02)
    fabric = dict(density=cfg["density"], k_stretch=cfg["k_stretch"], k_bend=cfg["k_bend"])
    to_flap = Vf[flap].mean(axis=0) - c
    centre = c + np.round(np.array([to_flap[0], 0.0, to_flap[2]]) * 32) / 32 + np.array([0.0, 0.125, 0.0])
    r0 = cfg["sphere_radius"]
    prim = dict(kind=capi.DC_PRIM_SPHERE, group=0, center=centre, radius=r0 - 0.5, mu=cfg["sphere_mu"])
    nb, nsteps = 2, 2
    radii = (r0, r0 - 0.0625 + 1e-9)
    SH = np.zeros((nb, 1, 8))
    SH[:, 0, 6] = radii
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

    e = po.engine(V, F, [prim], selfcollision=1, fabric=fabric)
    e.alloc_batch(nb, nsteps)
    e.set_primitive_shapes(SH)
    e.set_state(0, X0, V0)
    for s in range(nsteps):
        e.step_forward(s)
    stepwise = collect(e)
    e.set_state(0, X0, V0)
    e.rollout_forward(0, nsteps)                    # fused: the detection of every step runs inside the step kernel's launch
    same(collect(e), stepwise, range(nb))
    e.set_primitive_shapes(None)                    # the built radius: out of reach, no primitive contact seeds the layering
    e.set_state(0, X0, V0)
    e.rollout_forward(0, nsteps)
    assert all((q["grp"] >= 0).sum() == 0 for q in collect(e))
    e.close()
    for b in range(nb):
        em = po.engine(V, F, [dict(prim, radius=radii[b])], selfcollision=1, fabric=fabric)
        em.alloc_batch(nb, nsteps)
        em.set_state(0, X0, V0)
        em.rollout_forward(0, nsteps)
        same(collect(em), stepwise, [b])
        em.close()
    for s in range(nsteps):
        ids = contact_ids(stepwise[s]["grp"][0])
        got = stepwise[s]["selfc"][0]
        assert len(ids) >= 5 and got["count"] >= 10
        # the frontier matters here: vertices in primitive contact take part in self contacts
        assert len(set(ids.tolist()) & set(got["pairs"].reshape(-1).tolist())) > 0, f"step {s}: no vertex in both kinds of contact"
    assert set(contact_ids(stepwise[0]["grp"][0])) != set(contact_ids(stepwise[0]["grp"][1]))


# ---- 6. schedule = per-step calls, bitwise ----
def check_schedule_equals_per_step_calls(nx, cluster, monkeypatch):
    if cluster:
        monkeypatch.setenv("DC_CLUSTER", str(cluster))
    V, F, c, e = po.base_scene(nx, tight=(nx == 17))
    N = V.shape[0]
    SH = radius_schedule(e, base_radii())
    e.alloc_batch(B, S)
    assert e.cluster() == (cluster if cluster else 1)
    rng = np.random.default_rng(5)
    X0, V0 = rest_state(V, B)
    # ---- (a) per-step calls: the shapes of a step set before it
    e.set_state(0, X0, V0)
    for s in range(S):
        e.set_primitive_shapes(SH[s])
        e.step_forward(s)
        np.testing.assert_array_equal(e.get_primitive_shapes(s + 1), f32(SH[s]))
    xa, va = e.get_states(0, S + 1)
    ca = [e.get_contacts(s + 1) for s in range(S)]
    assert all((ca[s][0][b] >= 0).sum() >= 10 for s in range(S) for b in (0, 1, 3)) and all((ca[s][0][2] >= 0).sum() == 0 for s in range(S))
    gx = f32(rng.standard_normal((B, 3 * N))); gv = f32(0.01 * rng.standard_normal((B, 3 * N)))
    cx, cv = gx, gv
    for s in range(S, 0, -1):
        out = e.step_backward(s, cx, cv, is_start=(s == 1))
        cx, cv = out["dL_dx"], out["dL_dv"]
    # ---- (b) the schedule + one launch per direction
    e.set_primitive_shapes(None)
    e.set_state(0, X0, V0)
    e.set_primitive_shape_schedule(0, SH)
    e.rollout_forward(0, S)
    xb, vb = e.get_states(0, S + 1)
    np.testing.assert_array_equal(xa, xb)
    np.testing.assert_array_equal(va, vb)
    for s in range(S):
        np.testing.assert_array_equal(e.get_primitive_shapes(s + 1), f32(SH[s]))
        cb = e.get_contacts(s + 1)
        np.testing.assert_array_equal(ca[s][0], cb[0]); np.testing.assert_array_equal(ca[s][1], cb[1])
    e.set_gradient(gx, gv)
    e.rollout_backward(S, S)
    dx, dv, _ = e.get_gradient()
    print(f"\n[primitive shape schedule nx={nx} K={e.cluster()}] backward sweep vs per-step calls: dL_dx {rel(dx, cx):.2e} dL_dv {rel(dv, cv):.2e}")
    assert rel(dx, cx) <= 2e-6 and rel(dv, cv) <= 2e-6
    # ---- a schedule that covers only part of a FUSED sweep is an error, not a silent mix (the split kernels and the packet kernels fuse; the
    # resident / global-memory families of DC_FWD_VARIANT run a rollout step by step, where every step takes its own entry or the current shapes)
    built = np.broadcast_to(f32(e.built_primitive_shapes()), (B, 1, 8))
    e.clear_schedules()
    e.set_primitive_shape_schedule(0, SH[:2])
    if cluster or os.environ.get("DC_FWD_VARIANT") is None:
        with pytest.raises(capi.DcError, match="covers only part"):
            e.rollout_forward(0, S)
    else:
        e.set_state(0, X0, V0)
        e.rollout_forward(0, S)
        for s in range(S):
            np.testing.assert_array_equal(e.get_primitive_shapes(s + 1), f32(SH[s]) if s < 2 else built)
    e.clear_schedules()
    e.set_state(0, X0, V0)
    e.rollout_forward(0, S)                          # and without a schedule the current shapes (the built ones) apply again
    xc, _ = e.get_states(S, 1)
    assert np.abs(xc[0] - xa[S]).max() > 1e-6
    for s in range(S):
        np.testing.assert_array_equal(e.get_primitive_shapes(s + 1), built)
    e.close()


@pytest.mark.parametrize("nx,cluster", [(17, 0), (48, 4)])
def test_schedule_equals_per_step_calls(nx, cluster, monkeypatch):
    check_schedule_equals_per_step_calls(nx, cluster, monkeypatch)


# ---- 7. the other kernel families ----
@pytest.mark.parametrize("name", ["DC_DENSE_MAX_N", "DC_WINDOWS"])
def test_kernel_families_selected_at_build(name, monkeypatch):
    """DC_DENSE_MAX_N=0: the packet kernel's PCG instead of the explicit inverse small meshes get; DC_WINDOWS=0: the global-memory corner passes
    (resident kernel). Both are read at dc_build."""
    monkeypatch.setenv(name, "0")
    _, _, _, e = po.base_scene()
    lay = e.layout()
    assert not (lay["dense_inverse"] if name == "DC_DENSE_MAX_N" else lay["element_windows"])
    e.close()
    check_sphere_radius_against_oracle(backward=False)
    check_schedule_equals_per_step_calls(17, 0, monkeypatch)
    V, F, prims, SH = sphere_case()
    X0, V0 = rest_state(V, 3)
    check_shapes_equal_built(V, F, prims, SH, X0, V0, monkeypatch, min_contacts=20)


@pytest.mark.parametrize("variant", ["global", "0", "1"])
def test_kernel_families_selected_per_process(variant):
    """DC_FWD_VARIANT is read once per process by the launchers: the built-shape comparison and test 6 in a child process per value"""
    env = dict(os.environ)
    env["DC_FWD_VARIANT"] = variant
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k",
                        "test_shape_equals_build_sphere or test_schedule_equals_per_step_calls"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0, f"DC_FWD_VARIANT={variant}:\n{tail}\n{r.stderr[-2000:]}"
    assert "3 passed" in tail and "failed" not in tail, tail


# ---- 8. unset and reset ----
def test_unset_and_reset_give_the_never_set_result():
    V, F, c, e = po.base_scene(tight=False)
    N = V.shape[0]
    SH = radius_schedule(e, base_radii())
    built = np.broadcast_to(f32(e.built_primitive_shapes()), (B, 1, 8))
    X0 = np.stack([f32(V.reshape(-1) + np.tile([0.0, -0.03 * b, 0.0], N)) for b in range(B)])      # (lowered: contacts with the built radius)
    V0 = np.zeros_like(X0)

    def run(fused):
        e.set_state(0, X0, V0)
        if fused:
            e.rollout_forward(0, S)
        else:
            for s in range(S):
                e.step_forward(s)
        x, v = e.get_states(0, S + 1)
        return x, v, [e.get_contacts(s + 1) for s in range(S)], np.stack([e.get_primitive_shapes(s + 1) for s in range(S)])

    def same(a, b):
        np.testing.assert_array_equal(a[0], b[0]); np.testing.assert_array_equal(a[1], b[1]); np.testing.assert_array_equal(a[3], b[3])
        for p, q in zip(a[2], b[2]):
            np.testing.assert_array_equal(p[0], q[0]); np.testing.assert_array_equal(p[1], q[1])

    e.alloc_batch(B, S)
    never = run(False)                               # no table exists: the kernels read the built primitive table
    assert (never[2][-1][0] >= 0).sum() > 10
    np.testing.assert_array_equal(never[3], np.broadcast_to(built, (S, B, 1, 8)))
    same(run(True), never)
    # a table holding the built shapes (the caller's unrounded rows)
    e.set_primitive_shapes(np.broadcast_to(e.built_primitive_shapes(), (B, 1, 8)))
    same(run(False), never); same(run(True), never)
    # set_primitive_shapes(None) after a set
    e.set_primitive_shapes(SH[0])
    changed = run(False)
    assert np.abs(changed[0][S] - never[0][S]).max() > 1e-6
    e.set_primitive_shapes(None)
    same(run(False), never); same(run(True), never)
    # clear_schedules
    e.set_primitive_shape_schedule(0, SH)
    assert np.abs(run(True)[0][S] - never[0][S]).max() > 1e-6
    e.clear_schedules()
    same(run(True), never); same(run(False), never)
    # a sweep with a schedule on only some of its steps
    e.set_primitive_shape_schedule(1, SH[:2])
    e.set_state(0, X0, V0)
    if os.environ.get("DC_FWD_VARIANT") is None:
        with pytest.raises(capi.DcError, match="code 1.*covers only part"):
            e.rollout_forward(0, S)
    # a fresh alloc_batch drops table and schedule
    e.set_primitive_shapes(SH[1])
    e.alloc_batch(B, S)
    same(run(False), never); same(run(True), never)
    # non-finite values are refused by the host forms, and leave the current shapes alone
    bad = SH[0].copy()
    bad[1, 0, 6] = np.nan
    with pytest.raises(capi.DcError, match="code 1.*non-finite"):
        e.set_primitive_shapes(bad)
    bad[1, 0, 6] = np.inf
    with pytest.raises(capi.DcError, match="code 1.*non-finite"):
        e.set_primitive_shape_schedule(0, bad[None])
    same(run(False), never)
    # no primitives: nothing to shape
    e2 = po.engine(V, F, [])
    e2.alloc_batch(1, 1)
    with pytest.raises(capi.DcError, match="code 1.*no primitives"):
        e2.set_primitive_shapes(np.zeros((1, 0, 8)))
    with pytest.raises(capi.DcError, match="code 1.*no primitives"):
        e2.set_primitive_shapes(None)
    e2.close(); e.close()


# ---- 9. device pointers ----
def test_device_pointer_setters_fill_the_host_paths_table():
    V, F, c, e = po.base_scene(tight=False)
    e.alloc_batch(B, S)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(8)
    noisy = radius_schedule(e, base_radii())
    noisy[..., 0, 0:6] = 0.3 * rng.standard_normal((S, B, 6))                       # (a sphere reads only the radius: the other values just travel)
    noisy[..., 0, 6] += 1e-3 * rng.standard_normal((S, B))
    for SH in (radius_schedule(e, base_radii()), noisy):                            # dyadic, and values that are no fp32 numbers
        for dtype in (torch.float32, torch.float64):
            Sh = f32(SH) if dtype == torch.float32 else SH                          # what the tensor holds
            e.alloc_batch(B, S)
            e.set_primitive_shape_schedule(0, Sh)
            host = np.stack([e.get_primitive_shapes(s + 1) for s in range(S)])
            np.testing.assert_array_equal(host, f32(Sh))
            wide = torch.zeros((S, B, 1, 16), dtype=dtype, device=dev)
            wide[..., :8] = torch.as_tensor(Sh, dtype=dtype)
            for t in (torch.as_tensor(Sh, dtype=dtype).to(dev), wide[..., :8]):     # contiguous, and a strided view the wrapper copies
                e.alloc_batch(B, S)                                                 # (the table is gone: the _dev form is its first setter)
                e.set_primitive_shape_schedule_dev(0, S, t)
                e.sync()
                np.testing.assert_array_equal(np.stack([e.get_primitive_shapes(s + 1) for s in range(S)]), host)
            assert not wide[..., :8].is_contiguous()
            # the shapes of the NEXT steps (a schedule entry of the slot would win): the step's row says what it used, and the step is the host form's
            e.clear_schedules()
            X0, V0 = rest_state(V, B)
            e.set_state(0, X0, V0)
            e.set_primitive_shapes_dev(torch.as_tensor(Sh[1], dtype=dtype).to(dev))
            st = e.step_forward(0)
            assert st["prim_contacts"][1] >= 20
            np.testing.assert_array_equal(e.get_primitive_shapes(1), host[1])
            xa, _ = e.get_state(1)
            e.set_primitive_shapes_dev(None)
            e.step_forward(0)
            np.testing.assert_array_equal(e.get_primitive_shapes(1), np.broadcast_to(f32(e.built_primitive_shapes()), (B, 1, 8)))
            assert np.abs(e.get_state(1)[0] - xa).max() > 1e-6
            e.set_primitive_shapes(Sh[1])
            e.step_forward(0)
            np.testing.assert_array_equal(e.get_state(1)[0], xa)
    e.close()


# ---- 10. sim_rollout ----
def test_sim_rollout_takes_primitive_shapes_on_both_paths():
    """sim_rollout(primitive_shapes=...) on CUDA tensors = on CPU tensors (host calls) = per-step engine calls, bit for bit; [B, P, 8] = the same
    row in every step; gradients to x0, actions, mu and primitive_velocities still flow over the record the shapes made"""
    att = (0, 16)
    V, F, c, e = po.base_scene(tight=False, att=att)
    N = V.shape[0]
    e.alloc_batch(B, S)
    sim = BatchedSim(e, S)
    SH = radius_schedule(e, base_radii())
    built = np.broadcast_to(f32(e.built_primitive_shapes()), (S, B, 1, 8))
    rng = np.random.default_rng(4)
    x0 = np.stack([f32(V.reshape(-1) + np.tile([0.01 * b, 0.0, 0.0], N)) for b in range(B)])
    actions = np.stack([np.stack([f32((V[list(att)] + np.array([0.0, 0.01 * (s + 1), 0.002 * b])).reshape(-1)) for b in range(B)]) for s in range(S)])
    mu0 = np.full((B, 1), 0.4)
    pv0 = np.zeros((S, B, 1, 3)); pv0[..., 0] = 0.25
    w = f32(1e-3 * rng.standard_normal((S, B, 3 * N)))

    def run(device, ps):
        t = lambda a, grad=False: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(device).requires_grad_(grad)
        tx, ta, tm, tv = t(x0, True), t(actions, True), t(mu0, True), t(pv0, True)
        xs, vs = sim_rollout(sim, tx, t(np.zeros_like(x0)), ta, mu=tm, primitive_velocities=tv, primitive_shapes=None if ps is None else t(ps))
        (xs * t(w)).sum().backward()
        shapes = np.stack([e.get_primitive_shapes(s + 1) for s in range(S)])
        return (xs.detach().cpu().numpy(), vs.detach().cpu().numpy(), shapes) + tuple(g.grad.cpu().numpy() for g in (tx, ta, tm, tv))

    host, devc = run("cpu", SH), run("cuda", SH)
    for k in range(3):
        np.testing.assert_array_equal(devc[k], host[k])
    np.testing.assert_array_equal(host[2], f32(SH))
    for k, name in ((3, "x0"), (4, "actions"), (5, "mu"), (6, "primitive_velocities")):
        assert rel(devc[k], host[k]) <= 2e-6, name
        assert np.abs(host[k]).max() > 0, name
    assert host[5][2, 0] == 0                                                # rollout 2's sphere (radius 0.5) touches nothing: no friction gradient
    # per-step engine calls
    e.clear_schedules()
    e.set_state(0, x0, np.zeros_like(x0))
    e.set_primitive_velocities(pv0[0])
    for s in range(S):
        e.set_primitive_shapes(SH[s])
        e.step_forward(s, fixed_pts=actions[s])
    xs, vs = e.get_states(1, S)
    np.testing.assert_array_equal(xs.astype(np.float32), devc[0]); np.testing.assert_array_equal(vs.astype(np.float32), devc[1])
    e.set_primitive_shapes(None)
    # constant over the episode, and omitted: the schedule is cleared like the others
    const_h, const_d = run("cpu", SH[0]), run("cuda", SH[0])
    np.testing.assert_array_equal(const_d[0], const_h[0])
    np.testing.assert_array_equal(const_d[2], np.broadcast_to(f32(SH[0]), (S, B, 1, 8)))
    none_d = run("cuda", None)
    np.testing.assert_array_equal(none_d[2], built)
    assert np.abs(none_d[0] - const_d[0]).max() > 1e-6 and np.abs(const_d[0] - devc[0]).max() > 1e-6
    with pytest.raises(ValueError, match="does not see an obstacle's shape"):
        sim_rollout(sim, torch.zeros(B, 3 * N), torch.zeros(B, 3 * N), None, steps=S, primitive_shapes=torch.zeros(B, 1, 8, requires_grad=True))
    e.close()
