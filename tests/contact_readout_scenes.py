"""Scenes of the contact read-out tests (tests/test_contact_readout_host.py, tests/test_gpu_contact_readout.py): the fp64 oracle's
teacher-forced trajectories, computed once per process on the CPU, with everything the read-out is compared against — helpers, not tests.

A scene is a mesh, a list of engine primitives (group ids 0 .. G-1; several primitives of one group are the children of ONE LowerLeg), per
rollout a friction coefficient per group, a frame velocity w (the engine steps (x, v + w) under obstacles moving at w, the oracle the static
step at (x, v): tests/test_gpu_primitive_velocities.py) and per step and rollout an offset of every group's centre. The oracle's primitives
are cleared and re-added at the step's centre before every step (it reads them per step), so an offset schedule needs no rebuild.

What the oracle says about a contact: prim_contacts(rid) gives particle, prim (= group), type (CollisionType: 0 take-off, 1 stick, 2 slide),
normal, d and r. The public state is type + 1.

MARGINS. A contact whose d lies on a boundary of the friction law may be decided the other way by a record that is not the oracle's bit
for bit. How far a record may be off depends on where it comes from, and so does the margin a decision must keep — the smaller of
|sd| / |d| and, in contact, ||dT| - mu |sd|| / |d| (decision_margin) — to be compared:
  * the ORACLE's record handed in with dc_set_record: f, n, the masses and the motion row are rounded to fp32 once and d and the two
    comparisons take some ten fp32 operations, so d is off by at most GATE_F32 = 1e-6 |d| (16 ulp). MARGIN_RECORD = 100 x GATE_F32. Contacts
    inside it are left out of the state comparison; their share of a scene's contacts is at most MAX_UNSAFE_SHARE, asserted on the oracle alone.
  * the ENGINE's own record of the same step: its PD iterate is not the oracle's. The gates on such a record are those of
    tests/test_gpu_parity.py, |f - f_oracle| <= 1e-3 |f_oracle| (GATE_F) and |r - r_oracle| <= 2e-3 |r_oracle| (GATE_R); MARGIN_STEP =
    100 x GATE_F = 0.1. A cloth on a sphere has contacts at every distance from the friction cone, and a third of them lie inside a band that
    wide (measured on the oracle alone: 36 % ... 47 % on these scenes), so no share is bounded here: the state of an own record is compared with
    the oracle's type outside MARGIN_STEP, and at EVERY contact outside MARGIN_RECORD with the rule evaluated in fp64 on the engine's own
    record (classify), which no difference between two PD iterates touches.
"""
import functools

import numpy as np

import meshes
import orc
import test_gpu_primitive_offsets as po
from diffcloth_amd import capi, workloads

H = po.H
FABRIC = po.FABRIC
f32 = po.f32
GATE_F, GATE_R = 1e-3, 2e-3
SUM_RTOL = 1e-4                 # sums: |diff| <= 1e-4 x the sum of the terms' magnitudes, the rule of dL/dw (tests/test_gpu_primitive_velocities.py)
GATE_F32 = 1e-6
MARGIN_STEP = 100 * GATE_F
MARGIN_RECORD = 100 * GATE_F32
MAX_UNSAFE_SHARE = 0.02
SURFACE_SPEED = 8.0             # the reference's rotating sphere: v_rot = 8 (y^ x n)
FALL = np.array([0.0, -6.0, 0.0])


def add_to_oracle(o, group_prims, centre_shift, mu):
    """one oracle primitive for one engine group, its centre moved by centre_shift"""
    p = group_prims[0]
    c = f32(np.asarray(p["center"], dtype=np.float64) + centre_shift)
    if len(group_prims) > 1:            # LowerLeg: children relative to the collection's centre = the first child's parent centre
        raise NotImplementedError
    k = p["kind"]
    if k == capi.DC_PRIM_SPHERE:
        o.add_sphere(c, p["radius"], mu, rotates=bool(p.get("oracle_rotates", p.get("rotates", 0))))
    elif k == capi.DC_PRIM_SPHERE_DISCRETIZED:
        o.add_discretized_sphere(c, p["radius"], mu)
    elif k == capi.DC_PRIM_CAPSULE:
        o.add_capsule(c, p["top_offset"], p["radius"], p["length"], mu)
    elif k == capi.DC_PRIM_PLANE:
        o.add_plane(c, p["top_offset"], p["corner2"], mu)
    elif k == capi.DC_PRIM_BOWL:
        o.add_bowl(c, p["radius"], mu)
    else:
        raise KeyError(k)


class Scene:
    def __init__(self, V, F, prims, X0, V0, steps, W=None, D=None, mu=None, selfcollision=False, fabric=FABRIC, leg=None, att=(), XF=None):
        """X0, V0: [nb][3N] start states in the STATIC frame; W: [nb][G][3] (one frame velocity per rollout: row 0 is the cloth's frame);
        D: [steps][nb][G][3] centre offsets; mu: [nb][G]; leg: (centre, mu, children) of the oracle's LowerLeg standing for ALL prims;
        att / XF [steps][nb][3 Af]: attachment vertices and their targets"""
        self.V, self.F, self.prims, self.steps, self.fabric, self.selfcollision = V, F, prims, steps, fabric, selfcollision
        self.N = N = V.shape[0]
        self.nb = nb = X0.shape[0]
        self.G = G = len({p["group"] for p in prims})
        self.W = np.zeros((nb, G, 3)) if W is None else np.asarray(W, dtype=np.float64)
        self.D = np.zeros((steps, nb, G, 3)) if D is None else np.asarray(D, dtype=np.float64)
        self.mu = np.array([[next(p["mu"] for p in prims if p["group"] == g) for g in range(G)]] * nb) if mu is None else np.asarray(mu, dtype=np.float64)
        self.att = tuple(att)
        self.XF = XF
        self.ref = [[None] * nb for _ in range(steps)]
        self.Xe = np.zeros((steps, nb, 3 * N)); self.Ve = np.zeros_like(self.Xe)
        for b in range(nb):
            o = orc.Oracle(V, F, h=H, fwd_tol=1e-9, bwd_tol=1e-9, selfcollision=bool(selfcollision), contact=True, gradient_clipping=False,
                           attachments=list(self.att), **fabric)
            o.build()
            wt = np.tile(self.W[b, 0], N)
            x, ve = f32(X0[b]), f32(V0[b] + wt)
            for s in range(steps):
                orc.lib().orc_clear_primitives(o.h)
                o.nprim = 0
                if leg is not None:
                    o.add_lower_leg(f32(np.asarray(leg[0]) + self.D[s, b, 0]), self.mu[b, 0], [np.concatenate([[k], c0, t, [r, ln]]) for k, c0, t, r, ln in leg[2]])
                else:
                    for g in range(G):
                        add_to_oracle(o, [p for p in prims if p["group"] == g], self.D[s, b, g], self.mu[b, g])
                self.Xe[s, b], self.Ve[s, b] = x, ve
                r = o.step(x, ve - wt, None if XF is None else XF[s, b])
                r["pc"] = o.prim_contacts(r["id"])
                r["f"], r["r"] = o.record_fr(r["id"])
                self.ref[s][b] = r
                x, ve = f32(r["x"]), f32(r["v"] + wt)

    # ---- what the read-out must give, from the oracle alone ----
    def mu_of(self, b, pc):
        return self.mu[b][pc["prim"]]

    def centre(self, s, b, g):
        """the fp32 centre of group g's FIRST flattened primitive in step s"""
        p = next(p for p in self.prims if p["group"] == g)
        return f32(np.asarray(p["center"], dtype=np.float64) + self.D[s, b, g])

    def expected(self, s, b, centre=None):
        """state [N], jn [N], |d| [N] and per group the wrench row with the scales of its sums, all from prim_contacts and the oracle's x_new"""
        r = self.ref[s][b]
        pc = r["pc"]
        N, G = self.N, self.G
        state = np.zeros(N, dtype=np.int32); jn = np.zeros(N); dn = np.zeros(N)
        state[pc["particle"]] = pc["type"] + 1
        jn[pc["particle"]] = np.einsum("kd,kd->k", pc["r"], pc["normal"])
        dn[pc["particle"]] = np.linalg.norm(pc["d"], axis=1)
        x = (r["x"] + np.tile(self.W[b, 0], N) * H).reshape(-1, 3)          # the engine's frame: moved by w h
        rows, scales = np.zeros((G, 10)), np.zeros((G, 2))
        for g in range(G):
            sel = pc["prim"] == g
            rr, arm = pc["r"][sel], x[pc["particle"][sel]] - (self.centre(s, b, g) if centre is None else centre[g])
            rows[g, 0:3] = -rr.sum(axis=0)
            rows[g, 3:6] = -np.cross(arm, rr).sum(axis=0)
            rows[g, 6] = jn[pc["particle"][sel]].sum()
            for t in range(3):
                rows[g, 7 + t] = np.sum(pc["type"][sel] == t)
            scales[g] = np.linalg.norm(rr, axis=1).sum(), (np.linalg.norm(arm, axis=1) * np.linalg.norm(rr, axis=1)).sum()
        return dict(state=state, jn=jn, dnorm=dn, rows=rows, scales=scales, safe_step=self.safe(s, b, MARGIN_STEP), safe_record=self.safe(s, b, MARGIN_RECORD))

    def safe(self, s, b, margin):
        """[N] bool: the oracle's decision at that vertex keeps `margin` from both boundaries (True where there is no contact)"""
        pc = self.ref[s][b]["pc"]
        out = np.ones(self.N, dtype=bool)
        out[pc["particle"]] = decision_margin(pc["normal"], pc["d"], self.mu_of(b, pc)) > margin
        return out

    def census(self, margin=MARGIN_RECORD):
        """over all steps and rollouts: contacts, take-off / stick / slide counts, contacts inside the margin"""
        n = np.zeros(5, dtype=np.int64)
        for s in range(self.steps):
            for b in range(self.nb):
                pc = self.ref[s][b]["pc"]
                n[0] += len(pc["particle"])
                for t in range(3):
                    n[1 + t] += np.sum(pc["type"] == t)
                n[4] += np.sum(~self.safe(s, b, margin))
        return dict(contacts=int(n[0]), takeoff=int(n[1]), stick=int(n[2]), slide=int(n[3]), unsafe=int(n[4]))


def decision_margin(n, d, mu):
    """per contact: the smaller of |sd| / |d| and (in contact) ||dT| - mu |sd|| / |d|"""
    sd = np.einsum("kd,kd->k", d, n)
    dT = d - sd[:, None] * n
    dn = np.maximum(np.linalg.norm(d, axis=1), 1e-300)
    m1 = np.abs(sd) / dn
    m2 = np.abs(np.linalg.norm(dT, axis=1) - mu * np.abs(sd)) / dn
    return np.where(sd >= 0, m1, np.minimum(m1, m2))


def classify(n, d, mu):
    """the friction law's decision as the public state code"""
    sd = np.einsum("kd,kd->k", d, n)
    dT = d - sd[:, None] * n
    return np.where(sd >= 0, 1, np.where(np.linalg.norm(dT, axis=1) <= mu * np.abs(sd), 2, 3)).astype(np.int32)


def sphere(c, group=0, mu=0.4, radius=2.0, **kw):
    return dict(kind=capi.DC_PRIM_SPHERE, group=group, center=c, radius=radius, mu=mu, **kw)


def grid(nx=17):
    V, F = meshes.grid_cloth(nx, nx, 4.5, 4.5, "DOWN")
    V = f32(V)
    return V, F, f32(meshes.sphere_scene_center(V, 2.0))


def landing(V, nb, fall=FALL):
    return np.tile(f32(V.reshape(-1)), (nb, 1)), np.tile(f32(np.tile(fall, V.shape[0])), (nb, 1))


W3 = np.array([[0.0, 0.0, 0.0], [2.0, -1.0, -0.5], [-4.0, 0.0, 2.0]]).reshape(3, 1, 3)          # the velocities of the velocity tests
D3 = np.array([[0.0, 0.125, 0.0], [0.25, 0.1875, 0.125], [0.0, 0.125, 0.0]]).reshape(3, 1, 3)   # ... and their centre offsets


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "static":                 # the landing scene of the spin tests under a sphere at rest
        V, F, c = grid()
        X0, V0 = landing(V, 3)
        return Scene(V, F, [sphere(c)], X0, V0, steps=3, D=np.tile(D3, (3, 1, 1, 1)))
    if name == "moving_spinning":        # the oracle's rotating sphere; the engine: (x, v + w), w, omega = (0, 8 / radius, 0) on a plain sphere
        V, F, c = grid()
        X0, V0 = landing(V, 3)
        return Scene(V, F, [sphere(c, oracle_rotates=1)], X0, V0, steps=2, W=W3, D=np.tile(D3, (2, 1, 1, 1)))
    if name == "mu":                     # the same cloth and sphere at mu 0.05 and 0.8
        V, F, c = grid()
        X0, V0 = landing(V, 2)
        return Scene(V, F, [sphere(c)], X0, V0, steps=2, D=np.tile(D3[:1], (2, 2, 1, 1)), mu=[[0.05], [0.8]])
    if name == "three_groups":           # two spheres side by side under the cloth, a third far below: its row must be zero
        V, F, c = grid()
        X0, V0 = landing(V, 2)
        prims = [sphere(f32(c + np.array([-1.0, 0.125, 0.0])), 0), sphere(f32(c + np.array([0.0, -6.0, 0.0])), 1), sphere(f32(c + np.array([1.0, 0.125, 0.0])), 2, mu=0.2)]
        return Scene(V, F, prims, X0, V0, steps=2)
    if name == "offset_schedule":        # the sphere rises and drifts sideways from step to step: tau is about the MOVED centre
        V, F, c = grid()
        X0, V0 = landing(V, 2)
        D = np.stack([np.array([[[0.25 * s, 0.125 + 0.03125 * s, -0.125 * s]], [[-0.5 * s, 0.125, 0.25 * s]]]) for s in range(3)])
        return Scene(V, F, [sphere(c)], X0, V0, steps=3, D=D)
    if name == "flap":                   # the folded flap lying on the sphere: primitive AND self contacts
        cfg = workloads.C4_CLOTH
        V, F, Vf, flap, c = workloads.c4_scene(grid=16, fold_rows=3, fold_gap=0.02)
        fabric = dict(density=cfg["density"], k_stretch=cfg["k_stretch"], k_bend=cfg["k_bend"])
        to_flap = Vf[flap].mean(axis=0) - c
        cm = f32(c + np.round(np.array([to_flap[0], 0.0, to_flap[2]]) * 32) / 32 + np.array([0.0, 0.125, 0.0]))
        X0 = f32(Vf.reshape(1, -1))
        V0 = np.zeros_like(V)
        V0[flap, 1] = -3.0               # the flap coming down on the cloth: at rest the layers leave r unchanged at the vertices that stick to the sphere
        return Scene(V, F, [sphere(cm, mu=cfg["sphere_mu"], radius=cfg["sphere_radius"])], X0, f32(V0.reshape(1, -1)), steps=3, selfcollision=True, fabric=fabric)
    if name == "split":                  # the 29 x 29 grid the split kernels take (DC_CLUSTER = 2, 4)
        V, F, c = grid(29)
        X0, V0 = landing(V, 2)
        return Scene(V, F, [sphere(c)], X0, V0, steps=2, D=np.tile(D3[:2], (2, 1, 1, 1)))
    if name == "plane":                  # the tilted rectangle of tests/test_gpu_primitive_offsets.py
        V, F = meshes.grid_cloth(22, 22, 4.5, 4.5, "DOWN")
        V = f32(V)
        c = f32(V.mean(axis=0) + np.array([0.13, -0.25, 0.07]))
        p = dict(kind=capi.DC_PRIM_PLANE, group=0, center=c, top_offset=f32([-1.5, 0.3, -1.5]), corner2=f32([1.5, 0.3, -1.5]), radius=0.0, mu=0.2)
        X0, V0 = landing(V, 1, fall=np.array([0.5, -3.0, 0.0]))
        return Scene(V, F, [p], X0, V0, steps=2)
    if name == "capsule":                # a lying capsule under the landing cloth
        V, F, c = grid()
        p = dict(kind=capi.DC_PRIM_CAPSULE, group=0, center=f32(c + np.array([-1.5, 1.0, 0.0])), top_offset=f32([3.0, 0.0, 0.0]), radius=1.0, length=3.0, mu=0.3)
        X0, V0 = landing(V, 1)
        return Scene(V, F, [p], X0, V0, steps=2)
    if name == "bowl":                   # the sheet laid on the shell across its equator, moving outwards (tests/test_gpu_primitive_offsets.py)
        V, F = meshes.grid_cloth(14, 14, 1.3, 1.3, "DOWN")
        V = f32(V)
        R = 1.2
        c = f32(np.array([V[:, 0].mean(), 0.0, V[:, 2].mean()]) + np.array([0.125, 0.25, 0.0]))
        u, w = (V[:, 0] - V[:, 0].mean()) / R, (V[:, 2] - V[:, 2].mean()) / R
        unit = np.stack([np.cos(u) * np.cos(w), np.sin(u), np.cos(u) * np.sin(w)], axis=1)
        X0 = f32((c + R * unit).reshape(1, -1))
        V0 = f32((0.3 * unit + np.array([0.0, 0.0, 0.2])).reshape(1, -1))
        return Scene(V, F, [dict(kind=capi.DC_PRIM_BOWL, group=0, center=c, radius=R, mu=0.4)], X0, V0, steps=1)
    if name == "discretised_sphere":     # the BIG_SPHERE of tests/test_gpu_primitive_offsets.py: face normals, not radial ones
        V, F = meshes.grid_cloth(22, 22, 4.5, 4.5, "DOWN")
        V = f32(V)
        R = 15.0
        c = np.array([-0.125, -15.75, -0.125])
        X = V.copy()
        X[:, 0] += c[0] - V[:, 0].mean() + 0.37; X[:, 2] += c[2] - V[:, 2].mean() - 0.21
        X[:, 1] = c[1] + np.sqrt(R * R - (X[:, 0] - c[0]) ** 2 - (X[:, 2] - c[2]) ** 2) + 0.02
        vel = np.zeros_like(V); vel[:, 1] = -0.3; vel[:, 0] = 0.2
        return Scene(V, F, [dict(kind=capi.DC_PRIM_SPHERE_DISCRETIZED, group=0, center=c, radius=R, mu=0.3)], f32(X.reshape(1, -1)), f32(vel.reshape(1, -1)), steps=1)
    if name == "lower_leg":              # the LowerLeg of tests/test_gpu_primitive_offsets.py threaded through a sheet: ONE group, torque about its first child
        V, F = meshes.grid_cloth(12, 12, 4.5, 4.5, "DOWN")
        V = f32(V)
        center, children = workloads.sock_leg(V.min(axis=0), V.max(axis=0))
        center = f32(center)
        children = [(k, f32(c0), f32(t), float(np.float32(r)), float(np.float32(ln))) for k, c0, t, r, ln in children]
        prims = [dict(kind=capi.DC_PRIM_SPHERE if k == 0 else capi.DC_PRIM_CAPSULE, group=0, center=center + c0, radius=r, mu=0.4, top_offset=t, length=ln)
                 for k, c0, t, r, ln in children]
        mid = V.mean(axis=0)
        X0 = np.stack([f32((V + (center + np.array([0.0, height, 0.0]) - mid)).reshape(-1)) for height in (2.0, 4.1)])
        V0 = np.tile(f32(np.tile([0.3, -0.5, 0.0], V.shape[0])), (2, 1))
        return Scene(V, F, prims, X0, V0, steps=1, leg=(center, 0.4, children))
    raise KeyError(name)


# scenes whose states are compared against the oracle's types: each holds take-off, stick and slide contacts (the landing cloth rebounds)
STATE_SCENES = ("static", "moving_spinning", "mu", "three_groups", "offset_schedule", "split")
