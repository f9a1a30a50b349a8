"""Scenes of tests/test_gpu_contact_readout_grad.py: the scenes of tests/contact_readout_scenes.py once more, with the oracles KEPT (the
read-out's adjoint model differentiates their records: adjoint_matrix, step_backward) and with calcSeparateAtp on (dL/dk), plus random
weights and a random state loss per step and rollout. The steps are the same teacher-forced steps from the same fp32 states, so record s of
oracle b is the record contact_readout_scenes holds. Helpers, not tests; computed once per process on the CPU."""
import functools

import numpy as np

import contact_readout_scenes as cs
import orc
import readout_grad_model as model
import records
from diffcloth_amd import capi

H, f32 = cs.H, cs.f32


def clipped_scene():
    """the static scene with two vertices under the crown clipped to targets that follow their free fall (the static scene's own trajectory,
    pressed 0.03 into the sphere): both are in primitive contact, so the attachment terms of the read-out's adjoint — h k_att q on dL_dxfixed, the k_att sum
    of dL/dk, h^2 k_att q in the seed's operator — are as large as the others"""
    free = cs.scene("static")
    att = (143, 145)          # row 8, columns 7 and 9 of the 17 x 17 grid: next to the centre vertex, on the sphere's crown
    steps, nb = 2, 2
    V, F, c = cs.grid()
    X0, V0 = cs.landing(V, nb)
    ids = (3 * np.asarray(att)[:, None] + np.arange(3)).reshape(-1)
    XF = np.stack([np.stack([f32(free.ref[s][b]["x"][ids] + np.tile([0.0, -0.03, 0.0], len(att))) for b in range(nb)]) for s in range(steps)])
    return cs.Scene(V, F, [cs.sphere(c)], X0, V0, steps=steps, D=np.tile(cs.D3[:nb], (steps, 1, 1, 1)), att=att, XF=XF)


class GradScene:
    def __init__(self, name):
        self.name = name
        self.sc = sc = clipped_scene() if name == "clipped" else cs.scene(name)
        N, nb, G, steps = sc.N, sc.nb, sc.G, sc.steps
        self.oracles, self.rid = [], [[None] * nb for _ in range(steps)]
        for b in range(nb):
            o = orc.Oracle(sc.V, sc.F, h=H, fwd_tol=1e-9, bwd_tol=1e-9, selfcollision=bool(sc.selfcollision), contact=True, gradient_clipping=False,
                           attachments=list(sc.att), calc_atp=True, **sc.fabric)
            o.build()
            wt = np.tile(sc.W[b, 0], N)
            for s in range(steps):
                orc.lib().orc_clear_primitives(o.h)
                o.nprim = 0
                for g in range(G):
                    cs.add_to_oracle(o, [p for p in sc.prims if p["group"] == g], sc.D[s, b, g], sc.mu[b, g])
                r = o.step(sc.Xe[s, b], sc.Ve[s, b] - wt, None if sc.XF is None else sc.XF[s, b])
                assert np.array_equal(r["x"], sc.ref[s][b]["x"])          # the same step as the read-out scenes' oracle took
                self.rid[s][b] = r["id"]
            self.oracles.append(o)
        rng = np.random.default_rng(97)
        self.gx = f32(rng.standard_normal((steps, nb, 3 * N)))
        self.gv = f32(0.01 * rng.standard_normal((steps, nb, 3 * N)))
        self.ix = f32(rng.standard_normal((steps, nb, 3 * N)))
        self.iv = f32(0.01 * rng.standard_normal((steps, nb, 3 * N)))
        # weights on jn, J, tau and sum jn (the counts' entries are set too: they must be ignored); sized so that the read-out's part of every
        # gradient is of the order of the state loss's
        self.wj = f32(rng.standard_normal((steps, nb, N)))
        self.ww = f32(rng.standard_normal((steps, nb, G, 10)))
        self.radius = [next(p["radius"] if p["kind"] == capi.DC_PRIM_SPHERE else 0.0 for p in sc.prims if p["group"] == g) for g in range(G)]

    def primitives_at(self, o, s, b):
        """the oracle reads its primitives when it differentiates (mu, the rotating sphere's flag): those of step s"""
        sc = self.sc
        orc.lib().orc_clear_primitives(o.h)
        o.nprim = 0
        for g in range(sc.G):
            cs.add_to_oracle(o, [p for p in sc.prims if p["group"] == g], sc.D[s, b, g], sc.mu[b, g])

    def centres(self, s, b):
        return np.stack([self.sc.centre(s, b, g) for g in range(self.sc.G)])

    def arm_x(self, s, b, x=None):
        """positions of the torque arm in the engine's frame"""
        sc = self.sc
        x = sc.ref[s][b]["x"] if x is None else x
        return (x + np.tile(sc.W[b, 0], sc.N) * H).reshape(-1, 3)

    def terms(self, s, b, weights=True, state=None, x=None):
        o = self.oracles[b]
        self.primitives_at(o, s, b)
        wj = self.wj[s, b] if weights else np.zeros(self.sc.N)
        ww = self.ww[s, b] if weights else np.zeros((self.sc.G, 10))
        return model.contact_terms(o, self.rid[s][b], self.sc.mu[b], self.arm_x(s, b, x), self.centres(s, b), wj, ww, radius=self.radius, state=state), ww

    def backward(self, s, b, gx, gv, ix=None, iv=None, is_start=False, weights=True, state=None, x=None):
        sc = self.sc
        t, ww = self.terms(s, b, weights, state, x)
        v_prev = sc.Ve[s, b] - np.tile(sc.W[b, 0], sc.N)
        out = model.backward(self.oracles[b], self.rid[s][b], gx, gv, t, ww, ix=ix, iv=iv, is_start=is_start, v_prev=v_prev, att=sc.att,
                             k_att=self.oracles[b].params["k_att"])
        out["terms"] = t
        return out

    def oracle_records(self, s):
        """record s of every rollout as dc_set_record takes it, in the engine's frame (x + w h, v + w, f + m w)"""
        sc = self.sc
        recs = []
        for b in range(sc.nb):
            o = self.oracles[b]
            ref = dict(sc.ref[s][b], id=self.rid[s][b])
            q = records.oracle_record(o, ref)
            wt = np.tile(sc.W[b, 0], sc.N)
            m3 = np.repeat(o.vertex_data()[0], 3)
            q["x"] = q["x"] + wt * H; q["v"] = q["v"] + wt; q["f"] = q["f"] + m3 * wt
            recs.append(q)
        return recs


@functools.lru_cache(maxsize=None)
def scene(name):
    return GradScene(name)
