"""The fp64 model of the contact read-out's adjoint (tests/readout_grad_model.py, the rule of dc_set_contact_readout_gradients) against central
differences of the fp64 oracle with the step's contact set and normals frozen (Oracle.step(frozen=rid)), the way tests/test_oracle_step.py
checks the oracle's own stepBackward — and with its gates: 2e-5 max(|fd|, |model|, 1e-3), 1e-4 for k and density.

The loss is a random linear state loss plus a random linear loss on the read-out of the step, L = cx . x_new + cv . v_new + sum jn^_i jn_i +
sum_g W_g . {J, tau, sum jn}_g. Every scene holds stick and slide contacts, and every difference is taken at two step sizes that must agree: a
contact that changed its case inside the difference would show there. No GPU needed."""
import functools

import numpy as np
import pytest

import meshes
import orc
import readout_grad_model as model

H = 1 / 180
RADIUS = 2.0


@functools.lru_cache(maxsize=None)
def case(nx, mu, att, rotates):
    """a cloth falling on the sphere with a sideways drift, stopped while it still slides at the rim and sticks at the crown"""
    if att == "crown":
        return crown_case(nx, mu)
    V, F = meshes.grid_cloth(nx, nx, 4.5, 4.5, "DOWN")
    o = orc.Oracle(V, F, h=H, density=0.3, k_stretch=150.0, k_bend=0.05, fwd_tol=1e-13, bwd_tol=1e-13, attachments=att, selfcollision=False,
                   pd_iter_cap=20000, calc_atp=True)
    c = meshes.sphere_scene_center(V, RADIUS)
    o.add_sphere(c, RADIUS, mu, rotates=rotates)
    o.build()
    xf = V.reshape(-1, 3)[list(att)].reshape(-1) + 0.02 if len(att) else None
    x = V.reshape(-1).copy()
    # (at mu 0.05 only a vertex that meets the crown head-on sticks: no drift there, and one such contact is what there is)
    v = np.tile([0.4, -1.0, 0.25] if mu > 0.1 else [0.0, -1.0, 0.0], V.shape[0])
    need = 2 if mu > 0.1 and not rotates else 1       # (the rotating sphere's surface runs at 8: one contact at the pole sticks, at mu 0.9)
    for s in range(400):
        out = o.step(x, v, xf, t_prev=s * H)
        ty = o.prim_contacts(out["id"])["type"]
        if np.sum(ty == 1) >= need and np.sum(ty == 2) >= need:
            break
        x, v = out["x"], out["v"]
    else:
        raise AssertionError(f"no state with stick and slide contacts (nx {nx}, mu {mu})")
    return V, F, o, np.asarray(c, dtype=np.float64), x, v, xf


def crown_case(nx, mu):
    """the centre vertex clipped to a target that follows its free fall, pressed 0.03 into the sphere: an attached vertex IN contact, so that the
    attachment terms of the rule (h k_att q on dL_dxfixed, the k_att sum, h^2 k_att q in the seed's operator) carry weight"""
    V, F, free, c, x0, v0, _ = case(nx, mu, (), False)
    a = (nx // 2) * nx + nx // 2
    o = orc.Oracle(V, F, h=H, density=0.3, k_stretch=150.0, k_bend=0.05, fwd_tol=1e-13, bwd_tol=1e-13, attachments=(a,), selfcollision=False,
                   pd_iter_cap=20000, calc_atp=True)
    o.add_sphere(c, RADIUS, mu)
    o.build()
    xf = free.step(x0, v0, None)["x"][3 * a:3 * a + 3] - np.array([0.0, 0.03, 0.0])
    return V, F, o, c, x0, v0, xf


CASES = [(7, 0.05, (), False), (9, 0.4, (), False), (8, 0.9, (), False), (9, 0.4, (0, 8), False), (7, 0.9, (), True), (9, 0.4, "crown", False)]


class Setup:
    def __init__(self, nx, mu, att, rotates):
        self.V, self.F, self.o, self.c, self.x0, self.v0, self.xf = case(nx, mu, att, rotates)
        self.mu, self.att = mu, (((nx // 2) * nx + nx // 2,) if att == "crown" else att)
        att = self.att
        o = self.o
        self.n3 = self.x0.size
        rng = np.random.default_rng(5)
        self.cx, self.cv = rng.standard_normal(self.n3), 0.01 * rng.standard_normal(self.n3)
        self.wj = rng.standard_normal(o.N)
        self.ww = rng.standard_normal((1, 10))
        self.field = None
        o.set_force_extras(None, None, 1.0)
        self.base = o.step(self.x0, self.v0, self.xf)
        self.rid = self.base["id"]

    def loss(self, x=None, v=None, xf=None, mu=None, field=None):
        o = self.o
        mu = self.mu if mu is None else mu
        o.set_mu(0, mu)
        o.set_force_extras(None, field, 1.0)
        out = o.step(self.x0 if x is None else x, self.v0 if v is None else v, self.xf if xf is None else xf, frozen=self.rid)
        o.set_mu(0, self.mu)
        o.set_force_extras(None, None, 1.0)
        assert out["converged"]
        return self.cx @ out["x"] + self.cv @ out["v"] + model.readout_loss(o, out["id"], [mu], out["x"].reshape(-1, 3), self.c[None], self.wj, self.ww)

    def model(self, with_readout=True):
        o = self.o
        ww = self.ww if with_readout else np.zeros_like(self.ww)
        wj = self.wj if with_readout else np.zeros_like(self.wj)
        t = model.contact_terms(o, self.rid, [self.mu], self.base["x"].reshape(-1, 3), self.c[None], wj, ww)
        return t, model.backward(o, self.rid, self.cx + self.cv / H, self.cv, t, ww, is_start=True, v_prev=self.v0, att=self.att, k_att=o.params["k_att"])


def fd(f, eps):
    """central difference at eps and eps / 2; the two must agree (no contact changes its case inside the difference)"""
    a = (f(eps) - f(-eps)) / (2 * eps)
    b = (f(eps / 2) - f(-eps / 2)) / eps
    assert abs(a - b) <= 2e-5 * max(abs(a), abs(b), 1e-3), (a, b)
    return b


@pytest.mark.parametrize("nx,mu,att,rotates", CASES)
def test_state_mu_force_and_fixed_point_gradients(nx, mu, att, rotates):
    S = Setup(nx, mu, att, rotates)
    ty = S.o.prim_contacts(S.rid)["type"]
    assert np.sum(ty == 1) >= 1 and np.sum(ty == 2) >= 1, ty
    t, bw = S.model()
    plain = bw["plain"]
    rng = np.random.default_rng(11)
    lines = []
    miss = 0.0
    for name, grad, pgrad, eps in (("x", bw["dL_dx"], plain["dL_dx"], 1e-6), ("v", bw["dL_dv"], plain["dL_dv"], 1e-6),
                                   ("field", bw["dL_dfext_vec"], plain["dL_dfext_vec"], 1e-5), ("xf", bw["dL_dxfixed"], plain["dL_dxfixed"], 1e-6)):
        if name == "xf" and not len(att):
            continue
        for trial in range(3):
            d = rng.standard_normal(grad.size)
            d /= np.linalg.norm(d)
            if name == "x":
                num = fd(lambda e: S.loss(x=S.x0 + e * d), eps)
            elif name == "v":
                num = fd(lambda e: S.loss(v=S.v0 + e * d), eps)
            elif name == "field":
                num = fd(lambda e: S.loss(field=e * d), eps)
            else:
                num = fd(lambda e: S.loss(xf=S.xf + e * d), eps)
            an, un = grad @ d, pgrad @ d
            lines.append(f"{name} trial {trial}: fd {num:+.6e} model {an:+.6e} without the read-out's part {un:+.6e}")
            assert abs(num - an) <= 2e-5 * max(abs(num), abs(an), 1e-3), lines[-1]
            miss = max(miss, abs(num - un) / max(abs(num), 1e-3))
    num = fd(lambda e: S.loss(mu=mu + e), 1e-6)
    lines.append(f"mu: fd {num:+.6e} model {bw['dL_dmu'][0]:+.6e} without the read-out's part {plain['dL_dmu'][0]:+.6e}")
    print("\n" + "\n".join(lines))
    assert abs(num - bw["dL_dmu"][0]) <= 2e-5 * max(abs(num), abs(bw["dL_dmu"][0]), 1e-3), lines[-1]
    assert miss > 1e-2, f"the read-out's part is invisible in this scene (largest miss of the plain adjoint {miss:.2e})"


@pytest.mark.parametrize("nx,mu,att,rotates", [CASES[1], CASES[3], CASES[5]])
def test_stiffness_and_density_gradients(nx, mu, att, rotates):
    S = Setup(nx, mu, att, rotates)
    att = S.att
    o = S.o
    t, bw = S.model()
    lines = []
    try:
        for key, gi, eps in (("k_stretch", 0, 1e-4), ("k_bend", 1, 1e-6), ("density", None, 1e-7)) + ((("k_att", 2, 1e-2),) if len(att) else ()):
            base = o.params[key]

            def at(e):
                o.set(**{key: base + e}); o.build()
                return S.loss()
            num = (at(eps) - at(-eps)) / (2 * eps)
            num2 = (at(eps / 2) - at(-eps / 2)) / eps
            o.set(**{key: base}); o.build()
            an = bw["dL_dk"][gi] if gi is not None else bw["dL_ddensity"]
            un = bw["plain"]["dL_dk"][gi] if gi is not None else bw["plain"]["dL_ddensity"]
            lines.append(f"{key}: fd {num2:+.6e} (at twice the step {num:+.6e}) model {an:+.6e} without the read-out's part {un:+.6e}")
            assert abs(num - num2) <= 1e-4 * max(abs(num), 1e-3), lines[-1]
            assert abs(num2 - an) <= 1e-4 * max(abs(num2), 1e-3), lines[-1]
    finally:
        print("\n" + "\n".join(lines))
