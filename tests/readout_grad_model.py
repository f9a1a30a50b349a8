"""fp64 numpy model of the contact read-out's adjoint (dc_set_contact_readout_gradients; include/diffcloth_hip.h states the rule) — a helper of
tests/test_readout_grad_model.py (which checks it against central differences of the oracle) and tests/test_gpu_contact_readout_grad.py (which
checks the engine against it), not a test.

Everything is built from pieces the oracle exposes: prim_contacts (particle, group, normal, d), orc.friction (r, the case, J = dr/dd, dr/dmu),
adjoint_matrix, vertex_data and step_backward with a given u, as step_backward_lu does. The contact-free operator h^2 (A - dp/dx)^T A is the
adjoint matrix of the SAME record with the oracle's contact switch off (K = P - dP^T then has no dr_df part), minus the mass matrix; the oracle
reads that switch when it differentiates, so no second oracle and no copied record are needed.

With the weights jn^ [N] and W [G][10] (J^ = W[g][0:3], tau^ = W[g][3:6], S^ = W[g][6]; 7..9 unread) of ONE record:
    Phi   = sum_i jn^_i jn_i + sum_g W[g][0:7] . row_g            (the read-out loss of that record)
    phi_i = -J^ - tau^ x (x_i - c_g) + (jn^_i + S^) n_i           q_i = J_i^T phi_i
"""
import numpy as np

import orc


def readout_values(o, rid, mu, x, centres):
    """jn [N] and rows [G][7] = {J, tau, sum jn} of record rid as dc_get_contact_readout defines them, from the oracle's contacts with the
    friction law re-evaluated at mu[g]; x [N][3] the positions of the torque arm, centres [G][3]"""
    pc = o.prim_contacts(rid)
    G = len(centres)
    jn, rows = np.zeros(o.N), np.zeros((G, 7))
    for k in range(len(pc["particle"])):
        i, g = int(pc["particle"][k]), int(pc["prim"][k])
        if g < 0:
            continue
        n = pc["normal"][k]
        r = orc.friction(n, pc["d"][k], mu[g])[0]
        jn[i] = r @ n
        rows[g, 0:3] -= r
        rows[g, 3:6] -= np.cross(x[i] - centres[g], r)
        rows[g, 6] += jn[i]
    return jn, rows


def readout_loss(o, rid, mu, x, centres, wj, ww):
    jn, rows = readout_values(o, rid, mu, x, centres)
    return float(wj @ jn + np.sum(ww[:, 0:7] * rows))


def friction_case(n, d, mu, st):
    """r, J = dr/dd and dr/dmu of the friction law in the GIVEN case (1 take-off, 2 stick, 3 slide): what orc.friction returns where it
    decides that case itself (Simulation.cpp:865-919)"""
    if st == 1:
        return np.zeros(3), np.zeros((3, 3)), np.zeros(3)
    if st == 2:
        return -d, -np.eye(3), np.zeros(3)
    sd = d @ n
    dT = d - sd * n
    nT = np.linalg.norm(dT)
    a = dT / nT
    Pn = np.eye(3) - np.outer(n, n)
    J = -np.outer(n, n) + mu * ((sd / nT) * Pn @ (np.eye(3) - np.outer(a, a)) @ Pn + np.outer(a, n))      # (dri_dfi_T_d, transposed back)
    return -sd * n - dT * (mu * abs(sd) / nT), J, dT * (-abs(sd) / nT)


def contact_terms(o, rid, mu, x, centres, wj, ww, radius=None, state=None):
    """phi, q, r_p [N][3], sum (dr/dmu) . phi per group [G], group per vertex [N] (-1: none), the case per vertex (0 none, 1 take-off, 2 stick,
    3 slide) and {-sum m q, -sum m radius (n x q)} per group [G][6] (radius[g] None / 0: no spin term). state [N]: the case the engine
    reports; where it differs from the oracle's own decision (a contact on a boundary of the law) the terms take the engine's."""
    pc = o.prim_contacts(rid)
    N, G = o.N, len(centres)
    m = o.vertex_data()[0]
    phi, q, r = np.zeros((N, 3)), np.zeros((N, 3)), np.zeros((N, 3))
    dmu, grp, case, motion = np.zeros(G), -np.ones(N, dtype=np.int32), np.zeros(N, dtype=np.int32), np.zeros((G, 6))
    own = np.zeros(N, dtype=np.int32)          # the oracle's own decision, before a reported case replaces it
    for k in range(len(pc["particle"])):
        i, g = int(pc["particle"][k]), int(pc["prim"][k])
        if g < 0:
            continue
        n = pc["normal"][k]
        rr, ty, J, dm = orc.friction(n, pc["d"][k], mu[g])
        own[i] = ty + 1
        if state is not None and state[i] != ty + 1:
            ty = int(state[i]) - 1
            rr, J, dm = friction_case(n, pc["d"][k], mu[g], ty + 1)
        grp[i], case[i] = g, ty + 1
        phi[i] = -ww[g, 0:3] - np.cross(ww[g, 3:6], x[i] - centres[g]) + (wj[i] + ww[g, 6]) * n
        if ty == 0:
            phi[i] = 0.0          # a take-off contact contributes nothing (r_p = 0 and dr/dd = 0)
        q[i] = J.T @ phi[i]
        r[i] = rr
        dmu[g] += dm @ phi[i]
        motion[g, 0:3] -= m[i] * q[i]
        if radius is not None and radius[g]:
            motion[g, 3:6] -= m[i] * radius[g] * np.cross(n, q[i])
    return dict(phi=phi, q=q, r=r, dmu=dmu, grp=grp, case=case, own_case=own, motion=motion)


def _contact_off(o):
    class _Off:
        def __enter__(self):
            self.saved = o.flags["contact"]
            o.flags["contact"] = 0
            o._push_params()

        def __exit__(self, *a):
            o.flags["contact"] = self.saved
            o._push_params()
    return _Off()


def seeds(o, rid, terms, ww):
    """items 1 and 2: (the addition to the loss gradient w.r.t. x at the record's slot, the addition to dL/dv at the slot before), 3N each"""
    h = o.params["h"]
    m3 = np.repeat(o.vertex_data()[0], 3)
    q = terms["q"].reshape(-1)
    with _contact_off(o):
        Knc = o.adjoint_matrix(rid)
    g1 = -(Knc @ q - m3 * q) / h
    tau = np.where(terms["grp"][:, None] >= 0, ww[np.maximum(terms["grp"], 0), 3:6], 0.0)
    g1 = g1 - np.cross(terms["r"], tau).reshape(-1)
    return g1, m3 * q


def backward(o, rid, gx, gv, terms, ww, ix=None, iv=None, is_start=False, v_prev=None, att=(), k_att=None):
    """The backward step through record rid with the read-out's part: the dict of Oracle.step_backward_lu (gx, gv, ix, iv in its
    conventions: gx = the carried gradient) with every entry including items 1..4, plus dw [G][6] = the read-out's part of {dL/dw, dL/domega}
    and plain = the same step without weights."""
    h = o.params["h"]
    n3 = 3 * o.N
    z = np.zeros(n3)
    g1, dv1 = seeds(o, rid, terms, ww)
    ix = z if ix is None else np.asarray(ix, dtype=np.float64)
    iv = z if iv is None else np.asarray(iv, dtype=np.float64)
    plain = o.step_backward_lu(rid, gx, gv, dL_dxinit=ix, dL_dvinit=iv, is_start=is_start)
    out = o.step_backward_lu(rid, np.asarray(gx) + g1, gv, dL_dxinit=ix, dL_dvinit=iv + dv1, is_start=is_start)
    q = terms["q"].reshape(-1)
    # items 3 and 4 on what the oracle leaves
    out["dL_dfext_vec"] = out["dL_dfext_vec"] + h * q
    out["dL_dmu"] = out["dL_dmu"] + terms["dmu"][:len(out["dL_dmu"])]
    if len(att):
        out["dL_dxfixed"] = out["dL_dxfixed"] + h * k_att * terms["q"][list(att)].reshape(-1)
    # dL/dk: the oracle's own sum is t2 y . (Atp - L x) per type; with the contact switch off and u = q / h given, y = u = q / h
    with _contact_off(o):
        uu = orc.f64(q / h)
        o.L.orc_set_given_u(o.h, orc._d(uu))
        try:
            extra = o.step_backward(rid, z, z, direct=True)
        finally:
            o.L.orc_set_given_u(o.h, None)
    out["dL_dk"] = out["dL_dk"] + extra["dL_dk"]
    if v_prev is not None:      # the w = y - u term of dL_ddensity: h (q / h) . area (v_prev + h g)
        area = np.repeat(o.vertex_data()[1], 3)
        grav = np.tile(np.asarray(o.params["gravity"], dtype=np.float64) * o.flags["gravity"], o.N)
        out["dL_ddensity"] = out["dL_ddensity"] + float(q @ (area * (np.asarray(v_prev) + h * grav)))
    out["dw"] = terms["motion"]
    out["plain"] = plain
    return out


def motion_gradients(o, rid, gx, gv, terms, ww, radius):
    """{dL/dw, dL/domega} [G][6] of the seeded step, and the sum of the terms' magnitudes [G][2]: -h m_i J_i^T (u_i + phi_i / h) summed per
    group, the part in u read off the is_start outputs as tests/test_gpu_primitive_velocities.py does (c_i = h dL_dx_i + g_v,i - dL_dv_i)"""
    h = o.params["h"]
    g1, dv1 = seeds(o, rid, terms, ww)
    out = o.step_backward_lu(rid, np.asarray(gx) + g1, gv, is_start=True)
    m = o.vertex_data()[0]
    c = (h * out["dL_dx"] + np.asarray(gv) - out["dL_dv"]).reshape(-1, 3) - m[:, None] * terms["q"]
    pc = o.prim_contacts(rid)
    nrm = np.zeros((o.N, 3))
    nrm[pc["particle"]] = pc["normal"]
    G = terms["motion"].shape[0]
    rows, scale = np.zeros((G, 6)), np.zeros((G, 2))
    for g in range(G):
        ids = np.nonzero(terms["grp"] == g)[0]
        rows[g, 0:3] = c[ids].sum(axis=0)
        scale[g, 0] = np.linalg.norm(c[ids], axis=1).sum()
        if radius[g]:
            rows[g, 3:6] = radius[g] * np.cross(nrm[ids], c[ids]).sum(axis=0)
            scale[g, 1] = radius[g] * np.linalg.norm(c[ids], axis=1).sum()
    return rows, scale
