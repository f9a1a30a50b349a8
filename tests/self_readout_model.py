"""The self-contact read-out's rule (dc_get_self_contact_readout, include/diffcloth_hip.h) as plain numpy — a helper, not a test.

walk() is steps 1-3 of the rule: g = f + r_p at the start, the layers in record order, per pair k = (A, B)
    d_k = g_A / m_A - g_B / m_B,   r_k = r(n_k, d_k, 0.1) / (1/m_A + 1/m_B),   g_A += r_k,   g_B -= r_k,   r_self,i = sum of +-r_k.
In fp64 the friction law is the oracle's (orc.friction); in fp32 (`replay`) it is dry_friction / contact_state of csrc/dc_devlib.h restated
operation by operation on np.float32 scalars, without the fused multiply-adds a compiler may form. tests/test_self_readout_model.py holds
the fp64 walk to the oracle's SelfContact::d, its types and Record::r, and measures how far the fp32 replay of the SAME record (rounded to fp32
once) strays from it.

GATE. The worst deviation of the replay's d_k and r_k from the fp64 walk over the eight cases of CASES, relative to
s_k = |g_A| / m_A + |g_B| / m_B (for r_k: to k s_k, k the reduced mass), measured by tests/test_self_readout_model.py:
    worst 8.20e-07 (with_sphere, d), at most 2.4e-07 on the other seven, no growth with the number of layers (1.4e-07 at the 524 of stack4_29)
GATE = 4 x that worst value, rounded up to two digits: another kernel's FMA contraction and reciprocals differ by a few ulps per operation.
The CPU test asserts 4 x its own measurement <= GATE <= 1e-5 and that GATE is no looser than 1.25 x (4 x its measurement); the GPU tests
(tests/test_gpu_self_contact_readout.py) compare the kernel's outputs with the fp64 walk within GATE.
"""
import functools

import numpy as np

CLOTH_MU = 0.1                 # kClothMu (csrc/dc_devlib.h), clothFrictionalCoeff of the reference
GATE = 3.3e-6
MARGIN_RECORD = 1e-4           # tests/contact_readout_scenes.py: a decision this far from both boundaries is compared
MAX_UNSAFE_SHARE = 0.02
SUM_RTOL = 1e-4
CASES = ("cloud_hubs", "cloud_hubs_b", "cloud_hubs_c", "with_sphere", "stack3", "stack4_sphere", "stack4_29", "zigzag40")


def friction64(n, d, mu):
    """(r, state) of the oracle's friction law; state = CollisionType + 1"""
    import orc
    r, ty, _, _ = orc.friction(n, d, mu)
    return r, ty + 1


def _dot32(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def friction32(n, d, mu):
    """dry_friction and contact_state of dc_devlib.h on float32 values"""
    z = np.zeros(3, dtype=np.float32)
    mu = np.float32(mu)
    sd = _dot32(d, n)
    if sd >= 0:
        return z, 1
    dN = n * sd
    dT = d - dN
    nT = np.sqrt(_dot32(dT, dT))
    r = z - dN
    if nT <= mu * np.abs(sd):
        return r - dT, 2
    return r - dT * (mu * np.abs(sd) / nT), 3


def prim_part(f, particles, normals, mu, dt=np.float64):
    """r_p [N][3] under STATIC primitives (d = f): the friction law at the vertices in primitive contact, 0 elsewhere"""
    f = np.asarray(f, dtype=dt).reshape(-1, 3)
    law = friction64 if dt == np.float64 else friction32
    rp = np.zeros_like(f)
    for i, n, m in zip(particles, np.asarray(normals, dtype=dt).reshape(-1, 3), np.broadcast_to(mu, len(particles))):
        rp[i] = law(n, f[i], m)[0]
    return rp


def walk(f, mass, pairs, layer, normal, rp=None, replay=False, reverse_layers=False):
    """Steps 1-3 on one rollout's record. f [N][3] or [3N], mass [N], pairs [C][2], layer [C], normal [C][3] in any order (the walk sorts
    by layer, stably), rp [N][3] or None (no primitive part). replay: every operation in float32 on the inputs rounded to float32.
    Returns per contact, IN THE ORDER GIVEN: d, r, state, s (the scale |g_A| / m_A + |g_B| / m_B), k (the reduced mass), jn = r . n, rt = |r - jn n|, o (the scale of
    the OPERANDS of g = f + r: (|f_A| + |r_A|) / m_A + (|f_B| + |r_B|) / m_B, see degenerate()); and r_self [N][3], accumulated in float64."""
    dt = np.float32 if replay else np.float64
    law = friction32 if replay else friction64
    f = np.asarray(f, dtype=dt).reshape(-1, 3)
    m = np.asarray(mass, dtype=dt)
    nrm = np.asarray(normal, dtype=dt).reshape(-1, 3)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    layer = np.asarray(layer, dtype=np.int64).reshape(-1)
    C = len(layer)
    r = np.zeros_like(f) if rp is None else np.array(rp, dtype=dt).reshape(-1, 3)
    one = dt(1)
    key = -layer if reverse_layers else layer
    out = dict(d=np.zeros((C, 3)), r=np.zeros((C, 3)), state=np.zeros(C, dtype=np.int32), s=np.zeros(C), k=np.zeros(C), jn=np.zeros(C), rt=np.zeros(C), o=np.zeros(C),
               r_self=np.zeros((len(m), 3)))
    for c in np.argsort(key, kind="stable"):
        a, b = pairs[c]
        iA, iB = one / m[a], one / m[b]
        gA, gB = f[a] + r[a], f[b] + r[b]
        d = gA * iA - gB * iB
        rk, st = law(nrm[c], d, CLOTH_MU)
        k = one / (iA + iB)
        rk = np.asarray(rk, dtype=dt) * k
        r[a] = r[a] + rk
        r[b] = r[b] - rk
        rk64 = rk.astype(np.float64)
        out["d"][c], out["r"][c], out["state"][c], out["k"][c] = d, rk64, st, k
        out["s"][c] = np.linalg.norm(gA.astype(np.float64)) * float(iA) + np.linalg.norm(gB.astype(np.float64)) * float(iB)
        out["o"][c] = (np.linalg.norm(f[a]) + np.linalg.norm(gA - f[a])) * float(iA) + (np.linalg.norm(f[b]) + np.linalg.norm(gB - f[b])) * float(iB)
        n64 = nrm[c].astype(np.float64)
        out["jn"][c] = rk64 @ n64
        out["rt"][c] = np.linalg.norm(rk64 - out["jn"][c] * n64)
        out["r_self"][a] += rk64
        out["r_self"][b] -= rk64
    return out


def decision_margin(n, d, s):
    """per contact min(|d.n|, ||d_T| - 0.1 |d.n||) / s: how far the friction law's decision is from its two boundaries"""
    n, d = np.asarray(n, dtype=np.float64).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3)
    sd = np.einsum("kd,kd->k", d, n)
    dT = d - sd[:, None] * n
    return np.minimum(np.abs(sd), np.abs(np.linalg.norm(dT, axis=1) - CLOTH_MU * np.abs(sd))) / np.maximum(s, 1e-300)


GATE_F32 = 1e-6                # tests/contact_readout_scenes.py: what one rounding of a record to fp32 and some ten fp32 operations move d by


def degenerate(w):
    """per contact: g = f + r has cancelled on both sides to below fp32's resolution of its operands, s_k <= GATE_F32 o_k. Two vertices that
    stick to an obstacle have g = f + r_p = 0: the fp64 walk gets s_k = 0 (or a residue of 1e-16), while ANY fp32 evaluation of f + r_p leaves a
    rounding residue of some 1e-7 (|f| + |r_p|), so the scale s_k the gate refers to is 0 / 0 there. Such a contact is compared on the scale of
    the operands instead, |diff| <= GATE k o_k — the quantity fp32 rounding is proportional to — and its state, decided by that residue, is
    not compared. Every other contact keeps the scale s_k, partial cancellation included. None of the eight oracle cases has such a contact;
    the flap lying on its sphere (tests/contact_readout_scenes.py) has twelve, eleven and ten in its three steps."""
    return w["s"] <= GATE_F32 * w["o"]


def oracle_inputs(name):
    """(case, f [N][3], r [N][3], mass, prim contacts, self contacts, rp [N][3]) of the oracle's record of a case of tests/selfdetect_cases.py"""
    import selfdetect_cases as sd
    case, o, ref, _, sc = sd.reference(name)
    f, r = o.record_fr(ref["id"])
    pc = o.prim_contacts(ref["id"])
    mass = o.vertex_data()[0]
    mu = case["sphere"]["mu"] if case["sphere"] is not None else 0.0
    rp = prim_part(f, pc["particle"], pc["normal"], mu)
    return case, f.reshape(-1, 3), r.reshape(-1, 3), mass, pc, sc, rp


@functools.lru_cache(maxsize=None)
def oracle_walk(name):
    """the oracle's record of a case and the fp64 walk `w` on it — computed once per process and shared; nobody writes to it"""
    case, f, r, mass, pc, sc, rp = oracle_inputs(name)
    pairs = np.stack([sc["p1"], sc["p2"]], axis=1)
    return dict(case=case, f=f, r=r, mass=mass, pc=pc, sc=sc, rp=rp, pairs=pairs, w=walk(f, mass, pairs, sc["layer"], sc["normal"], rp=rp))
