"""Flat-rest bending as per-vertex matrix rows on the device (csrc/dc_winlib.h: the row gather of the element windows; the forward set-up
of csrc/dc_forward_pk_kernel.h; the adjoint operator of csrc/dc_adjoint.hip), one workgroup per rollout (the split kernels keep their flaps).

Two flat grids dropped on the sphere — 48 x 34 (1 632 vertices: at least two element windows, PCG forward solve) and 24 x 24 (one window, the
explicit-inverse instances) — with k_stretch 150 and k_bend 1.0, so that bending carries a visible share of the force and a wrong row fails the
bar; settled with the oracle until primitive contacts exist (y != z at the contact vertices of the adjoint), then 3 consecutive steps, each
checked against the fp64 oracle with check_rollouts' three statements at its stated tolerances: positions 1e-5 L, gradients 1e-4 end to end,
same record (both directions) flat 1e-4, contact sets identical; the PD iteration count of the unperturbed rollout equals the oracle's.
The same scenes pass with DC_BEND_ROWS=0 (a fresh context per setting). The host tables are checked in tests/test_bend_rows.py.

Measured (MI355X, whole suite): worst end-to-end gradient error 2.7e-5 (dL/dmu; dL/dx, dL/dv <= 4.4e-7), same-record errors <= 6.6e-7, positions
1.2e-7, PD iteration counts and contact sets identical on every step of both scenes and both settings. With the forward threshold at 1e-8
instead of 1e-9 the first checked step of the 48 x 34 grid (rows on) came out at dL/dmu 1.01e-4 end to end with same-record errors of 1e-7 — the
step stops after 8 PD iterations there, and what differs is the iterate, not the adjoint; the tolerances were left as stated and the scenes run at
the threshold of the other flat-grid parity scenes. NOT recorded: a rows-on run with the own-slot difference dropped from the gather.

A mesh with curved flaps (the T-shirt) reports rows off, and two of its steps are bitwise equal with DC_BEND_ROWS unset and = 0."""
import numpy as np
import pytest

import meshes
import orc
import scenes
from diffcloth_amd import capi
from test_gpu_configs import check_rollouts

pytestmark = pytest.mark.gpu

L_SCENE = 4.5
H = 1.0 / 180
MAT = dict(density=0.3, k_stretch=150.0, k_bend=1.0)
RADIUS, MU = 2.0, 0.4
FWD_TOL = 1e-9          # the forward threshold of the flat-grid parity scenes (tests/test_gpu_parity.py: build_pair)
SETTLE, STEPS, B = 6, 3, 2


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


_trajectory = {}


def scene(nx, ny):
    """mesh, sphere centre, oracle and the oracle's settled trajectory (computed once per grid, shared by both settings, never changed)"""
    if (nx, ny) not in _trajectory:
        V, F = meshes.grid_cloth(nx, ny, L_SCENE, L_SCENE * (ny - 1) / (nx - 1), "DOWN")
        V = f32(V)
        c = f32(meshes.sphere_scene_center(V, RADIUS))
        o = orc.Oracle(V, F, h=H, fwd_tol=FWD_TOL, bwd_tol=1e-9, selfcollision=False, gradient_clipping=False, **MAT)
        o.add_sphere(c, RADIUS, MU)
        o.build()
        x = f32(V.reshape(-1) + np.tile([0.0, -0.06, 0.0], V.shape[0]))
        v = np.zeros_like(x)
        states = []
        for s in range(SETTLE + STEPS):
            if s >= SETTLE:
                states.append((x, v))
            out = o.step(x, v)
            assert out["converged"]
            x, v = f32(out["x"]), f32(out["v"])
            if s >= SETTLE:
                states[-1] += (int(out["iters"]), int(out["nprim"]))
        _trajectory[(nx, ny)] = (V, F, c, o, states)
    return _trajectory[(nx, ny)]


@pytest.mark.parametrize("rows", [True, False], ids=["rows", "DC_BEND_ROWS=0"])
@pytest.mark.parametrize("nx,ny,dense", [(48, 34, False), (24, 24, True)], ids=["48x34-two-windows", "24x24-explicit-inverse"])
def test_flat_grid_on_the_sphere_matches_the_oracle(nx, ny, dense, rows, monkeypatch):
    monkeypatch.setenv("DC_CLUSTER", "1")          # one workgroup per rollout: the kernels that read the rows
    if rows:
        monkeypatch.delenv("DC_BEND_ROWS", raising=False)
    else:
        monkeypatch.setenv("DC_BEND_ROWS", "0")
    V, F, c, o, states = scene(nx, ny)
    e = capi.Engine(0)
    try:
        e.set_mesh(V, F)
        e.set_params(time_step=H, forward_tol=FWD_TOL, backward_tol=1e-9, cg_rel_tol=1e-6, cg_max_iter=3000, gradient_clipping=0, selfcollision_enabled=0,
                     adjoint_mode=1, adjoint_rel_tol=1e-7, **MAT)
        e.set_primitives([dict(kind=capi.DC_PRIM_SPHERE, group=0, center=c, radius=RADIUS, mu=MU)])
        e.build()                                  # dc_build reads DC_BEND_ROWS
        lay = e.layout()
        assert lay["element_windows"] and lay["packet_kernel"] and lay["dense_inverse"] == dense
        assert lay["windows"] >= 2 if not dense else lay["windows"] == 1
        assert e.bend_rows() == rows
        rng = np.random.default_rng(12)
        for k, (x, v, iters, nprim) in enumerate(states):
            assert nprim >= 10, "primitive contacts must exist in the checked steps"
            X0 = np.stack([x] + [f32(x + 1e-4 * rng.standard_normal(x.size)) for _ in range(B - 1)])
            V0 = np.stack([v] + [f32(v + 1e-3 * rng.standard_normal(x.size)) for _ in range(B - 1)])
            st = check_rollouts(o, e, X0, V0, None, sample=tuple(range(B)), pos_tol=1e-5 * L_SCENE, grad_tol=1e-4, same_record_tol=1e-4, h=H,
                                scene=f"flat-grid-{nx}x{ny}-{'rows' if rows else 'flaps'}-step{k}")
            assert e.cluster() == 1
            print(f"\n[bend rows] {nx} x {ny} rows={rows} step {k}: PD iterations gpu {st['pd_iters'][0]} / oracle {iters}, contacts {st['prim_contacts'][0]} / {nprim}")
            assert st["pd_iters"][0] == iters and st["prim_contacts"][0] == nprim
    finally:
        e.close()


def tshirt_steps():
    cfg = scenes.TSHIRT
    V, F = scenes.load_mesh("tshirt")
    P, rmin, rmax = scenes.normalise_model(V, cfg["orientation"], cfg["cloth_dim"])
    P = f32(P)
    att = scenes.corner_attachments(P, rmin, rmax)
    e = capi.Engine(0)
    try:
        e.set_mesh(P, F)
        e.set_attachments(att)
        e.set_params(time_step=cfg["h"], density=cfg["density"], k_stretch=cfg["k_stretch"], k_bend=cfg["k_bend"], forward_tol=1e-7, backward_tol=1e-7,
                     cg_rel_tol=1e-6, cg_max_iter=3000, gradient_clipping=0, selfcollision_enabled=0, adjoint_mode=1)
        e.build()
        rows = e.bend_rows()
        S = 2
        e.alloc_batch(2, S)
        assert e.cluster() == 1
        rng = np.random.default_rng(3)
        X0 = np.stack([f32(P.reshape(-1) + 0.002 * rng.standard_normal(P.size)) for _ in range(2)])
        e.set_state(0, X0, np.zeros_like(X0))
        e.rollout_forward(0, S)
        e.seed_gradient(S, None, 1.0 / e.N)
        e.rollout_backward(S, S)
        out = {}
        for s in range(1, S + 1):
            out[f"x{s}"], out[f"v{s}"] = e.get_state(s)
            out[f"f{s}"], out[f"r{s}"] = e.get_record(s)
            out[f"pd{s}"] = e.get_stats(s)[0]["pd_iters"]
        out["dL_dx"], out["dL_dv"], out["dL_dmu"] = e.get_gradient()
        return rows, out
    finally:
        e.close()


def test_a_mesh_with_curved_flaps_keeps_its_flaps_bitwise(monkeypatch):
    monkeypatch.setenv("DC_CLUSTER", "1")
    monkeypatch.delenv("DC_BEND_ROWS", raising=False)
    rows_a, a = tshirt_steps()
    monkeypatch.setenv("DC_BEND_ROWS", "0")
    rows_b, b = tshirt_steps()
    assert not rows_a and not rows_b, "the T-shirt has curved flaps: rows must be refused"
    assert a["pd1"].min() > 1
    for k in a:
        p, q = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert p.dtype == q.dtype and p.shape == q.shape and p.tobytes() == q.tobytes(), f"{k} differs between DC_BEND_ROWS unset and = 0"
