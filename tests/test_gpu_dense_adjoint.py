"""adjoint_mode 2, the dense direct adjoint solve (csrc/dc_adjoint_dense.hip), against the fp64 oracle's exact solve.

Teacher forced as in tests/test_gpu_adjoint_options.py: the oracle runs a 4-step trajectory, its records go to the engine (dc_set_record),
and the backward chain runs from slot 4 to slot 1. Scenes: the pressed-on hat (primitive contacts, 579 vertices) and a 24 x 24 cloth on the
sphere with a folded flap (primitive and layered self contacts, 576 vertices).

  1. the matrix: dc_get_adjoint_matrix equals the oracle's K = P - dP^T of the same record within 1e-12 (relative, Frobenius) — on the
     columns of the vertices in self contact within SELF_MU_TOL: the engine's operator (apply_K64, dc_adjoint64.h) takes the cloth's
     self-friction coefficient as the fp32 constant kClothMu = fl32(0.1), the oracle as 0.1 (relative difference 1.5e-8; a self-contact
     factor S_l = I + ... only mixes the columns of its two vertices). Measured: hat 6.1e-14 (no self contacts); flap 3.5e-16, and 3.3e-10
     on the self-contact columns;
  2. the exact solve: the oracle solves every step with scipy's sparse LU of its own K (Orc.step_backward_lu, solveDirect's SparseLU,
     reference Simulation.cpp:1431-1440); both sides get the same fp32-rounded incoming gradient per step. Mode-2 gradients (dL_dx, dL_dv,
     dL_dmu, dL_ddensity, dL_dk where compared) within 1e-6 relative; every rollout converged with used_direct = 2, no fall-back
     iteration, 1 ... 3 substitutions and a relative fp64 residual <= 1e-10. Measured worst: hat 3.8e-8 (dL_dmu, dL_ddensity), flap 7.4e-7
     (dL_dk; dL_dx / dL_dv / dL_dmu <= 2.6e-8), one substitution per step, residuals 1.7e-13 / 5.1e-16;
  3. mode 2 and mode 1 agree within the suite's 1e-4 on the same records (measured: hat 3.2e-7, flap 1.0e-6);
  4. determinism: two contexts give bitwise-equal mode-2 gradients, and so does a run with one rollout per chunk (DC_DENSE_CHUNK=1);
  5. the rollout path: dc_rollout_backward over 10 steps of the hat x 64 in mode 2 is bitwise the dc_step_backward loop, within 1e-4 of mode 1.
  6. engine-level edges, on cloths dropped onto the sphere (primitive contacts, B = 3, 2 steps, against Orc.step_backward_lu at EXACT_TOL
     with the statistics of 2.): 3 x 3 (N = 9, n = 27, less than one panel), 10 x 10 (n = 300, n mod 64 = 44), 32 x 24 (N = 768, the limit);
     a partial last chunk (DC_DENSE_CHUNK=2 with B = 3: bitwise the unchunked gradients, K of rollout 2 equals the oracle's); gradient
     clipping in k_adjoint_dense_step (one rollout over the threshold, one under: `clipped` as predicted, EXACT_TOL against the LU chain
     fed the gradient pre-scaled in fp64, GRAD_TOL against mode 1); a zero gradient (outputs exactly zero, converged 1, used_direct 0,
     no cycle, the other rollouts bitwise unaffected); the fall-back of a flagged rollout (DC_DENSE_FLAG=1: converged, no substitution,
     fp64_iters > 0, residual <= adjoint_rel_tol, GRAD_TOL against the LU chain, rollouts 0 and 2 bitwise).
     Measured: sizes worst 2.5e-7 (dL_ddensity at n = 27; dL_dx / dL_dv 2.6 ... 3.5e-8), one substitution, residuals <= 5.7e-16; K of
     rollout 2 in the second chunk 8.8e-17; clipping 1.8e-7 against the LU chain, 3.2e-7 against mode 1; the fall-back rollout 6 fp64
     BiCGSTAB iterations per step, residual 3.0e-11, gradients 5.3e-8 (dL_ddensity; dL_dx 2.6e-8) from the LU chain. The seven tests
     add about 4 s to this module on an MI355X (24 s in all).
     Not tested: the "no progress, take the correction back" branch of k_adjoint_dense_step: no honest input reaches it.

Pivoting on the fixtures (test_matrix_matches_oracle computes and asserts it): scipy's partial pivoting swaps 56 / 74 rows (interleaved order;
68 / 98 in the kernels' planar order) of the hat's K of rollouts 0 / 1 (n = 1737: the attachment stiffness and the pressed-on contacts take it
away from diagonal dominance), and 0 rows of the flap's (n = 1728). So the scenes reach the swap paths only through about 5 % of the hat's
columns; the pivot search, the swaps, the factor layout and the tie rule are pinned on synthetic matrices by tests/test_gpu_dense_lu.py.
"""
import os

import numpy as np
import pytest
import scipy.linalg

import meshes
import orc
import records
from diffcloth_amd import capi, workloads
from test_gpu_adjoint_options import H, THREADS, Scene, cluster_env, f32, rel

pytestmark = pytest.mark.gpu
EXACT_TOL = 1e-6
GRAD_TOL = 1e-4
MATRIX_TOL = 1e-12
SELF_MU_TOL = 2 * abs(float(np.float32(0.1)) - 0.1) / 0.1      # 3e-8: see the module docstring


@pytest.fixture(scope="module")
def flap24():
    """A folded flap pressed onto a 24 x 24 cloth on the sphere (the flap scene of test_gpu_adjoint_options at a mesh the dense solve takes)"""
    nx, B = 24, 2
    V, F = meshes.grid_cloth(nx, nx, 4.5, 4.5, "DOWN")
    V = f32(V)
    c = f32(meshes.sphere_scene_center(V, 2.0))
    fab = dict(density=0.3, k_stretch=150.0, k_bend=1e-5)
    o = orc.Oracle(V, F, h=H, fwd_tol=1e-8, bwd_tol=1e-9, selfcollision=True, gradient_clipping=False, calc_atp=True, threads=THREADS, **fab)
    o.add_sphere(c, 2.0, 0.9)
    o.build()
    V0, flap_mask = meshes.fold_flap(V, nx, nx, 4, 0.05)
    X0 = np.empty((B, V.size))
    for b in range(B):
        rng = np.random.default_rng(3000 + b)
        X0[b] = f32((f32(V0) + np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.09, -0.03), rng.uniform(-0.3, 0.3)])).reshape(-1))
    MU = f32(np.array([[0.2], [0.7]]))

    def make_engine(**opts):
        e = capi.Engine(0)
        e.set_mesh(V, F)
        e.set_params(time_step=H, forward_tol=1e-8, backward_tol=1e-9, cg_rel_tol=1e-6, cg_max_iter=3000, gradient_clipping=0,
                     selfcollision_enabled=1, adjoint_rel_tol=1e-6, **fab, **opts)
        e.set_primitives([dict(kind=capi.DC_PRIM_SPHERE, group=0, center=c, radius=2.0, mu=0.9)])
        e.build()
        return e
    e = make_engine()
    field = np.zeros((V.shape[0], 3))
    field[flap_mask, 1] = -2.0 * 9.8 * e.vertex_data()[0][flap_mask]
    e.close()
    o.set_force_extras(None, f32(field.reshape(-1)), 1.0)
    sc = Scene(make_engine, o, X0, np.zeros_like(X0), MU)
    sc.o = o
    layers = [[int(np.max(q["self"]["layer"])) + 1 if len(q["self"]["layer"]) else 0 for q in row] for row in sc.recs]
    print(f"\n[flap24 scene] primitive contacts per step {sc.nprim}, self contacts per step {sc.nself}, layers {layers}")
    assert min(min(r) for r in sc.nself) > 0 and min(min(r) for r in sc.nprim) > 0 and max(max(r) for r in layers) >= 2
    yield sc


@pytest.fixture(scope="module")
def hat():
    """The hat pressed onto the head (the hat scene of test_gpu_adjoint_options: 18 lead-in steps run by the engine, two rollouts, then four
    oracle steps); dL_dk is left out for the reason given there."""
    w = workloads.hat_workload()
    B = 2
    X0, V0, lead_xf, timed, MU = w["start"](B, np.random.default_rng(0))
    p = w["params"]

    def make_engine(**opts):
        e = capi.Engine(0)
        e.set_mesh(w["P"], w["F"]); e.set_attachments(w["att"])
        e.set_params(forward_tol=w["fwd_tol"], backward_tol=5e-4, cg_rel_tol=1e-4, cg_max_iter=2000, gradient_clipping=0,
                     adjoint_rel_tol=1e-6, forward_deflation=1, **p, **opts)
        e.set_primitives(w["prims"]); e.build()
        return e
    e = make_engine(adjoint_mode=1)
    L = len(lead_xf)
    with cluster_env(1):
        e.alloc_batch(B, L)
    e.set_mu(MU)
    e.set_state(0, X0, V0)
    e.set_fixed_point_schedule(0, lead_xf)
    e.rollout_forward(0, L)
    XL, VL = e.get_state(L)
    e.close()
    prim = w["prims"][0]
    o = orc.Oracle(w["P"], w["F"], h=p["time_step"], density=p["density"], k_stretch=p["k_stretch"], k_bend=p["k_bend"], attachments=w["att"],
                   fwd_tol=w["fwd_tol"], bwd_tol=5e-4, selfcollision=False, gradient_clipping=False, calc_atp=True, threads=THREADS)
    o.add_sphere(prim["center"], prim["radius"], prim["mu"])
    o.build()
    sc = Scene(make_engine, o, XL, VL, MU, xf=timed(4), dk_types=())
    sc.o = o
    print(f"\n[hat scene] primitive contacts per step {sc.nprim}")
    assert min(min(r) for r in sc.nprim) > 0
    yield sc


def scene(request, name):
    sc = request.getfixturevalue(name)
    if not hasattr(sc, "lu_chain"):
        sc.lu_chain = lu_chain(sc)
    return sc


def lu_chain(sc, gx0=None, gv0=None, clip_thr=None):
    """the oracle's backward chain with the sparse-LU solve; every step's input is the fp32 rounding of the step above's output (what the
    engine's carried gradient holds). gx0 / gv0: another gradient into the last step. clip_thr: gradient clipping as the engine applies
    it (Simulation.cpp:1460-1466: dL_dxnew of a rollout with |dL_dxnew| > thr N is scaled to that norm), done here in fp64 on the
    oracle's input, since step_backward_lu takes g as passed; chain[s]["clipped"] says which rollouts it scaled."""
    steps, B = len(sc.refs), sc.MU.shape[0]
    gx, gv = sc.chain[steps - 1]["gx"] if gx0 is None else gx0, sc.chain[steps - 1]["gv"] if gv0 is None else gv0
    chain = [None] * steps
    for s in range(steps - 1, -1, -1):
        gx, gv = f32(gx), f32(gv)
        outs, clipped, norms = [], [], []
        for b in range(B):
            sc.o.set_mu(0, float(sc.MU[b, 0]))
            g, nrm = gx[b], float(np.linalg.norm(gx[b]))
            lim = None if clip_thr is None else clip_thr * (g.size // 3)
            clipped.append(int(lim is not None and nrm > lim))
            norms.append(nrm)
            if clipped[-1]:
                g = g * (lim / nrm)
            outs.append(sc.o.step_backward_lu(sc.refs[s][b]["id"], g, gv[b], is_start=(s == 0)))
        chain[s] = dict(gx=gx, gv=gv, out=outs, clipped=clipped, norms=norms)
        gx = np.stack([q["dL_dx"] for q in outs]); gv = np.stack([q["dL_dv"] for q in outs])
    return chain


def run_chain(sc, chain, **opts):
    """the engine over the oracle's records, each step fed the chain's input; per step (slot, step_backward dict, param gradients)"""
    e = sc.make_engine(**opts)
    B, steps = sc.MU.shape[0], len(sc.refs)
    try:
        with cluster_env(1):
            e.alloc_batch(B, steps + 1)
        e.set_mu(sc.MU)
        got = []
        for s in range(steps - 1, -1, -1):
            e.set_state(s, *sc.starts[s])
            records.upload_oracle_records(e, s + 1, sc.recs[s], x_fixed=None if sc.xf is None else sc.xf[s])
            gb = e.step_backward(s + 1, chain[s]["gx"], chain[s]["gv"], is_start=(s == 0))
            got.append((s + 1, gb, e.get_param_gradients(s + 1)))
        return got
    finally:
        e.close()


def errors(sc, chain, got):
    worst = {}
    for slot, gb, pg in got:
        for b, rb in enumerate(chain[slot - 1]["out"]):
            e = dict(dx=rel(gb["dL_dx"][b], rb["dL_dx"]), dv=rel(gb["dL_dv"][b], rb["dL_dv"]), dmu=records.mu_err(gb["dL_dmu"][b], rb["dL_dmu"]),
                     ddensity=abs(pg["dL_ddensity"][b] - rb["dL_ddensity"]) / max(abs(rb["dL_ddensity"]), 1e-30))
            if sc.dk_types:
                e["dk"] = rel(pg["dL_dk"][b][sc.dk_types], rb["dL_dk"][sc.dk_types])
            for k, v in e.items():
                worst[k] = max(worst.get(k, 0.0), v)
    return worst


SCENES = ["hat", "flap24"]


@pytest.mark.parametrize("name", SCENES)
def test_matrix_matches_oracle(request, name):
    sc = scene(request, name)
    e = sc.make_engine(adjoint_mode=2)
    try:
        B = sc.MU.shape[0]
        with cluster_env(1):
            e.alloc_batch(B, 2)
        e.set_mu(sc.MU)
        s = len(sc.refs) - 1
        e.set_state(0, *sc.starts[s])
        records.upload_oracle_records(e, 1, sc.recs[s], x_fixed=None if sc.xf is None else sc.xf[s])
        worst, worst_self = 0.0, 0.0
        for b in range(B):
            sc.o.set_mu(0, float(sc.MU[b, 0]))
            Ko = sc.o.adjoint_matrix(sc.refs[s][b]["id"]).toarray()
            Kd = e.adjoint_matrix(1, b)
            planar = np.arange(Ko.shape[0]).reshape(-1, 3).T.reshape(-1)      # the kernels' row order (component-major)
            swaps = [int(np.count_nonzero(scipy.linalg.lu_factor(M)[1] != np.arange(M.shape[0]))) for M in (Ko, Ko[np.ix_(planar, planar)])]
            print(f"[{name}] rollout {b}: rows swapped by scipy's partial pivoting on the oracle's K: {swaps[0]} interleaved, {swaps[1]} planar")
            assert (min(swaps) > 0) if name == "hat" else (swaps == [0, 0]), (name, b, swaps)      # the module docstring's figures
            selfv = np.zeros(Ko.shape[0] // 3, dtype=bool)
            selfv[sc.recs[s][b]["self"]["pairs"].reshape(-1)] = True
            cols = np.repeat(selfv, 3)
            worst = max(worst, float(np.linalg.norm(Kd[:, ~cols] - Ko[:, ~cols]) / np.linalg.norm(Ko[:, ~cols])))
            if cols.any():
                worst_self = max(worst_self, float(np.linalg.norm(Kd[:, cols] - Ko[:, cols]) / np.linalg.norm(Ko[:, cols])))
        print(f"[{name}] |K_device - K_oracle|_F / |K_oracle|_F: {worst:.2e}, on the columns of self-contact vertices {worst_self:.2e}")
        assert worst <= MATRIX_TOL and worst_self <= SELF_MU_TOL
    finally:
        e.close()


@pytest.mark.parametrize("name", SCENES)
def test_exact_solve_parity_and_mode1_agreement(request, name):
    sc = scene(request, name)
    got2 = run_chain(sc, sc.lu_chain, adjoint_mode=2)
    for slot, gb, _ in got2:
        print(f"[{name} mode 2] slot {slot}: converged {gb['converged'].tolist()} used_direct {gb['used_direct'].tolist()} "
              f"refine {gb['refine_cycles'].tolist()} fp64 {gb['fp64_iters'].tolist()} last_udiff {np.array2string(gb['last_udiff'], precision=2)}")
        assert (gb["converged"] == 1).all() and (gb["used_direct"] == 2).all() and (gb["fp64_iters"] == 0).all()
        assert ((gb["refine_cycles"] >= 1) & (gb["refine_cycles"] <= 3)).all() and (gb["last_udiff"] <= 1e-10).all()
        assert (gb["adjoint_iters"] == 0).all() and (gb["cg_iters"] == 0).all() and (gb["residual_verified"] == 1).all()
        assert (gb["workgroups"] == 1).all()
    w2 = errors(sc, sc.lu_chain, got2)
    print(f"[{name}] mode 2 vs the oracle's sparse LU: " + " ".join(f"{k} {v:.1e}" for k, v in w2.items()))
    assert max(w2.values()) <= EXACT_TOL
    got1 = run_chain(sc, sc.lu_chain, adjoint_mode=1)
    worst = 0.0
    for (slot, g2, p2), (_, g1, p1) in zip(got2, got1):
        for b in range(sc.MU.shape[0]):
            worst = max(worst, rel(g2["dL_dx"][b], g1["dL_dx"][b]), rel(g2["dL_dv"][b], g1["dL_dv"][b]),
                        records.mu_err(g2["dL_dmu"][b], g1["dL_dmu"][b]))
    print(f"[{name}] mode 2 vs mode 1: {worst:.1e}")
    assert worst <= GRAD_TOL


def test_bitwise_determinism_and_chunking(request):
    sc = scene(request, "flap24")
    a = run_chain(sc, sc.lu_chain, adjoint_mode=2)
    b = run_chain(sc, sc.lu_chain, adjoint_mode=2)
    old = os.environ.get("DC_DENSE_CHUNK")
    os.environ["DC_DENSE_CHUNK"] = "1"
    try:
        c = run_chain(sc, sc.lu_chain, adjoint_mode=2)
    finally:
        if old is None:
            os.environ.pop("DC_DENSE_CHUNK", None)
        else:
            os.environ["DC_DENSE_CHUNK"] = old
    for other in (b, c):
        for (slot, g, p), (_, g2, p2) in zip(a, other):
            for k in ("dL_dx", "dL_dv", "dL_dmu"):
                assert np.array_equal(g[k], g2[k]), (slot, k)
            assert np.array_equal(p["dL_ddensity"], p2["dL_ddensity"])


def test_rollout_backward_matches_step_loop_hat64():
    w = workloads.hat_workload()
    B, K = 64, 10
    X0, V0, lead_xf, timed, MU = w["start"](B, np.random.default_rng(1))
    L = len(lead_xf)

    def engine(mode):
        e = capi.Engine(0)
        e.set_mesh(w["P"], w["F"]); e.set_attachments(w["att"])
        e.set_params(forward_tol=w["fwd_tol"], backward_tol=5e-4, cg_rel_tol=1e-4, cg_max_iter=2000, gradient_clipping=0,
                     adjoint_mode=mode, **w["params"])
        e.set_primitives(w["prims"]); e.build()
        e.alloc_batch(B, L + K)
        e.set_mu(MU)
        e.set_state(0, X0, V0)
        e.set_fixed_point_schedule(0, np.concatenate([lead_xf, timed(K)]))
        e.rollout_forward(0, L + K)
        return e
    rng = np.random.default_rng(5)
    gx0 = f32(rng.standard_normal((B, 3 * w["P"].shape[0]))); gv0 = f32(0.01 * rng.standard_normal(gx0.shape))
    e2 = engine(2)
    try:
        e2.set_gradient(gx0, gv0)
        e2.kernel_times(reset=True)
        e2.rollout_backward(L + K, K)
        kt = e2.kernel_times()
        rx, rv, _ = e2.get_gradient()
        st = e2.get_stats(L + 1)[1]
        assert (st["used_direct"] == 2).all() and (st["converged"] == 1).all(), st
        assert kt["bwd_launches"] > K and kt["bwd_ms"] > 0
        gx, gv = gx0, gv0
        for s in range(L + K, L, -1):
            gb = e2.step_backward(s, gx, gv, is_start=False)
            gx, gv = gb["dL_dx"], gb["dL_dv"]
        assert np.array_equal(rx, gx) and np.array_equal(rv, gv)
    finally:
        e2.close()
    e1 = engine(1)
    try:
        e1.set_gradient(gx0, gv0)
        e1.rollout_backward(L + K, K)
        mx, mv, _ = e1.get_gradient()
    finally:
        e1.close()
    worst = max(max(rel(rx[b], mx[b]), rel(rv[b], mv[b])) for b in range(B))
    print(f"[hat x 64, {K} steps] rollout mode 2 vs mode 1: {worst:.1e}")
    assert worst <= GRAD_TOL


# ---------------------------------------------------------------------------------------------------------------- engine-level edges of mode 2
class env_var:
    def __init__(self, name, value):
        self.name, self.value = name, str(value)

    def __enter__(self):
        self.old = os.environ.get(self.name)
        os.environ[self.name] = self.value

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.old


# N = 9 (n = 27 < one panel; its middle vertex moved over the top of the sphere), N = 100 (n = 300, n mod 64 = 44), N = 768 (n = 2304)
GRIDS = {"tiny": (3, 3, (0.6, -0.12, 0.2)), "mid": (10, 10, (0.0, -0.04, 0.0)), "limit": (32, 24, (0.0, -0.04, 0.0))}


def sphere_cloth(nx, ny, shift):
    """an nx x ny cloth, moved by `shift` (and 0.02 further down per rollout), dropped onto the sphere: primitive contacts only, three rollouts (mu 0.2, 0.5, 0.8), two oracle steps"""
    B = 3
    V, F = meshes.grid_cloth(nx, ny, 4.5, 4.5, "DOWN")
    V = f32(V)
    c = f32(meshes.sphere_scene_center(V, 2.0))
    fab = dict(density=0.3, k_stretch=150.0, k_bend=0.05)
    # forward tolerance 1e-12: dL_dk is compared, and the oracle forms it from A^T p of its LAST PD iterate while the engine re-forms p from
    # the record's x_new (see the hat fixture of test_gpu_adjoint_options); the two agree as far as the forward solve has converged
    o = orc.Oracle(V, F, h=H, fwd_tol=1e-12, bwd_tol=1e-9, selfcollision=False, gradient_clipping=False, calc_atp=True, threads=THREADS, **fab)
    o.add_sphere(c, 2.0, 0.5)
    o.build()
    X0 = np.empty((B, V.size))
    for b in range(B):
        X0[b] = f32(V.reshape(-1) + np.tile([shift[0], shift[1] - 0.02 * b, shift[2]], V.shape[0]))
    MU = f32(np.array([[0.2], [0.5], [0.8]]))

    def make_engine(**opts):
        opts.setdefault("gradient_clipping", 0)
        e = capi.Engine(0)
        e.set_mesh(V, F)
        e.set_params(time_step=H, forward_tol=1e-12, backward_tol=1e-9, cg_rel_tol=1e-6, cg_max_iter=3000, selfcollision_enabled=0,
                     adjoint_rel_tol=1e-6, **fab, **opts)
        e.set_primitives([dict(kind=capi.DC_PRIM_SPHERE, group=0, center=c, radius=2.0, mu=0.5)])
        e.build()
        return e
    sc = Scene(make_engine, o, X0, np.zeros_like(X0), MU, steps=2)
    sc.o = o
    print(f"\n[sphere cloth {nx} x {ny}] primitive contacts per step {sc.nprim}")
    assert min(min(r) for r in sc.nprim) > 0
    return sc


@pytest.fixture(scope="module")
def tiny():
    yield sphere_cloth(*GRIDS["tiny"])


@pytest.fixture(scope="module")
def mid():
    yield sphere_cloth(*GRIDS["mid"])


@pytest.fixture(scope="module")
def limit():
    yield sphere_cloth(*GRIDS["limit"])


def assert_direct_stats(gb, rollouts=None):
    """what test_exact_solve_parity_and_mode1_agreement asserts of a step solved by the factors"""
    q = slice(None) if rollouts is None else rollouts
    assert (gb["converged"][q] == 1).all() and (gb["used_direct"][q] == 2).all() and (gb["fp64_iters"][q] == 0).all()
    assert ((gb["refine_cycles"][q] >= 1) & (gb["refine_cycles"][q] <= 3)).all() and (gb["last_udiff"][q] <= 1e-10).all()
    assert (gb["adjoint_iters"][q] == 0).all() and (gb["cg_iters"][q] == 0).all() and (gb["residual_verified"][q] == 1).all()
    assert (gb["workgroups"][q] == 1).all()


def assert_bitwise(a, b, rollouts, what):
    for (slot, g, p), (_, g2, p2) in zip(a, b):
        for k in ("dL_dx", "dL_dv", "dL_dmu"):
            assert np.array_equal(g[k][rollouts], g2[k][rollouts]), (what, slot, k)
        assert np.array_equal(np.asarray(p["dL_ddensity"])[rollouts], np.asarray(p2["dL_ddensity"])[rollouts]), (what, slot)


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_sizes_on_the_device(request, name):
    """below one panel, a trailing matrix that is no multiple of the tile, and the advertised limit, through the engine"""
    sc = scene(request, name)
    got = run_chain(sc, sc.lu_chain, adjoint_mode=2)
    for slot, gb, _ in got:
        print(f"[{name} mode 2] slot {slot}: refine {gb['refine_cycles'].tolist()} last_udiff {np.array2string(gb['last_udiff'], precision=2)}")
        assert_direct_stats(gb)
    w = errors(sc, sc.lu_chain, got)
    print(f"[{name}, n = {sc.starts[0][0].shape[1]}] mode 2 vs the oracle's sparse LU: " + " ".join(f"{k} {v:.1e}" for k, v in w.items()))
    assert max(w.values()) <= EXACT_TOL


def test_partial_last_chunk(request):
    sc = scene(request, "mid")
    whole = run_chain(sc, sc.lu_chain, adjoint_mode=2)
    with env_var("DC_DENSE_CHUNK", 2):
        parts = run_chain(sc, sc.lu_chain, adjoint_mode=2)
        e = sc.make_engine(adjoint_mode=2)
        try:
            with cluster_env(1):
                e.alloc_batch(3, 2)
            e.set_mu(sc.MU)
            s = len(sc.refs) - 1
            e.set_state(0, *sc.starts[s])
            records.upload_oracle_records(e, 1, sc.recs[s], x_fixed=None)
            sc.o.set_mu(0, float(sc.MU[2, 0]))
            Ko = sc.o.adjoint_matrix(sc.refs[s][2]["id"]).toarray()
            err = float(np.linalg.norm(e.adjoint_matrix(1, 2) - Ko) / np.linalg.norm(Ko))
        finally:
            e.close()
    assert_bitwise(whole, parts, slice(None), "DC_DENSE_CHUNK=2")
    print(f"[mid, chunks of 2] K of rollout 2 vs the oracle: {err:.2e}")
    assert err <= MATRIX_TOL


def test_clipping(request):
    """k_adjoint_dense_step's own copy of the clipping code: rollout 0 over the threshold, rollout 1 under it"""
    sc = scene(request, "mid")
    N, thr = sc.starts[0][0].shape[1] // 3, 0.05
    gx0 = sc.chain[-1]["gx"] * np.array([1.0, 0.01, 1.0])[:, None]
    chain = lu_chain(sc, gx0=gx0, gv0=sc.chain[-1]["gv"], clip_thr=thr)
    last = chain[-1]
    print(f"[clipping] threshold {thr * N}: |gx| per step {[np.round(c['norms'], 3).tolist() for c in chain]}, clipped {[c['clipped'] for c in chain]}")
    assert last["clipped"][0] == 1 and last["clipped"][1] == 0
    for c in chain:                                  # no rollout so close to the threshold that fp32 sums could decide otherwise
        assert all(abs(nrm - thr * N) > 1e-3 * thr * N for nrm in c["norms"])
    got2 = run_chain(sc, chain, adjoint_mode=2, gradient_clipping=1, gradient_clipping_threshold=thr)
    for (slot, gb, _) in got2:
        assert gb["clipped"].tolist() == chain[slot - 1]["clipped"], (slot, gb["clipped"])
        assert_direct_stats(gb)
    w = errors(sc, chain, got2)
    print("[clipping] mode 2 vs the LU chain on the pre-scaled gradient: " + " ".join(f"{k} {v:.1e}" for k, v in w.items()))
    assert max(w.values()) <= EXACT_TOL
    got1 = run_chain(sc, chain, adjoint_mode=1, gradient_clipping=1, gradient_clipping_threshold=thr)
    worst = 0.0
    for (slot, g2, p2), (_, g1, p1) in zip(got2, got1):
        assert g1["clipped"].tolist() == g2["clipped"].tolist()
        for b in range(3):
            worst = max(worst, rel(g2["dL_dx"][b], g1["dL_dx"][b]), rel(g2["dL_dv"][b], g1["dL_dv"][b]), records.mu_err(g2["dL_dmu"][b], g1["dL_dmu"][b]))
    print(f"[clipping] mode 2 vs mode 1: {worst:.1e}")
    assert worst <= GRAD_TOL


def test_zero_gradient_rollout(request):
    sc = scene(request, "mid")
    base = run_chain(sc, sc.lu_chain, adjoint_mode=2)
    chain = []
    for c in sc.lu_chain:
        gx, gv = c["gx"].copy(), c["gv"].copy()
        gx[1] = 0.0; gv[1] = 0.0
        chain.append(dict(gx=gx, gv=gv, out=c["out"]))
    got = run_chain(sc, chain, adjoint_mode=2)
    for slot, gb, pg in got:
        for k in ("dL_dx", "dL_dv", "dL_dmu"):
            assert not np.any(gb[k][1]), (slot, k)
        assert np.asarray(pg["dL_ddensity"])[1] == 0.0 and not np.any(np.asarray(pg["dL_dk"])[1])
        assert gb["converged"][1] == 1 and gb["used_direct"][1] == 0 and gb["refine_cycles"][1] == 0 and gb["fp64_iters"][1] == 0
        assert_direct_stats(gb, [0, 2])
    assert_bitwise(base, got, [0, 2], "zero gradient in rollout 1")


def test_flagged_rollout_takes_the_fp64_fallback(request):
    """DC_DENSE_FLAG=1 marks rollout 1 as if its factorisation had met a zero pivot: bicgstab64 from u = 0"""
    sc = scene(request, "mid")
    base = run_chain(sc, sc.lu_chain, adjoint_mode=2)
    with env_var("DC_DENSE_FLAG", 1):
        got = run_chain(sc, sc.lu_chain, adjoint_mode=2)
    for slot, gb, _ in got:
        print(f"[flagged rollout 1] slot {slot}: converged {gb['converged'].tolist()} refine {gb['refine_cycles'].tolist()} "
              f"fp64 {gb['fp64_iters'].tolist()} last_udiff {np.array2string(gb['last_udiff'], precision=2)}")
        assert gb["converged"][1] == 1 and gb["refine_cycles"][1] == 0 and gb["fp64_iters"][1] > 0 and gb["last_udiff"][1] <= 1e-6
        assert gb["used_direct"][1] == 2 and gb["residual_verified"][1] == 1
        assert_direct_stats(gb, [0, 2])
    assert_bitwise(base, got, [0, 2], "DC_DENSE_FLAG=1")
    worst = {}
    for slot, gb, pg in got:
        rb = sc.lu_chain[slot - 1]["out"][1]
        e = dict(dx=rel(gb["dL_dx"][1], rb["dL_dx"]), dv=rel(gb["dL_dv"][1], rb["dL_dv"]), dmu=records.mu_err(gb["dL_dmu"][1], rb["dL_dmu"]),
                 ddensity=abs(pg["dL_ddensity"][1] - rb["dL_ddensity"]) / max(abs(rb["dL_ddensity"]), 1e-30))
        for k, v in e.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("[flagged rollout 1] fall-back vs the LU chain: " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert max(worst.values()) <= GRAD_TOL
