"""The adjoint solve's public options against the fp64 oracle (Simulation::stepBackward with the direct solve, Simulation.cpp:1431-1440,
1455-1780): adjoint_mode, adjoint_block_precond and adjoint_fp32_only (include/diffcloth_hip.h), on the one-workgroup and the split
adjoint kernels (dc_adjoint.hip, dc_adjoint_cl.hip), and on the coarse-level instances (the hat: deflation vectors as the coarse level of the
block preconditioner and of the fp64 fall-back).

Teacher forced: the oracle runs a 4-step trajectory and its records are handed to the engine (dc_set_record), so both sides differentiate
the SAME record and the comparison measures the adjoint solve alone, not the forward's summation order. The backward chain runs from slot 4
to slot 1 (is_start on slot 1); every step gets the oracle's outgoing gradient of the step above as its input and is compared on dL_dx,
dL_dv, dL_dmu and the parameter gradients dL_dk, dL_ddensity.

Gates:
  * mixed precision (adjoint_fp32_only = 0): every rollout converged (1), the fp64-evaluated residual within adjoint_rel_tol (1 % slack for
    the fp32 rounding of last_udiff), gradients within the suite's 1e-4 relative;
  * adjoint_fp32_only = 1: one fp32 BiCGSTAB solve, nothing after it — no fp64 fall-back, no fp64-verified residual, and (adjoint_mode 1)
    no CG: that mode has no stage that could take over from a CG cycle on its short leash, nor from a coarse-level solve's early
    hand-over. On the flap no rollout unconverged (0) and gradients within FP32_ONLY_TOL = 5e-4, the header's documented accuracy of the
    mode (eps_fp32 * cond(K), 1-3e-4 on stiff / large scenes; measured <= 1.1e-4, on dL_ddensity). The hat's systems are beyond fp32 (the
    mixed-precision solve finishes them in fp64): there a rollout may end unconverged, but only after the mode's whole budget of
    4 x adjoint_iter_cap iterations, and the rollouts it reports converged are within FP32_BEYOND_TOL = 1e-2 (measured <= 5e-3);
  * the statistics name the method: adjoint_mode 1 runs CG (cg_iters > 0) exactly where CG-first applies — mixed precision with the
    diag(P) preconditioner — and none elsewhere;
  * adjoint_mode 0 (the reference's fixed-point iteration, one workgroup per rollout even on a split tape: workgroups == 1) to the
    same gradient gate, its stopping rule set tight (backward_tol 1e-9)."""
import os

import numpy as np
import pytest

import meshes
import orc
import records
from diffcloth_amd import capi, workloads

pytestmark = pytest.mark.gpu
H = 1.0 / 180
REL_TOL = 1e-6            # adjoint_rel_tol (the default)
GRAD_TOL = 1e-4
FP32_ONLY_TOL = 5e-4
FP32_BEYOND_TOL = 1e-2
FP32_BUDGET = 4 * 400     # iterations of the fp32-only solve: 4 x adjoint_iter_cap (default 400)
THREADS = min(os.cpu_count() or 1, 32)


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-30))


class cluster_env:
    def __init__(self, k):
        self.k = k

    def __enter__(self):
        self.old = os.environ.get("DC_CLUSTER")
        os.environ["DC_CLUSTER"] = str(self.k)

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("DC_CLUSTER", None)
        else:
            os.environ["DC_CLUSTER"] = self.old


def oracle_trajectory(o, X0, V0, MU, xf=None, steps=4):
    """per rollout: `steps` oracle steps, each from the fp32 rounding of the previous step's state (the engine's tape holds fp32 states);
    returns the start states of the steps [steps][B] and the oracle records [steps][B]"""
    B = X0.shape[0]
    starts = [(f32(X0), f32(V0))]
    refs = [[None] * B for _ in range(steps)]
    for s in range(steps):
        xs, vs = starts[-1]
        xn, vn = np.empty_like(xs), np.empty_like(vs)
        for b in range(B):
            o.set_mu(0, float(MU[b, 0]))
            ref = o.step(xs[b], vs[b], None if xf is None else xf[s][b])
            refs[s][b] = ref
            xn[b], vn[b] = ref["x"], ref["v"]
        starts.append((f32(xn), f32(vn)))
    return starts, refs


def oracle_chain(o, refs, MU, gx, gv):
    """the oracle's backward chain (direct solve) from the last step to the first: per step the incoming (gx, gv) and its outputs"""
    steps, B = len(refs), len(refs[0])
    chain = [None] * steps
    for s in range(steps - 1, -1, -1):
        outs = []
        for b in range(B):
            o.set_mu(0, float(MU[b, 0]))
            outs.append(o.step_backward(refs[s][b]["id"], gx[b], gv[b], is_start=(s == 0), direct=True))
        chain[s] = dict(gx=gx, gv=gv, out=outs)
        gx = np.stack([q["dL_dx"] for q in outs]); gv = np.stack([q["dL_dv"] for q in outs])
    return chain


class Scene:
    """engine factory + the oracle's trajectory, records and backward chain (shared by every option of the matrix)"""

    def __init__(self, make_engine, o, X0, V0, MU, xf=None, steps=4, seed=7, dk_types=(0, 1, 2)):
        self.make_engine, self.MU, self.xf, self.dk_types = make_engine, MU, xf, list(dk_types)
        self.starts, self.refs = oracle_trajectory(o, X0, V0, MU, xf, steps)
        self.recs = [[records.oracle_record(o, r) for r in row] for row in self.refs]
        rng = np.random.default_rng(seed)
        gx = f32(rng.standard_normal(X0.shape)); gv = f32(0.01 * rng.standard_normal(X0.shape))
        self.chain = oracle_chain(o, self.refs, MU, gx, gv)
        self.nprim = [[r["nprim"] for r in row] for row in self.refs]
        self.nself = [[r["nself"] for r in row] for row in self.refs]


@pytest.fixture(scope="module")
def flap():
    """A folded flap pressed onto the 40 x 40 cloth on the sphere (tests/test_gpu_cluster.py::test_split_kernels_with_self_contacts):
    primitive contacts, self contacts in layers, sticking and sliding; four rollouts, mu 0.1 ... 0.9."""
    nx, B = 40, 4
    V, F = meshes.grid_cloth(nx, nx, 4.5, 4.5, "DOWN")
    V = f32(V)
    c = f32(meshes.sphere_scene_center(V, 2.0))
    fab = dict(density=0.3, k_stretch=150.0, k_bend=1e-5)
    o = orc.Oracle(V, F, h=H, fwd_tol=1e-8, bwd_tol=1e-9, selfcollision=True, gradient_clipping=False, calc_atp=True, threads=THREADS, **fab)
    o.add_sphere(c, 2.0, 0.9)
    o.build()
    V0, flap_mask = meshes.fold_flap(V, nx, nx, 6, 0.05)
    X0 = np.empty((B, V.size))
    for b in range(B):
        rng = np.random.default_rng(2000 + b)
        X0[b] = f32((f32(V0) + np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.09, -0.03), rng.uniform(-0.4, 0.4)])).reshape(-1))
    MU = f32(np.array([[0.1], [0.35], [0.6], [0.9]]))

    def make_engine(**opts):
        e = capi.Engine(0)
        e.set_mesh(V, F)
        e.set_params(time_step=H, forward_tol=1e-8, backward_tol=1e-9, cg_rel_tol=1e-6, cg_max_iter=3000, gradient_clipping=0,
                     selfcollision_enabled=1, adjoint_rel_tol=REL_TOL, **fab, **opts)
        e.set_primitives([dict(kind=capi.DC_PRIM_SPHERE, group=0, center=c, radius=2.0, mu=0.9)])
        e.build()
        return e
    e = make_engine()
    field = np.zeros((V.shape[0], 3))
    field[flap_mask, 1] = -2.0 * 9.8 * e.vertex_data()[0][flap_mask]
    e.close()
    o.set_force_extras(None, f32(field.reshape(-1)), 1.0)
    sc = Scene(make_engine, o, X0, np.zeros_like(X0), MU)
    print(f"\n[flap scene] primitive contacts per step {sc.nprim}, self contacts per step {sc.nself}")
    assert min(min(r) for r in sc.nself) > 100 and min(min(r) for r in sc.nprim) > 0
    yield sc


@pytest.fixture(scope="module")
def hat():
    """The hat pressed onto the head (workloads.hat_workload: 18 lead-in steps of the clips run by the engine), two rollouts, then four
    oracle steps. forward_deflation = 1: the adjoint's block preconditioner and fp64 fall-back get the coarse level (COARSE instances)."""
    w = workloads.hat_workload()
    B = 2
    X0, V0, lead_xf, timed, MU = w["start"](B, np.random.default_rng(0))
    p = w["params"]

    def make_engine(**opts):
        e = capi.Engine(0)
        e.set_mesh(w["P"], w["F"]); e.set_attachments(w["att"])
        e.set_params(forward_tol=w["fwd_tol"], backward_tol=5e-4, cg_rel_tol=1e-4, cg_max_iter=2000, gradient_clipping=0,
                     adjoint_rel_tol=REL_TOL, forward_deflation=1, **p, **opts)
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
    # dL_dk is left out here: the oracle keeps A^T p of the LAST PD iterate (calcSeparateAtp, Simulation.cpp:1212-1218), the engine re-forms
    # p from the record's x_new (dc_adjoint64.h), and with the hat's forward_tol of 1e-6 the two differ by 5e-4 ... 7e-2 (bending the most)
    # — the same in every option of the matrix, so not a property of the solve this module tests
    sc = Scene(make_engine, o, XL, VL, MU, xf=timed(4), dk_types=())
    print(f"\n[hat scene] primitive contacts per step {sc.nprim}")
    assert min(min(r) for r in sc.nprim) > 0
    yield sc


def run_case(sc, K, **opts):
    """the engine's backward chain over the oracle's records; per step (stats, worst gradient errors over the rollouts)"""
    e = sc.make_engine(**opts)
    B, steps = sc.MU.shape[0], len(sc.refs)
    try:
        with cluster_env(K):
            e.alloc_batch(B, steps + 1)
        assert e.cluster() == K
        e.set_mu(sc.MU)
        got = []
        for s in range(steps - 1, -1, -1):
            e.set_state(s, *sc.starts[s])
            records.upload_oracle_records(e, s + 1, sc.recs[s], x_fixed=None if sc.xf is None else sc.xf[s])
            ch = sc.chain[s]
            gb = e.step_backward(s + 1, ch["gx"], ch["gv"], is_start=(s == 0))
            pg = e.get_param_gradients(s + 1)
            err = {k: np.zeros(B) for k in ("dx", "dv", "dmu", "dk", "ddensity")}      # per rollout
            for b, rb in enumerate(ch["out"]):
                err["dx"][b] = rel(gb["dL_dx"][b], rb["dL_dx"])
                err["dv"][b] = rel(gb["dL_dv"][b], rb["dL_dv"])
                err["dmu"][b] = records.mu_err(gb["dL_dmu"][b], rb["dL_dmu"])
                err["dk"][b] = rel(pg["dL_dk"][b][sc.dk_types], rb["dL_dk"][sc.dk_types])
                err["ddensity"][b] = abs(pg["dL_ddensity"][b] - rb["dL_ddensity"]) / max(abs(rb["dL_ddensity"]), 1e-30)
            got.append((s + 1, gb, err))
        return got
    finally:
        e.close()


def report(tag, got):
    for slot, gb, err in got:
        print(f"[{tag}] slot {slot}: converged {gb['converged'].tolist()} last_udiff {np.array2string(gb['last_udiff'], precision=2)} "
              f"adjoint {gb['adjoint_iters'].tolist()} cg {gb['cg_iters'].tolist()} fp64 {gb['fp64_iters'].tolist()} "
              f"verified {gb['residual_verified'].tolist()} workgroups {gb['workgroups'].tolist()} | "
              + " ".join(f"{k} {v.max():.1e}" for k, v in err.items()))


def worst_error(err, rollouts):
    return max((float(v[rollouts].max()) for v in err.values()), default=0.0) if np.any(rollouts) else 0.0


def check_mode1(got, fp32_only, block, tag, beyond_fp32=False):
    """beyond_fp32: the hat's adjoint systems, which the mixed-precision solve finishes in fp64 — see the module docstring"""
    report(tag, got)
    failures = []
    for slot, gb, err in got:
        every = np.ones(len(gb["converged"]), dtype=bool)
        if fp32_only:
            if gb["fp64_iters"].any() or gb["residual_verified"].any():
                failures.append(f"slot {slot}: fp64 stage ran in fp32-only mode")
            if gb["cg_iters"].any():
                failures.append(f"slot {slot}: CG ran in fp32-only mode, cg_iters = {gb['cg_iters'].tolist()}")
            unconv = gb["converged"] == 0
            if beyond_fp32:
                if (gb["adjoint_iters"][unconv] != FP32_BUDGET).any():
                    failures.append(f"slot {slot}: unconverged rollouts stopped before the budget: converged {gb['converged'].tolist()}, "
                                    f"adjoint_iters {gb['adjoint_iters'].tolist()}, cg_iters {gb['cg_iters'].tolist()}, last_udiff {gb['last_udiff'].tolist()}")
                if worst_error(err, ~unconv) > FP32_BEYOND_TOL:
                    failures.append(f"slot {slot}: converged rollouts with gradient error {worst_error(err, ~unconv):.2e} > {FP32_BEYOND_TOL}")
            else:
                if unconv.any():
                    failures.append(f"slot {slot}: unconverged rollouts, converged = {gb['converged'].tolist()}, last_udiff = {gb['last_udiff'].tolist()}")
                if worst_error(err, every) > FP32_ONLY_TOL:
                    failures.append(f"slot {slot}: gradient error {worst_error(err, every):.2e} > {FP32_ONLY_TOL}")
        else:
            if not (gb["converged"] == 1).all() or gb["last_udiff"].max() > 1.01 * REL_TOL:
                failures.append(f"slot {slot}: converged = {gb['converged'].tolist()}, last_udiff = {gb['last_udiff'].tolist()}")
            if block and gb["cg_iters"].any():
                failures.append(f"slot {slot}: CG ran with the block preconditioner, cg_iters = {gb['cg_iters'].tolist()}")
            if not block and not (gb["cg_iters"] > 0).all():
                failures.append(f"slot {slot}: CG-first did not run with diag(P), cg_iters = {gb['cg_iters'].tolist()}")
            if worst_error(err, every) > GRAD_TOL:
                failures.append(f"slot {slot}: gradient error {worst_error(err, every):.2e} > {GRAD_TOL}")
        if not (gb["used_direct"] == 1).all():
            failures.append(f"slot {slot}: used_direct = {gb['used_direct'].tolist()}")
    assert not failures, f"[{tag}] " + "; ".join(failures)


@pytest.mark.parametrize("fp32_only", [0, 1], ids=["mixed", "fp32only"])
@pytest.mark.parametrize("block", [1, 0], ids=["block", "diagP"])
@pytest.mark.parametrize("K", [1, 4], ids=["one-workgroup", "split4"])
def test_direct_adjoint_options_match_oracle(flap, K, block, fp32_only):
    got = run_case(flap, K, adjoint_mode=1, adjoint_block_precond=block, adjoint_fp32_only=fp32_only)
    for slot, gb, err in got:
        assert (gb["workgroups"] == K).all(), (slot, gb["workgroups"])
    check_mode1(got, fp32_only, block, f"flap mode 1 K={K} block={block} fp32_only={fp32_only}")


@pytest.mark.parametrize("K", [1, 4], ids=["one-workgroup", "split4"])
def test_fixed_point_adjoint_matches_oracle(flap, K):
    got = run_case(flap, K, adjoint_mode=0)
    tag = f"flap mode 0 K={K}"
    report(tag, got)
    for slot, gb, err in got:
        assert (gb["workgroups"] == 1).all(), (slot, gb["workgroups"])      # the split adjoint kernel does not implement mode 0: reported
        assert (gb["converged"] != 0).all(), (slot, gb["converged"])
        assert worst_error(err, np.ones(len(gb["converged"]), dtype=bool)) <= GRAD_TOL, (slot, err)


@pytest.mark.parametrize("fp32_only", [0, 1], ids=["mixed", "fp32only"])
@pytest.mark.parametrize("block", [1, 0], ids=["block-coarse", "diagP"])
def test_ill_conditioned_hat_adjoint_matches_oracle(hat, block, fp32_only):
    """block: the COARSE instances (deflation vectors as the coarse level); diag(P): the systems where CG-first stalls and BiCGSTAB has to
    take over"""
    got = run_case(hat, 1, adjoint_mode=1, adjoint_block_precond=block, adjoint_fp32_only=fp32_only)
    check_mode1(got, fp32_only, block, f"hat mode 1 block={block} fp32_only={fp32_only}", beyond_fp32=True)
