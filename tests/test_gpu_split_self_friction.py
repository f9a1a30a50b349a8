"""The split forward kernel's layered self friction (csrc/dc_forward_cl_kernel.h): with its parts on one XCD every part of a rollout walks
the contact layers itself (DC_SELF_REDUNDANT=1, the default) instead of part 0 alone between two cross-part barriers (=0). Both paths
stage the same f / r, run the same contact arithmetic in the same layer order on the same LDS layout and form the right-hand side with
the same expression, so they must agree BITWISE — states, records, iteration and contact counts, and every gradient of the backward
sweep over that tape. A part must not overwrite r of its rows while a peer may still be staging them; the engine's test hook
DC_TEST_SKEW_PART=p makes part p of every rollout start the pass 30 us late (a delay, far below the 2 s spin bound), which turns that
interleaving from a rare event into the common case. dc_get_self_friction_path proves which path each rollout actually took."""
import os

import numpy as np
import pytest

import meshes
from diffcloth_amd import capi, workloads

pytestmark = pytest.mark.gpu
H = 1.0 / 180


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


class env:
    """Environment of the next alloc_batch (build_cluster reads DC_CLUSTER, DC_SELF_REDUNDANT and the test hooks there)."""

    def __init__(self, **kv):
        self.kv = {k: None if v is None else str(v) for k, v in kv.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def sphere_flap_scene():
    """tests/test_gpu_cluster.py::test_split_kernels_with_self_contacts: 40 x 40 cloth over the sphere, a folded flap pressed on with
    twice its weight; four rollouts (shift, mu)."""
    nx, B = 40, 4
    V, F = meshes.grid_cloth(nx, nx, 4.5, 4.5, "DOWN")
    V = f32(V)
    c = f32(meshes.sphere_scene_center(V, 2.0))
    e = capi.Engine(0)
    e.set_mesh(V, F)
    e.set_params(time_step=H, density=0.3, k_stretch=150.0, k_bend=1e-5, forward_tol=1e-8, backward_tol=1e-9, cg_rel_tol=1e-6,
                 cg_max_iter=3000, gradient_clipping=0, selfcollision_enabled=1, adjoint_mode=1, adjoint_rel_tol=1e-8)
    e.set_primitives([dict(kind=capi.DC_PRIM_SPHERE, group=0, center=c, radius=2.0, mu=0.9)])
    e.build()
    V0, flap = meshes.fold_flap(V, nx, nx, 6, 0.05)
    X0 = np.empty((B, V.size)); MU = np.empty((B, 1))
    for b in range(B):
        rng = np.random.default_rng(2000 + b)
        shift = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.09, -0.03), rng.uniform(-0.4, 0.4)])
        X0[b] = f32((f32(V0) + shift).reshape(-1)); MU[b, 0] = rng.uniform(0.1, 0.9)
    field = np.zeros((V.shape[0], 3))
    field[flap, 1] = -2.0 * 9.8 * e.vertex_data()[0][flap]
    return e, dict(K=4, X0=X0, MU=f32(MU), field=f32(field.reshape(-1)))


def c4_scene():
    """The benchmark's rank-share line: the C4 cloth (100 x 100, folded flap pressed with twice its weight) at 32 rollouts, 8 workgroups each,
    with bench.py's solver settings."""
    V, F, V0, flap, center = workloads.c4_scene()
    c = workloads.C4_CLOTH
    e = capi.Engine(0)
    e.set_mesh(V, F)
    e.set_params(time_step=c["h"], density=c["density"], k_stretch=c["k_stretch"], k_bend=c["k_bend"], forward_tol=1e-8, backward_tol=5e-4,
                 cg_rel_tol=1e-4, cg_max_iter=500, gradient_clipping=1, selfcollision_enabled=1, adjoint_mode=1, adjoint_rel_tol=1e-6,
                 adjoint_block_precond=0)
    e.set_primitives([dict(kind=capi.DC_PRIM_SPHERE, group=0, center=center, radius=c["sphere_radius"], mu=c["sphere_mu"])])
    e.build()
    X0, MU = workloads.c4_rollout_inputs(V0, np.arange(32))
    return e, dict(K=8, X0=X0, MU=MU, field=workloads.c4_flap_force(e.vertex_data()[0], flap, 2.0))


S = 10          # fused forward steps (detection inlined on part 0), then one per-step forward (stand-alone detection kernel)


def run(e, sc, redundant, skew=None):
    """Forward sweep of S + 1 steps and the full backward sweep over it; everything the tape and the gradients hold."""
    B = sc["X0"].shape[0]
    with env(DC_CLUSTER=sc["K"], DC_SELF_REDUNDANT=redundant, DC_TEST_SKEW_PART=skew):
        e.alloc_batch(B, S + 2)
    assert e.cluster() == sc["K"]
    e.set_mu(sc["MU"])
    e.set_vertex_forces(np.tile(sc["field"], (B, 1)))
    e.set_state(0, sc["X0"], np.zeros_like(sc["X0"]))
    e.rollout_forward(0, S)
    e.step_forward(S)
    out = {"path": e.self_friction_path()}
    for s in range(S + 2):
        x, v = e.get_state(s)
        out[f"x{s}"], out[f"v{s}"] = x, v
    for s in range(1, S + 2):
        f, r = e.get_record(s)
        out[f"f{s}"], out[f"r{s}"] = f, r
    e.seed_gradient(S + 1, None, 1e-3)
    e.rollout_backward(S + 1, S + 1)
    out["dL_dx"], out["dL_dv"], out["dL_dmu"] = e.get_gradient()
    for s in range(1, S + 2):
        fwd, bwd = e.get_stats(s)
        for k in ("converged", "pd_iters", "cg_iters", "prim_contacts", "self_contacts", "last_xdiff"):
            out[f"fwd_{k}{s}"] = np.asarray(fwd[k])
        for k in ("converged", "adjoint_iters", "cg_iters", "last_udiff", "workgroups"):
            out[f"bwd_{k}{s}"] = np.asarray(bwd[k])
        pg = e.get_param_gradients(s)
        out[f"dL_dk{s}"], out[f"dL_ddensity{s}"] = pg["dL_dk"], pg["dL_ddensity"]
    return out


def compare(ref, got, tag):
    """names of the outputs that differ, with the largest difference of each (for the message)"""
    bad = []
    for k in ref:
        if k == "path":
            continue
        a, b = np.asarray(ref[k]), np.asarray(got[k])
        if not np.array_equal(a, b):
            d = np.abs(a.astype(np.float64) - b.astype(np.float64))
            bad.append(f"{k} (max |diff| {np.nanmax(d):.3e})")
    print(f"\n[{tag}] {len(ref) - 1 - len(bad)} of {len(ref) - 1} outputs bitwise equal" + (": differ " + ", ".join(bad[:12]) if bad else ""))
    return bad


def check_scene(e, sc, name):
    K = sc["K"]
    ref = run(e, sc, 0)
    p0 = ref["path"]
    nself = np.stack([ref[f"fwd_self_contacts{s}"] for s in range(1, S + 2)])
    print(f"\n[{name}] K={K}, B={sc['X0'].shape[0]}: self contacts per step {int(nself.min())} ... {int(nself.max())}, "
          f"PD iterations with a self-friction pass per rollout {p0[:, 0].tolist()}")
    assert nself.min() > 50
    assert (p0[:, 0] > 0).all() and (p0[:, 1] == 0).all()          # part 0 alone
    assert np.all(np.isin(np.stack([ref[f"fwd_converged{s}"] for s in range(1, S + 2)]), (1, 2)))
    failures = {}
    for skew in (None, K // 2, K - 1):
        tag = f"{name} redundant, skew part {skew}"
        got = run(e, sc, 1, skew)
        p1 = got["path"]
        # every rollout took the redundant path in every PD iteration with self contacts (no fall-back to part 0 alone)
        assert (p1[:, 1] == p1[:, 0]).all() and (p1[:, 0] > 0).all(), (tag, p1.tolist())
        bad = compare(ref, got, tag)
        if bad:
            failures[tag] = bad
    assert not failures, failures


def test_redundant_self_friction_is_bitwise_the_part0_path_sphere_flap():
    e, sc = sphere_flap_scene()
    try:
        check_scene(e, sc, "sphere + pressed flap")
    finally:
        e.close()


def test_redundant_self_friction_is_bitwise_the_part0_path_c4_rank_share():
    e, sc = c4_scene()
    try:
        check_scene(e, sc, "C4 32 x 8")
    finally:
        e.close()
