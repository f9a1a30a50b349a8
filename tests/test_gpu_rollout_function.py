"""diffcloth_amd.functional.sim_rollout: a whole episode as one torch.autograd.Function over the fused sweeps, with CUDA tensors crossing
the C-ABI as device pointers (dc_rollout_*_async, dc_set_*_schedule_dev, dc_get_*_dev; kernels in csrc/dc_boundary.hip).

The comparison partner is the same function on CPU tensors, which takes the host calls of the engine. Every input is rounded to fp32
first, so both paths hand identical planar fp32 values to identical launches. Scene and settings are those of
tests/test_gpu_schedules.py. Two shapes cover the paths of the boundary kernels: N = 289 (odd: unaligned planes, one vertex per lane,
one workgroup per rollout) and N = 2 304 split over 4 workgroups per rollout (4 vertices per lane, 16-byte accesses).

Measured on an MI355X (printed by the tests): see docs/HISTORY.md, "Differentiable whole-episode rollouts".
"""
import numpy as np
import pytest
import torch          # before the engine's library: both must share ONE HIP runtime (torch's), see tests/test_gpu_functional.py

import meshes
from diffcloth_amd import capi
from diffcloth_amd.functional import BatchedSim, sim_rollout

pytestmark = pytest.mark.gpu

NAMES = ("x0", "v0", "actions", "uniform_force", "vertex_force_scale", "vertex_forces", "mu")
T = 5


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def rel(a, b):
    return np.linalg.norm(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) / max(np.linalg.norm(b), 1e-30)


def scene(nx, att):
    V, F = meshes.grid_cloth(nx, nx, 4.5, 4.5, "DOWN")
    V = f32(V)
    c = f32(meshes.sphere_scene_center(V, 2.0))
    e = capi.Engine(0)
    e.set_mesh(V, F)
    e.set_attachments(att)
    e.set_params(time_step=1 / 180, density=0.3, k_stretch=150.0, k_bend=0.05, forward_tol=1e-7, backward_tol=1e-7, cg_rel_tol=1e-5,
                 cg_max_iter=2000, gradient_clipping=0, selfcollision_enabled=0, adjoint_mode=1, adjoint_rel_tol=1e-7)
    e.set_primitives([dict(kind=capi.DC_PRIM_SPHERE, group=0, center=c, radius=2.0, mu=0.4)])
    e.build()
    return V, F, e


def make_inputs(V, att, B, rng, mu0=None):
    """the seven inputs of an episode and the loss weights, all exact in fp32 (float64 arrays holding fp32 values)"""
    N = V.shape[0]
    top = V[list(att)]
    inp = dict(
        x0=np.stack([f32(V.reshape(-1) + np.tile([0.05 * b, 0.0, 0.02 * b], N)) for b in range(B)]),
        v0=np.zeros((B, 3 * N)),
        actions=np.stack([np.stack([f32((top + np.array([0.01 * (s + 1) * (b + 1), 0.02 * (s + 1), 0.0])).reshape(-1)) for b in range(B)]) for s in range(T)]),
        uniform_force=f32(0.02 * rng.standard_normal((T, B, 3))),
        vertex_force_scale=np.array([[0.5, 1.0, 0.25, 2.0][(s + b) % 4] for s in range(T) for b in range(B)], dtype=np.float64).reshape(T, B),   # powers of two
        vertex_forces=f32(0.001 * rng.standard_normal((B, 3 * N))),
        mu=f32(np.full((B, 1), 0.4) if mu0 is not None else 0.4 + 0.05 * np.arange(B).reshape(B, 1)))
    wx = f32(1e-3 * rng.standard_normal((T, B, 3 * N)))
    wv = f32(1e-5 * rng.standard_normal((T, B, 3 * N)))
    return inp, wx, wv


def leaf(a, device, dtype, unaligned=False):
    """a leaf tensor holding `a`; unaligned: a contiguous view that starts one element into a larger buffer"""
    t = torch.as_tensor(np.ascontiguousarray(a), dtype=dtype)
    if unaligned:
        buf = torch.empty(t.numel() + 1, dtype=dtype, device=device)
        buf[1:].copy_(t.reshape(-1))
        t = buf[1:].view(t.shape)
        assert t.is_contiguous() and t.data_ptr() % 16 != 0
    else:
        t = t.to(device)
    return t.detach().requires_grad_()


def run(sim, inp, wx, wv, device, dtype=torch.float32, backward=True, unaligned=(), after=None):
    """one evaluation through sim_rollout; returns numpy arrays: xs, vs and the gradient of sum(wx xs) + sum(wv vs) w.r.t. every input"""
    ts = {k: leaf(inp[k], device, dtype, k in unaligned) for k in NAMES}
    xs, vs = sim_rollout(sim, ts["x0"], ts["v0"], ts["actions"], uniform_force=ts["uniform_force"], vertex_force_scale=ts["vertex_force_scale"],
                         vertex_forces=ts["vertex_forces"], mu=ts["mu"])
    out = dict(xs=xs.detach().cpu().numpy(), vs=vs.detach().cpu().numpy())
    if backward:
        w = lambda a: torch.as_tensor(a, dtype=dtype).to(device)
        loss = (xs * w(wx)).sum() + (vs * w(wv)).sum()
        loss.backward()
        for k in NAMES:
            out["d_" + k] = ts[k].grad.detach().cpu().numpy()
        if after is not None:
            out.update(after(sim.engine))
    return out


def kept_tape(e):
    """what the last backward sweep left readable on the host: the per-slot parameter gradients and h^2 y of every step"""
    return dict(sum_dfext=np.stack([e.get_param_gradients(s)["sum_dfext"] for s in range(1, T + 1)]), h2y=e.get_force_gradients(1, T))


@pytest.fixture(scope="module", params=[(17, 0, 3), (48, 4, 2)], ids=["nx17", "nx48-split4"])
def episode(request):
    """engine, inputs, and ONE evaluation on each path, shared by the tests below"""
    nx, cluster, B = request.param
    att = (0, nx - 1)
    with pytest.MonkeyPatch.context() as mp:
        if cluster:
            mp.setenv("DC_CLUSTER", str(cluster))
        V, F, e = scene(nx, att)
        e.alloc_batch(B, T)
    assert e.cluster() == (cluster if cluster else 1)
    sim = BatchedSim(e, T)
    inp, wx, wv = make_inputs(V, att, B, np.random.default_rng(5))
    host = run(sim, inp, wx, wv, "cpu")
    dev = run(sim, inp, wx, wv, "cuda", after=kept_tape)
    yield dict(nx=nx, B=B, N=V.shape[0], e=e, sim=sim, inp=inp, wx=wx, wv=wv, host=host, dev=dev)
    e.close()


def test_device_path_equals_host_path_forward(episode):
    h, d = episode["host"], episode["dev"]
    assert d["xs"].dtype == np.float32 and d["xs"].shape == (T, episode["B"], 3 * episode["N"])
    assert np.abs(d["xs"][-1] - episode["inp"]["x0"]).max() > 1e-3           # the cloth moved
    np.testing.assert_array_equal(d["xs"], h["xs"])
    np.testing.assert_array_equal(d["vs"], h["vs"])


def test_device_path_equals_host_path_backward(episode):
    h, d, inp = episode["host"], episode["dev"], episode["inp"]
    bits = {k: bool(np.array_equal(d["d_" + k], h["d_" + k])) for k in NAMES}
    print(f"\n[rollout function nx={episode['nx']}] device vs host path: " + " ".join(f"d_{k} {rel(d['d_' + k], h['d_' + k]):.2e}" for k in NAMES) +
          f"; bit-equal: {bits}")
    for k in ("x0", "v0", "actions"):
        assert np.abs(h["d_" + k]).max() > 0
        assert rel(d["d_" + k], h["d_" + k]) <= 2e-6, k
    np.testing.assert_allclose(d["d_mu"], h["d_mu"], rtol=1e-4, atol=1e-9)
    # uniform force: a copy of the per-slot parameter gradients of the same sweep
    np.testing.assert_array_equal(d["d_uniform_force"], d["sum_dfext"].astype(np.float32))
    assert np.abs(d["d_uniform_force"]).max() > 0
    # the two reductions over the kept y tape, against numpy in fp64 on the same data: one fp32 rounding of an fp64-accumulated sum of at
    # most 2^17 terms, |dev - host| <= 2^-23 |host| + 2^-36 sum |terms|
    h2y, fv, w = d["h2y"], inp["vertex_forces"], inp["vertex_force_scale"]
    assert h2y.shape[2] * T < 2 ** 17
    ref_s = np.einsum("kbq,bq->kb", h2y, fv); mag_s = np.einsum("kbq,bq->kb", np.abs(h2y), np.abs(fv))
    ref_f = np.einsum("kb,kbq->bq", w, h2y); mag_f = np.einsum("kb,kbq->bq", np.abs(w), np.abs(h2y))
    for name, got, ref, mag in (("vertex_force_scale", d["d_vertex_force_scale"], ref_s, mag_s), ("vertex_forces", d["d_vertex_forces"], ref_f, mag_f)):
        err, bound = np.abs(got.astype(np.float64) - ref), 2.0 ** -23 * np.abs(ref) + 2.0 ** -36 * mag
        print(f"[rollout function nx={episode['nx']}] d_{name}: max |dev - fp64 numpy| / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}, max |ref| {np.abs(ref).max():.3e}")
        assert np.abs(ref).max() > 0
        assert np.all(err <= bound), name


def test_fp64_tensors_and_unaligned_views(episode):
    sim, inp, wx, wv, d = episode["sim"], episode["inp"], episode["wx"], episode["wv"], episode["dev"]
    d64 = run(sim, inp, wx, wv, "cuda", dtype=torch.float64, backward=False)
    assert d64["xs"].dtype == np.float64
    np.testing.assert_array_equal(d64["xs"], d["xs"].astype(np.float64))
    np.testing.assert_array_equal(d64["vs"], d["vs"].astype(np.float64))
    for dtype in (torch.float32, torch.float64):
        u = run(sim, inp, wx, wv, "cuda", dtype=dtype, backward=False, unaligned=("actions", "x0"))
        np.testing.assert_array_equal(u["xs"], d["xs"])
        np.testing.assert_array_equal(u["vs"], d["vs"])
    sim.check_episode()


def test_stream_ordering_and_repeated_episodes(episode):
    sim, inp, wx, wv, d = episode["sim"], episode["inp"], episode["wx"], episode["wv"], episode["dev"]
    dev = torch.device("cuda", 0)
    ts = {k: torch.as_tensor(inp[k], dtype=torch.float32).to(dev) for k in NAMES}
    half = ts["actions"] * 0.5                       # exact in fp32
    ref_sum = torch.as_tensor(d["xs"]).to(dev).sum(dim=(1, 2))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        actions = half + half                        # produced by a torch kernel enqueued immediately before the call ...
        xs, vs = sim_rollout(sim, ts["x0"], ts["v0"], actions, uniform_force=ts["uniform_force"], vertex_force_scale=ts["vertex_force_scale"],
                             vertex_forces=ts["vertex_forces"], mu=ts["mu"])
        total = xs.sum(dim=(1, 2))                   # ... and consumed by one immediately after it: no synchronisation in between
    side.synchronize()
    np.testing.assert_array_equal(xs.cpu().numpy(), d["xs"])
    np.testing.assert_array_equal(vs.cpu().numpy(), d["vs"])
    np.testing.assert_array_equal(total.cpu().numpy(), ref_sum.cpu().numpy())
    sim.check_episode()
    # two consecutive episodes on the same BatchedSim (back on torch's default stream): reset, sim_rollout, twice
    runs = []
    for _ in range(2):
        sim.reset(inp["x0"], inp["v0"])
        runs.append(run(sim, inp, wx, wv, "cuda"))
    for k in runs[0]:
        np.testing.assert_array_equal(runs[0][k], runs[1][k], err_msg=k)
        np.testing.assert_array_equal(runs[0][k], d[k], err_msg=k)


def test_device_path_equals_per_step_calls():
    """loop (a) of tests/test_gpu_schedules.py::test_scheduled_rollout_equals_per_step_calls — every value handed to its step as an argument,
    the seeds as dL_dxinit — against sim_rollout on CUDA tensors with the same seeds as the loss weights"""
    nx, B = 17, 2
    att = (0, nx - 1)
    V, F, e = scene(nx, att)
    N = V.shape[0]
    e.alloc_batch(B, T)
    inp, wx, _ = make_inputs(V, att, B, np.random.default_rng(7), mu0=0.4)        # mu = the primitive's own 0.4: the per-step calls use the default
    XF, FU, FV, FVS = inp["actions"], inp["uniform_force"], inp["vertex_forces"], inp["vertex_force_scale"]
    seeds = np.concatenate([np.zeros((1, B, 3 * N)), wx])                          # loss gradient w.r.t. the state of every slot; slot 0: none
    zero = np.zeros((B, 3 * N))
    e.set_state(0, inp["x0"], inp["v0"])
    for s in range(T):
        e.set_uniform_force(FU[s])
        e.set_vertex_forces(FV * FVS[s][:, None])
        e.step_forward(s, fixed_pts=XF[s])
    xa, va = e.get_states(1, T)
    gx, gv = seeds[T].copy(), zero
    dxf_a, dmu_a = {}, np.zeros((B, 1))
    for s in range(T, 0, -1):
        out = e.step_backward(s, gx, gv, dL_dxinit=seeds[s - 1], dL_dvinit=zero, is_start=(s == 1))
        gx, gv = out["dL_dx"], out["dL_dv"]
        dxf_a[s] = out["dL_dxfixed"].copy(); dmu_a += out["dL_dmu"]
    e.set_uniform_force(None)
    d = run(BatchedSim(e, T), inp, wx, np.zeros_like(wx), "cuda")
    np.testing.assert_array_equal(d["xs"], xa)
    np.testing.assert_array_equal(d["vs"], va)
    e_f = max(rel(d["d_actions"][s - 1], dxf_a[s]) for s in range(1, T + 1))
    print(f"\n[rollout function nx={nx}] sim_rollout vs per-step calls: dL_dx0 {rel(d['d_x0'], gx):.2e} dL_dv0 {rel(d['d_v0'], gv):.2e} dL_dxfixed {e_f:.2e} "
          f"dL_dmu {rel(d['d_mu'], dmu_a):.2e}")
    assert rel(d["d_x0"], gx) <= 2e-6 and rel(d["d_v0"], gv) <= 2e-6 and e_f <= 2e-6
    np.testing.assert_allclose(d["d_mu"], dmu_a, rtol=1e-4, atol=1e-9)
    e.close()


def test_errors_on_the_device_are_host_side_refusals():
    nx, B = 17, 2
    att = (0, nx - 1)
    V, F, e = scene(nx, att)
    e.alloc_batch(B, T)
    sim = BatchedSim(e, T)
    inp, wx, wv = make_inputs(V, att, B, np.random.default_rng(9))
    ref = run(sim, inp, wx, wv, "cuda", backward=False)
    dev = torch.device("cuda", 0)

    def still_correct():
        again = run(sim, inp, wx, wv, "cuda", backward=False)
        np.testing.assert_array_equal(again["xs"], ref["xs"]); np.testing.assert_array_equal(again["vs"], ref["vs"])
        sim.check_episode()

    # an episode longer than the tape: refused before anything is enqueued
    z = lambda *s: torch.zeros(s, device=dev)
    with pytest.raises((RuntimeError, ValueError), match="tape"):
        sim_rollout(sim, z(B, 3 * e.N), z(B, 3 * e.N), z(T + 1, B, 3 * e.Af))
    still_correct()
    # a force schedule on 2 of 5 steps, set through the raw setter: the fused sweep refuses the partial schedule
    e.clear_schedules()
    e.set_force_schedule_dev(0, 2, fu=torch.as_tensor(inp["uniform_force"][:2], dtype=torch.float32).to(dev))
    with pytest.raises(capi.DcError, match="covers only part"):
        e.rollout_forward_async(0, T)
    still_correct()
    # the reductions over the y tape need it kept: no backward sweep of this batch has kept it
    out = torch.zeros(T, B, device=dev)
    with pytest.raises(capi.DcError, match="keep_force_gradients"):
        e.get_force_schedule_gradients_dev(1, T, dfv_scale=out)
    assert float(out.abs().max()) == 0.0
    still_correct()
    e.close()


@pytest.mark.parametrize("renumber", [0, 1])
@pytest.mark.parametrize("nx", [7, 8])
def test_conversion_kernels_round_trip(nx, renumber, monkeypatch):
    """the layout kernels alone, with and without the device renumbering, N = 49 (one vertex per lane) and N = 64 (four), fp32 and fp64,
    aligned tensors and views one element into a buffer: what goes in through dc_set_gradient_dev comes back through dc_get_gradient_dev,
    and several slots written by the host calls come back from ONE dc_get_states_dev as the host's dc_get_states returns them"""
    monkeypatch.setenv("DC_RENUMBER", str(renumber))
    V, F, e = scene(nx, (0, nx - 1))
    B, S, N = 3, 2, V.shape[0]
    e.alloc_batch(B, S)
    rng = np.random.default_rng(nx)
    a, b = f32(rng.standard_normal((B, 3 * N))), f32(rng.standard_normal((B, 3 * N)))
    states = f32(rng.standard_normal((S + 1, 2, B, 3 * N)))
    for s in range(S + 1):
        e.set_state(s, states[s, 0], states[s, 1])
    hx, hv = e.get_states(0, S + 1)
    np.testing.assert_array_equal(hx, states[:, 0])
    for dtype in (torch.float32, torch.float64):
        for unaligned in (False, True):
            ta, tb = leaf(a, "cuda", dtype, unaligned).detach(), leaf(b, "cuda", dtype, unaligned).detach()
            oa, ob = leaf(0 * a, "cuda", dtype, unaligned).detach(), leaf(0 * b, "cuda", dtype, unaligned).detach()
            e.set_gradient_dev(ta, tb)
            e.get_gradient_dev(oa, ob)
            xs, vs = leaf(np.zeros((S + 1, B, 3 * N)), "cuda", dtype, unaligned).detach(), leaf(np.zeros((S + 1, B, 3 * N)), "cuda", dtype, unaligned).detach()
            e.get_states_dev(0, S + 1, xs, vs)
            e.sync(); torch.cuda.synchronize()
            np.testing.assert_array_equal(oa.cpu().numpy(), a); np.testing.assert_array_equal(ob.cpu().numpy(), b)
            np.testing.assert_array_equal(xs.cpu().numpy(), hx); np.testing.assert_array_equal(vs.cpu().numpy(), hv)
    e.close()
