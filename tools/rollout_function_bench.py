"""Measures what the whole-episode torch function (diffcloth_amd.functional.sim_rollout) costs next to the host-schedule evaluation it
replaces, on the headline workload: bench.py's C4 definition (diffcloth_amd/workloads.py) with bench.py's solver settings, B = 256
rollouts, T = 20 steps, loss = mean squared distance of every state to the rest shape.

In ONE process, after warming both paths, the two are alternated `--reps` times, each evaluation ending in a device synchronise:
  (a) host schedules: numpy in, numpy out — dc_set_state, dc_rollout_forward, dc_get_states, the loss gradient in numpy,
      dc_set_seed_schedule + dc_set_gradient, dc_rollout_backward, dc_get_gradient;
  (b) sim_rollout on CUDA fp32 tensors, loss and backward in torch.
Reported: median and spread of the wall time per evaluation, the kernel time of (a) from dc_kernel_times, the boundary cost of (b) =
(b) - that kernel time, and the bytes (a) moves over PCIe (computed from the shapes).

The same run times the multi-slot layout conversion (ONE launch per array for all T slots) against T launches of the per-slot kernels
(dc_get_state_dev / dc_set_state_dev), for fp32 and fp64 tensors, with device events around each of `--conv-reps` repetitions, and
reports achieved GB/s (bytes read + bytes written) and the share of the HBM peak.

    python tools/rollout_function_bench.py [--batch 256] [--steps 20] [--grid 100] [--reps 5] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffcloth_amd import capi, workloads                       # noqa: E402
from diffcloth_amd.functional import BatchedSim, sim_rollout    # noqa: E402

HBM_PEAK_GBS = 8000.0       # MI355X: 8 TB/s


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return f"median {np.median(v):9.3f}  min {v.min():9.3f}  max {v.max():9.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--grid", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--conv-reps", dest="conv_reps", type=int, default=20)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rollout_function_bench.py needs a HIP device")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    B, T = args.batch, args.steps
    dev = torch.device("cuda", 0)
    V, F, V0, flap, center = workloads.c4_scene(args.grid, 5, 0.02)
    e = capi.Engine(0)
    e.set_mesh(V, F)
    c4 = workloads.C4_CLOTH           # bench.py: make_engine and its argument defaults
    e.set_params(time_step=c4["h"], density=c4["density"], k_stretch=c4["k_stretch"], k_bend=c4["k_bend"], forward_tol=1e-8, backward_tol=5e-4,
                 cg_rel_tol=1e-4, cg_max_iter=500, gradient_clipping=1, selfcollision_enabled=1, adjoint_mode=1, adjoint_rel_tol=1e-6,
                 adjoint_block_precond=0)
    e.set_primitives([dict(kind=capi.DC_PRIM_SPHERE, group=0, center=center, radius=c4["sphere_radius"], mu=c4["sphere_mu"])])
    e.build()
    N = e.N
    e.alloc_batch(B, T)
    X0, MU = workloads.c4_rollout_inputs(V0, np.arange(B))
    V00 = np.zeros_like(X0)
    field = np.tile(workloads.c4_flap_force(e.vertex_data()[0], flap, 2.0), (B, 1))
    target = V.reshape(-1)
    scale = 1.0 / (T * N)
    say(f"# rollout_function_bench: C4 grid {args.grid} (N = {N}), B = {B}, T = {T}, workgroups per rollout {e.cluster()}, {torch.cuda.get_device_name(0)}")

    side = torch.cuda.Stream(device=dev)      # the engine and torch on ONE explicit stream: device events bracket the engine's launches
    with torch.cuda.stream(side):
        sim = BatchedSim(e, T)
        sim.on_current_stream(dev)
        tx0 = torch.as_tensor(X0, dtype=torch.float32).to(dev)
        tv0 = torch.zeros_like(tx0)
        tmu = torch.as_tensor(MU, dtype=torch.float32).to(dev)
        tfield = torch.as_tensor(field, dtype=torch.float32).to(dev)
        ttarget = torch.as_tensor(target, dtype=torch.float32).to(dev)

        def eval_host():
            e.kernel_times(reset=True)
            e.set_trajectory_start(0); e.clear_schedules()
            e.set_mu(MU); e.set_vertex_forces(field)
            e.set_state(0, X0, V00)
            e.rollout_forward(0, T)
            xs, _ = e.get_states(1, T)
            d = xs - target
            loss = float(np.sum(d * d) * scale)
            g = (2.0 * scale) * d
            e.set_seed_schedule(0, np.concatenate([np.zeros((1, B, 3 * N)), g[:T - 1]]))
            e.set_gradient(g[T - 1], V00)
            e.rollout_backward(T, T)
            dx, dv, dmu = e.get_gradient()
            e.sync(); torch.cuda.synchronize()
            kt = e.kernel_times()
            return loss, dx, dmu, kt["fwd_ms"] + kt["bwd_ms"]

        def eval_torch():
            x0 = tx0.clone().requires_grad_(); v0 = tv0.clone().requires_grad_(); mu = tmu.clone().requires_grad_()
            xs, vs = sim_rollout(sim, x0, v0, steps=T, vertex_forces=tfield, mu=mu)
            loss = ((xs - ttarget) ** 2).sum() * scale
            loss.backward()
            torch.cuda.synchronize()
            return float(loss.detach()), x0.grad, mu.grad

        # warm both paths (allocations of the seed schedule, torch's caching allocator, code objects)
        la, dxa, dmua, _ = eval_host()
        lb, dxb, dmub = eval_torch()
        dxb, dmub = dxb.cpu().numpy().astype(np.float64), dmub.cpu().numpy().astype(np.float64)
        say(f"agreement of the two paths: loss (a) {la:.9e} (b) {lb:.9e}; |dL_dx0 (b) - (a)| / |(a)| = {np.linalg.norm(dxb - dxa) / max(np.linalg.norm(dxa), 1e-300):.2e}; "
            f"|dL_dmu (b) - (a)| / |(a)| = {np.linalg.norm(dmub - dmua) / max(np.linalg.norm(dmua), 1e-300):.2e}")
        del dxa, dxb
        wa, wb, ka = [], [], []
        for _ in range(args.reps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            out = eval_host()
            wa.append((time.perf_counter() - t0) * 1e3); ka.append(out[3])
            del out
            torch.cuda.synchronize(); t0 = time.perf_counter()
            eval_torch()
            wb.append((time.perf_counter() - t0) * 1e3)
        se = B * 3 * N * 8
        pcie = 2 * se + 2 * T * se + T * se + 2 * se + 2 * se
        say(f"wall time per evaluation, ms, {args.reps} alternating repetitions:")
        say(f"  (a) host schedules, numpy in / numpy out : {stats(wa)}")
        say(f"  (b) sim_rollout, CUDA fp32 tensors       : {stats(wb)}")
        say(f"  kernel time of (a), dc_kernel_times       : {stats(ka)}")
        say(f"  boundary cost of (b) = (b) - kernel time  : {np.median(wb) - np.median(ka):9.3f}  (medians)")
        say(f"  (b) faster than (a): {bool(np.median(wb) < np.median(wa))}  ((a) / (b) = {np.median(wa) / np.median(wb):.2f}); rollout-steps/s (a) {B * T / np.median(wa) * 1e3:.0f} (b) {B * T / np.median(wb) * 1e3:.0f}")
        say(f"  bytes (a) moves over PCIe per evaluation, from the shapes: {pcie / 1e9:.3f} GB (state in {2 * se / 1e9:.3f}, states out {2 * T * se / 1e9:.3f}, "
            f"seeds in {T * se / 1e9:.3f}, carried gradient in {2 * se / 1e9:.3f}, gradient out {2 * se / 1e9:.3f})")

        # ---- layout conversion: one multi-slot launch per array against T per-slot launches, x and v of T slots each
        say()
        say(f"layout conversion of 2 arrays x {T} slots x [{B}][{3 * N}], device events, {args.conv_reps} repetitions, ms and GB/s (read + written):")
        elems = 2 * T * B * 3 * N

        def timed(fn):
            ms = []
            fn(); torch.cuda.synchronize()
            for _ in range(args.conv_reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(side); fn(); b.record(side)
                b.synchronize()
                ms.append(a.elapsed_time(b))
            return np.asarray(ms)

        for dtype, name in ((torch.float32, "fp32"), (torch.float64, "fp64")):
            nbytes = elems * (4 + (4 if dtype == torch.float32 else 8))
            xs = torch.empty((T, B, 3 * N), dtype=dtype, device=dev); vs = torch.empty_like(xs)
            cases = (("tape -> tensors, multi-slot (dc_get_states_dev)      ", lambda: e.get_states_dev(1, T, xs, vs)),
                     ("tape -> tensors, per slot   (dc_get_state_dev x T)   ", lambda: [e.get_state_dev(1 + k, xs[k], vs[k]) for k in range(T)]),
                     ("tensors -> tape, multi-slot (dc_set_seed_schedule_dev)", lambda: e.set_seed_schedule_dev(0, T, xs, vs)),
                     ("tensors -> tape, per slot   (dc_set_state_dev x T)   ", lambda: [e.set_state_dev(1 + k, xs[k], vs[k]) for k in range(T)]))
            for label, fn in cases:
                ms = timed(fn)
                gbs = nbytes / np.median(ms) / 1e6
                say(f"  {name} {label}: {stats(ms)}  -> {gbs:8.1f} GB/s = {100 * gbs / HBM_PEAK_GBS:5.1f} % of the {HBM_PEAK_GBS / 1000:.0f} TB/s HBM peak")
            del xs, vs
        e.sync()
    torch.cuda.synchronize()
    e.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
