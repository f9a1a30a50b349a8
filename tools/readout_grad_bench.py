"""Measures what the contact read-out's adjoint (dc_set_contact_readout_gradients) costs in the backward sweep of the headline workload:
bench.py's C4 definition (diffcloth_amd/workloads.py) with bench.py's solver settings, B = 256 rollouts, T = 20 steps.

ONE process, one forward sweep, then the backward sweep over the same tape is repeated `--reps` times in each of three forms, ALTERNATING
(plain, zero, seeded, plain, ...) after one warm-up of each, so that clock and thermal drift fall on both alike:
  plain   no weights set: the sweep as it was (and, checked here by launch count, not one kernel more)
  zero    all-zero weights on every step: both passes run in full, the seeds they add are zeros, so the adjoint solves are the plain
          sweep's — zero - plain is the cost of the two passes alone
  seeded  random weights on jn and on the wrench of EVERY step: the seed pass before the step kernels, the parameter pass after them
Every sweep starts from the same carried gradient and seed schedule. Reported per form: median, min and max of the sweep's device time
(dc_kernel_times: HIP events around everything the sweep enqueues, the two passes included) and of its wall time, the launch counts, and the
differences of the medians to the plain sweep. The two passes' own kernel times: the same tool under a kernel trace
(`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/readout_grad_bench.py --reps 3`, rows k_readout_adjoint<0> and <1>).

    python tools/readout_grad_bench.py [--batch 256] [--steps 20] [--grid 100] [--reps 7] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch          # before the engine's library: one HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffcloth_amd import capi, workloads                       # noqa: E402


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return f"median {np.median(v):9.3f}  min {v.min():9.3f}  max {v.max():9.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--grid", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("readout_grad_bench.py needs a HIP device")
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
    field = np.tile(workloads.c4_flap_force(e.vertex_data()[0], flap, 2.0), (B, 1))
    say(f"# readout_grad_bench: C4 grid {args.grid} (N = {N}), B = {B}, T = {T}, workgroups per rollout {e.cluster()}, {torch.cuda.get_device_name(0)}")
    e.set_trajectory_start(0); e.clear_schedules()
    e.set_mu(MU); e.set_vertex_forces(field)
    e.set_state(0, X0, np.zeros_like(X0))
    e.rollout_forward(0, T)
    ro = e.contact_readout(1, T, state=False, normal_impulse=False)["wrench"]
    say(f"contacts per step and rollout (take-off + stick + slide): mean {ro[..., 7:10].sum(axis=-1).mean():.1f}, max {ro[..., 7:10].sum(axis=-1).max():.0f}")

    g = torch.Generator(device="cpu").manual_seed(5)
    scale = 1.0 / (T * N)
    seeds_x = (torch.randn((T, B, 3 * N), generator=g) * scale).to(dev)
    seeds_v = torch.zeros_like(seeds_x)
    wj = torch.randn((T, B, N), generator=g).to(dev) * scale
    ww = torch.randn((T, B, e.ngroups, 10), generator=g).to(dev) * scale
    e.set_seed_schedule_dev(0, T, seeds_x, seeds_v)
    top_x, top_v = seeds_x[T - 1].contiguous(), seeds_v[T - 1].contiguous()

    zj, zw = torch.zeros_like(wj), torch.zeros_like(ww)

    def sweep(form):
        if form == "seeded":
            e.set_contact_readout_gradients_dev(1, T, wj, ww)
        elif form == "zero":
            e.set_contact_readout_gradients_dev(1, T, zj, zw)
        else:
            e.set_contact_readout_gradients_dev(1, T, None, None)
        e.set_gradient_dev(top_x, top_v)
        e.sync(); torch.cuda.synchronize()
        e.kernel_times(reset=True)
        t0 = time.perf_counter()
        e.rollout_backward(T, T)
        wall = (time.perf_counter() - t0) * 1e3
        kt = e.kernel_times()
        return kt["bwd_ms"], wall, kt["bwd_launches"]

    forms = ("plain", "zero", "seeded")
    for form in forms:          # warm-up of every form (the setter has allocated what the passes need)
        sweep(form)
    res = {form: [] for form in forms}
    for _ in range(args.reps):
        for form in forms:
            res[form].append(sweep(form))
    for form in forms:
        dev_ms, wall, launches = (np.asarray(v) for v in zip(*res[form]))
        say(f"{form:6s}: device time of the sweep, ms: {stats(dev_ms)}   wall, ms: {stats(wall)}   launches {sorted(set(launches.tolist()))}")
    med = {form: np.median([r[0] for r in res[form]]) for form in forms}
    for form, what in (("zero", "the two passes alone"), ("seeded", "the passes and what the seeds change in the adjoint solves")):
        d = med[form] - med["plain"]
        say(f"{form} - plain (medians): {d:9.3f} ms = {100 * d / med['plain']:6.2f} % of the plain sweep, {1e3 * d / (B * T):8.3f} us per rollout-step ({what})")
    n0 = {r[2] for r in res["plain"]}
    assert len(n0) == 1 and {r[2] for r in res["seeded"]} == {min(n0) + 2}, "launch counts: the plain sweep must enqueue no kernel of the read-out's"
    e.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
