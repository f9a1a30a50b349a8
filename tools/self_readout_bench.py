"""Measures the self-contact read-out (dc_get_self_contact_readout_dev) on the records of the headline workload: bench.py's C4 definition
(diffcloth_amd/workloads.py) with bench.py's solver settings, B = 256 rollouts, T = 20 steps.

ONE process, one forward sweep, then the read-out of all T records into device tensors is repeated `--reps` times after a warm-up (which also
makes the first call's allocation), timed with events on the context's stream; reported: the records' contact counts from the totals, the
median / min / max time of a whole read-out, in fp32 with every output and with the totals alone. With N = 10 000 the context's largest
possible record does not fit one workgroup's LDS (dc_self_readout.h), so the range is T launches of B workgroups, not one. The kernel's own
time per launch: the same tool under a kernel trace
(`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/self_readout_bench.py --reps 3`, row k_self_readout).

    python tools/self_readout_bench.py [--batch 256] [--steps 20] [--grid 100] [--cap 1024] [--reps 7]
"""
import argparse
import os
import sys

import numpy as np
import torch          # before the engine's library: one HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffcloth_amd import capi, workloads                       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--grid", type=int, default=100)
    ap.add_argument("--cap", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("self_readout_bench.py needs a HIP device")
    B, T, cap = args.batch, args.steps, args.cap
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
    print(f"# self_readout_bench: C4 grid {args.grid} (N = {N}), B = {B}, T = {T}, list capacity {e.max_self_contacts}, cap {cap}, {torch.cuda.get_device_name(0)}", flush=True)
    e.set_trajectory_start(0); e.clear_schedules()
    e.set_mu(MU); e.set_vertex_forces(field)
    e.set_state(0, X0, np.zeros_like(X0))
    e.rollout_forward(0, T)
    e.sync()
    pairs = torch.empty((T, B, cap, 4), dtype=torch.int32, device=dev)
    imp = torch.empty((T, B, cap, 4), dtype=torch.float32, device=dev)
    vimp = torch.empty((T, B, N, 3), dtype=torch.float32, device=dev)
    tot = torch.empty((T, B, 8), dtype=torch.float32, device=dev)
    forms = (("every output", (pairs, imp, vimp, tot)), ("totals alone", (None, None, None, tot)))
    for name, out in forms:
        e.self_contact_readout_dev(1, T, cap, *out)          # warm-up; the first call allocates
    e.sync()
    t = tot.cpu().numpy()
    print(f"contacts per record: mean {t[..., 0].mean():.1f}, max {int(t[..., 0].max())}; layers max {int(t[..., 1].max())}; vertices max {int(t[..., 2].max())}; "
          f"sum jn over the job {t[..., 3].sum():.6e}", flush=True)
    for name, out in forms:
        ms = []
        for _ in range(args.reps):
            e.timer_start()
            e.self_contact_readout_dev(1, T, cap, *out)
            ms.append(e.timer_stop())
        ms = np.asarray(ms)
        print(f"{name:13s}: median {np.median(ms):8.3f} ms  min {ms.min():8.3f}  max {ms.max():8.3f}  ({T} records x {B} rollouts)", flush=True)
    e.close()


if __name__ == "__main__":
    main()
