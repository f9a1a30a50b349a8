"""Backward pass of the pressed-on hat x 64 (BASELINE C3) with the Krylov direct adjoint solve (adjoint_mode 1), the dense direct solve
(adjoint_mode 2, csrc/dc_adjoint_dense.hip) and the banded direct solve (adjoint_mode 3, csrc/dc_adjoint_band.hip): one forward sweep, then
the same backward sweep over K steps in each mode.

Prints one JSON line: backward ms per batch step of the three modes (HIP events, dc_kernel_times), modes 2 and 3 split into assembly /
factorisation / solve (dc_dense_phase_times; this script sets DC_DENSE_TIMES=1, which synchronises once per step), the flop count and the
achieved fp64 rate of the factorisations (2/3 n^3 per matrix, n = 3N; the band's upper bound 2 n kl (kl + ku)), and the relative difference
of the mode-2 and mode-3 gradients from mode 1's.

    python tools/dense_adjoint_bench.py [--steps 20] [--batch 64]
"""
import argparse
import json
import os
import sys

os.environ["DC_DENSE_TIMES"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from diffcloth_amd import capi, workloads  # noqa: E402


def run(mode, K, B):
    w = workloads.hat_workload()
    X0, V0, lead_xf, timed, MU = w["start"](B, np.random.default_rng(0))
    L = len(lead_xf)
    e = capi.Engine(0)
    try:
        e.set_mesh(w["P"], w["F"]); e.set_attachments(w["att"])
        e.set_params(forward_tol=w["fwd_tol"], adjoint_mode=mode, **w["params"])
        e.set_primitives(w["prims"]); e.build()
        e.alloc_batch(B, L + K)
        e.set_mu(MU)
        e.set_state(0, X0, V0)
        e.set_fixed_point_schedule(0, np.concatenate([lead_xf, timed(K)]))
        e.rollout_forward(0, L + K)
        e.seed_gradient(L + K, None, 1e-4); e.rollout_backward(L + K, 1); e.sync()      # warm-up: allocations, first launches
        e.kernel_times(reset=True); e.dense_phase_times(reset=True)
        e.seed_gradient(L + K, None, 2.0 / ((K + 1) * e.N))
        e.rollout_backward(L + K, K); e.sync()
        kt = e.kernel_times()
        ph = e.dense_phase_times()
        gx, gv, gmu = e.get_gradient()
        stats = [e.get_stats(s)[1] for s in range(L + 1, L + K + 1)]
        band = e.adjoint_band()
        return dict(band=band, bwd_ms=kt["bwd_ms"] / K, launches=kt["bwd_launches"], phases=[p / K for p in ph], N=e.N, g=(gx, gv, gmu),
                    fp64_iters=int(sum(s["fp64_iters"].sum() for s in stats)), refine=float(np.mean([s["refine_cycles"].mean() for s in stats])),
                    converged=bool(all((s["converged"] == 1).all() for s in stats)))
    finally:
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    m1 = run(1, a.steps, a.batch)
    m2 = run(2, a.steps, a.batch)
    m3 = run(3, a.steps, a.batch)
    n = 3 * m2["N"]
    flop = a.batch * 2.0 / 3.0 * n ** 3
    rel = max(float(np.linalg.norm(x2 - x1) / max(np.linalg.norm(x1), 1e-30)) for x1, x2 in zip(m1["g"][:2], m2["g"][:2]))
    rel3 = max(float(np.linalg.norm(x3 - x1) / max(np.linalg.norm(x1), 1e-30)) for x1, x3 in zip(m1["g"][:2], m3["g"][:2]))
    kl = m3["band"]["kl"]
    flop3 = a.batch * 2.0 * n * kl * (2 * kl)
    out = dict(workload=f"hat x {a.batch} pressed on, {a.steps} backward steps", n=n,
               mode1_bwd_ms_per_step=round(m1["bwd_ms"], 3), mode2_bwd_ms_per_step=round(m2["bwd_ms"], 3),
               mode2_assembly_ms=round(m2["phases"][0], 3), mode2_factor_ms=round(m2["phases"][1], 3), mode2_solve_ms=round(m2["phases"][2], 3),
               factor_gflop_per_step=round(flop / 1e9, 1), factor_tflops=round(flop / (m2["phases"][1] * 1e-3) / 1e12, 2) if m2["phases"][1] > 0 else None,
               mode2_launches=m2["launches"], mode2_fp64_iters=m2["fp64_iters"], mode2_mean_refine_cycles=round(m2["refine"], 2),
               mode1_converged=m1["converged"], mode2_converged=m2["converged"], grad_rel_diff_mode2_vs_mode1=rel,
               mode3_bwd_ms_per_step=round(m3["bwd_ms"], 3), mode3_assembly_ms=round(m3["phases"][0], 3), mode3_factor_ms=round(m3["phases"][1], 3),
               mode3_solve_ms=round(m3["phases"][2], 3), mode3_kl=kl, mode3_band_bytes=m3["band"]["bytes_per_rollout"],
               mode3_factor_gflop_bound_per_step=round(flop3 / 1e9, 1),
               mode3_factor_tflops_of_bound=round(flop3 / (m3["phases"][1] * 1e-3) / 1e12, 2) if m3["phases"][1] > 0 else None,
               mode3_launches=m3["launches"], mode3_fp64_iters=m3["fp64_iters"], mode3_mean_refine_cycles=round(m3["refine"], 2),
               mode3_converged=m3["converged"], grad_rel_diff_mode3_vs_mode1=rel3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
