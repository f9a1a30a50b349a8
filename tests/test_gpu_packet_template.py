"""The forward kernel on the packet matrix's template layout (csrc/dc_packets.h: values only under one set of twelve column offsets;
csrc/dc_pklib.h: PkTplRows — the row is the immediate offset of the gather) against the same kernel on the byte-offset layout that
DC_PK_TPL=0 keeps: the same gathers and the same products in the same order, with exact zeros times finite halves interleaved where a row
lacks a neighbour, so states, records, contact sets, iteration counts and gradients must agree BITWISE. Anything short of that means a
slot reads the wrong row, a guard row is not zero, or the order of a sum moved.

bench.py's C4 scene on the smallest grids that reach the instances (the halves instances exist at 512 x 20 rows, 8 193 ... 10 240 vertices,
and at 768 x 14 from 9 217 vertices): 91 x 91 (the smallest; 1 959 padding rows behind the mesh), 101 x 101 (10 201 vertices: the zero slots of
the rows 0 ... 200 point into the lower guard and those of the last 201 REAL rows, 10 000 ... 10 200, into the padding rows and, from row
10 039 on, into the upper guard) and 97 x 97 with DC_PK_THREADS=768 (bases refreshed at row 11 of 14). 2 rollouts with one workgroup each,
2 forward steps and 1 backward step per layout. The headline's own grid runs this kernel by default in tests/test_gpu_packet_offsets.py
(against the 10-bit column deltas) and tests/test_gpu_bench_parity.py (against the oracle). The CPU side is tests/test_packet_template.py."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                      # noqa: E402  (the scene under test is bench.py's)

pytestmark = pytest.mark.gpu


def run(grid, layout):
    args = types.SimpleNamespace(grid=grid, fold_rows=5, fold_gap=0.02, flap_force=2.0, h=1.0 / 180, fwd_tol=1e-8, bwd_tol=5e-4, cg_tol=1e-4, cg_max=500,
                                 adjoint_mode=1, adjoint_rel_tol=1e-6, block_precond=0, selfcollision=1)
    B, S = 2, 2
    V, F, V0, flap, center = bench.scene(args)
    e = bench.make_engine(0, args, V, F, center)          # dc_build reads DC_PK_TPL and DC_PK_THREADS
    assert e.N == grid * grid and e.layout()["packet_kernel"] and e.layout()["element_windows"] and not e.layout()["renumbered"]
    assert e.packet_layout() == layout and e.packet_byte_offsets()
    e.alloc_batch(B, S)                                   # dc_alloc_batch reads DC_CLUSTER
    assert e.cluster() == 1, "one workgroup per rollout: the kernel under test"
    X0, MU = bench.rollout_inputs(V0, np.arange(B))
    e.set_mu(MU)
    e.set_state(0, X0, np.zeros_like(X0))
    e.set_vertex_forces(np.tile(bench.flap_force(args, e.vertex_data()[0], flap), (B, 1)))
    e.rollout_forward(0, S)
    e.seed_gradient(S, None, 2.0 / ((S + 1) * e.N))
    e.rollout_backward(S, 1)
    out = {}
    for s in range(1, S + 1):
        out[f"x{s}"], out[f"v{s}"] = e.get_state(s)
        out[f"f{s}"], out[f"r{s}"] = e.get_record(s)
        out[f"prim{s}"], out[f"normal{s}"] = e.get_contacts(s)
        fs, bs = e.get_stats(s)
        for k in ("converged", "pd_iters", "cg_iters", "prim_contacts", "self_contacts", "last_xdiff"):
            out[f"fwd_{k}{s}"] = fs[k]
    bs = e.get_stats(S)[1]
    for k in ("converged", "adjoint_iters", "cg_iters", "last_udiff", "refine_cycles"):
        out[f"bwd_{k}"] = bs[k]
    out["dL_dx"], out["dL_dv"], out["dL_dmu"] = e.get_gradient()
    e.close()
    return out


@pytest.mark.parametrize("grid,threads", [(91, 0), (101, 0), (97, 768)])
def test_template_and_byte_offsets_agree_bitwise(monkeypatch, grid, threads):
    monkeypatch.setenv("DC_CLUSTER", "1")                 # 2 rollouts of this mesh would otherwise be split over several workgroups each
    if threads:
        monkeypatch.setenv("DC_PK_THREADS", str(threads))
    monkeypatch.setenv("DC_PK_TPL", "0")
    old = run(grid, 1)
    monkeypatch.setenv("DC_PK_TPL", "1")
    new = run(grid, 2)
    print(f"\n[packet template {grid} x {grid}] PD iterations", old["fwd_pd_iters1"], old["fwd_pd_iters2"], "CG iterations", old["fwd_cg_iters1"], old["fwd_cg_iters2"],
          "self contacts", old["fwd_self_contacts2"], "converged", old["fwd_converged2"], "adjoint iterations", old["bwd_adjoint_iters"])
    assert old["fwd_pd_iters2"].min() > 1 and old["fwd_self_contacts2"].min() > 0 and old["fwd_cg_iters2"].min() > 100, "the steps must do real work"
    for k in old:
        a, b = np.ascontiguousarray(old[k]), np.ascontiguousarray(new[k])
        assert np.all(np.isfinite(a.astype(np.float64))), f"{k} is not finite"
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{k} differs between the packet layouts (max |diff| {np.abs(a.astype(np.float64) - b.astype(np.float64)).max():.3e})"
