"""The forward kernel instance that holds the search direction as halves reads the packet matrix in its byte-offset layout
(csrc/dc_packets.h; one address instruction per non-zero of the PCG product, csrc/dc_pklib.h) — the same gathers and the same products in
the same order as with the 10-bit column deltas that DC_PK_OFS=0 keeps, so everything must agree BITWISE between the two: anything short
of that means the order of a sum moved.

bench.py's C4 scene at N = 10 000 (the instance exists only at 20 rows per thread, so this is its smallest shape), 2 rollouts with one
workgroup each, 2 forward steps and 1 backward step per layout. The CPU side of the layout is tests/test_packet_offsets.py."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                      # noqa: E402  (the scene under test is bench.py's)

pytestmark = pytest.mark.gpu


def run(byte_offsets):
    args = types.SimpleNamespace(grid=100, fold_rows=5, fold_gap=0.02, flap_force=2.0, h=1.0 / 180, fwd_tol=1e-8, bwd_tol=5e-4, cg_tol=1e-4, cg_max=500,
                                 adjoint_mode=1, adjoint_rel_tol=1e-6, block_precond=0, selfcollision=1)
    B, S = 2, 2
    V, F, V0, flap, center = bench.scene(args)
    e = bench.make_engine(0, args, V, F, center)          # dc_build reads DC_PK_OFS
    assert e.N == 10000 and e.layout()["packet_kernel"] and e.layout()["element_windows"]
    assert e.packet_byte_offsets() == byte_offsets
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


def test_byte_offsets_and_column_deltas_agree_bitwise(monkeypatch):
    monkeypatch.setenv("DC_CLUSTER", "1")                 # 2 rollouts of this mesh would otherwise be split over several workgroups each
    monkeypatch.setenv("DC_PK_OFS", "0")
    old = run(False)
    monkeypatch.delenv("DC_PK_OFS")
    new = run(True)
    assert np.all(old["fwd_converged2"] == 1) and old["fwd_self_contacts2"].min() >= 400 and old["fwd_cg_iters2"].min() > 100, "the steps must do real work"
    print("\n[packet layouts] PD iterations", old["fwd_pd_iters1"], old["fwd_pd_iters2"], "CG iterations", old["fwd_cg_iters1"], old["fwd_cg_iters2"],
          "adjoint iterations", old["bwd_adjoint_iters"])
    for k in old:
        a, b = np.ascontiguousarray(old[k]), np.ascontiguousarray(new[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{k} differs between the packet layouts (max |diff| {np.abs(a.astype(np.float64) - b.astype(np.float64)).max():.3e})"
