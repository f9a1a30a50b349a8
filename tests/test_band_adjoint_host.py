"""adjoint_mode 3 (the banded direct adjoint solve, include/diffcloth_hip.h) on host-only contexts: dc_get_adjoint_band's kl, ldab and bytes
from the matrix bandwidth dc_get_layout reports; dc_set_adjoint_band's argument check; mode 3 accepted above the dense solve's 768 vertices and
refused, with the band's bytes and the solve's LDS bytes in the message, where csrc/dc_bandplan.h's rule says so; dc_set_solver keeps mode 3."""
import numpy as np
import pytest

import meshes
from diffcloth_amd import capi, workloads

BUDGET = 8 << 30                     # dc_bandplan.h: kBandBudgetBytes
LDS = 160 * 1024 - 1024              # kBandLdsBytes


def r16(v):
    return (v + 15) // 16 * 16


def plan(N, bw, extra):
    """dc_bandplan.h's band_plan, restated"""
    kl = min(3 * N - 1, 3 * min(bw + extra, N) + 2)
    ldab = r16(3 * kl + 1)
    nbytes, lds = ldab * 3 * N * 8, 8 * (r16(3 * N) + max(kl, 32 * 32))      # one column of multipliers, or the 32 x 32 diagonal block
    return dict(kl=kl, ldab=ldab, bytes_per_rollout=nbytes), lds, nbytes <= BUDGET and lds <= LDS


def host_engine(V, F, att=None, **params):
    e = capi.Engine(-1)
    e.set_mesh(V, F)
    if att is not None:
        e.set_attachments(att)
    e.set_params(**params)
    return e


@pytest.mark.parametrize("mesh", ["grid12", "hat"])
def test_band_numbers(mesh):
    w = workloads.hat_workload()
    V, F, att = (w["P"], w["F"], w["att"]) if mesh == "hat" else (*meshes.grid_cloth(12, 12, 4.5, 4.5, "DOWN"), None)
    e = host_engine(V, F, att, adjoint_mode=3)
    try:
        e.build()
        N, bw = e.N, e.layout()["bandwidth"]
        for extra in (0, 1, 7, N, 10 ** 9):
            e.set_adjoint_band(extra)
            got = e.adjoint_band()
            want, _, ok = plan(N, bw, extra)
            assert ok and got == want, (mesh, extra, got, want)
            if extra == 0:
                assert got["kl"] == 3 * bw + 2 < 3 * N - 1
            if extra >= N:
                assert got["kl"] == 3 * N - 1
        if mesh == "hat":
            e.set_adjoint_band(0)
            assert e.adjoint_band() == dict(kl=218, ldab=656, bytes_per_rollout=656 * 1737 * 8)
        e.set_adjoint_band(3)
        before = e.adjoint_band()
        with pytest.raises(capi.DcError) as info:
            e.set_adjoint_band(-1)
        assert str(info.value).startswith("code 1:")
        assert before == plan(N, bw, 3)[0] and e.adjoint_band() == before             # a refused call changes nothing
    finally:
        e.close()


def test_mode3_accepted_above_the_dense_limit():
    V, F = meshes.grid_cloth(32, 32, 4.5, 4.5, "DOWN")
    e = host_engine(V, F, adjoint_mode=3)
    try:
        e.build()
        assert e.N == 1024 and e.params.adjoint_mode == 3
        with pytest.raises(capi.DcError):
            e.set_params(adjoint_mode=2)
        e.set_params(adjoint_mode=3)
        e.build()
    finally:
        e.close()


def test_mode3_refused_where_the_plan_says_so():
    V, F = meshes.grid_cloth(100, 100, 4.5, 4.5, "DOWN")
    e = host_engine(V, F, adjoint_mode=1)
    try:
        e.build()
        N, bw = e.N, e.layout()["bandwidth"]
        want, lds, ok = plan(N, bw, 0)
        assert not ok and want["bytes_per_rollout"] <= BUDGET and lds > LDS          # 3N doubles alone are beyond a workgroup's LDS
        with pytest.raises(capi.DcError) as info:
            e.set_params(adjoint_mode=3)                                             # on a built context
        msg = str(info.value)
        assert msg.startswith("code 1:") and "adjoint_mode 3" in msg and str(want["bytes_per_rollout"]) in msg and str(lds) in msg, msg
        # the whole matrix as the band: both numbers beyond their limits
        e.set_adjoint_band(N)
        full, lds_full, ok = plan(N, bw, N)
        assert not ok and full["bytes_per_rollout"] > BUDGET and e.adjoint_band() == full
        with pytest.raises(capi.DcError) as info:
            e.set_params(adjoint_mode=3)
        assert str(full["bytes_per_rollout"]) in str(info.value) and str(lds_full) in str(info.value)
    finally:
        e.close()
    # parameters set before the build: dc_build refuses
    g = capi.Engine(-1)
    try:
        g.set_mesh(V, F)
        g.set_params(adjoint_mode=3)
        with pytest.raises(capi.DcError) as info:
            g.build()
        assert str(info.value).startswith("code 1: dc_build") and str(lds) in str(info.value)
    finally:
        g.close()
    # dc_set_adjoint_band refuses a widening that leaves the plan, under mode 3 only
    V2, F2 = meshes.grid_cloth(60, 60, 4.5, 4.5, "DOWN")
    h = host_engine(V2, F2, adjoint_mode=3)
    try:
        h.build()
        N, bw = h.N, h.layout()["bandwidth"]
        assert plan(N, bw, 0)[2] and not plan(N, bw, N)[2]
        with pytest.raises(capi.DcError) as info:
            h.set_adjoint_band(N)
        assert str(info.value).startswith("code 1: dc_set_adjoint_band") and str(plan(N, bw, N)[1]) in str(info.value)
        assert h.adjoint_band() == plan(N, bw, 0)[0]
    finally:
        h.close()


def test_set_solver_keeps_mode3():
    V, F = meshes.grid_cloth(12, 12, 4.5, 4.5, "DOWN")
    e = host_engine(V, F, adjoint_mode=3)
    try:
        e.build()
        e.set_solver(backward_tol=1e-7)
        assert e.params.adjoint_mode == 3
        e.set_solver(force_direct_adjoint=True)
        assert e.params.adjoint_mode == 3
        e.set_solver(force_direct_adjoint=False)
        assert e.params.adjoint_mode == 0
        e.set_solver(force_direct_adjoint=True)
    finally:
        e.close()


def test_symbols_and_wrappers():
    lib = capi.load_library()
    for name in ("dc_set_adjoint_band", "dc_get_adjoint_band"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert callable(capi.Engine.set_adjoint_band) and callable(capi.Engine.adjoint_band)
