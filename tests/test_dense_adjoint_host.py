"""adjoint_mode 2 (the dense direct adjoint solve, include/diffcloth_hip.h) on host-only contexts: accepted up to the size limit of the dense
kernels (768 vertices), refused above it by dc_set_params and dc_build with DC_ERR_INVALID and a message naming the limit; modes 0 and 1 keep
working on every mesh; dc_set_solver keeps mode 2 when a direct solve is asked for."""
import numpy as np
import pytest

import meshes
from diffcloth_amd import capi, workloads

DENSE_MAX_N = 768


def host_engine(V, F, **params):
    e = capi.Engine(-1)
    e.set_mesh(V, F)
    e.set_params(**params)
    return e


def hat_mesh():
    w = workloads.hat_workload()
    return w["P"], w["F"]


@pytest.mark.parametrize("mesh", ["hat", "grid768"])
def test_mode2_accepted_up_to_the_limit(mesh):
    V, F = hat_mesh() if mesh == "hat" else meshes.grid_cloth(32, 24, 4.5, 4.5, "DOWN")
    assert V.shape[0] <= DENSE_MAX_N and (mesh == "hat" or V.shape[0] == DENSE_MAX_N)
    e = host_engine(V, F, adjoint_mode=2)
    try:
        e.build()
        assert e.N == V.shape[0] and e.params.adjoint_mode == 2
    finally:
        e.close()


def test_mode2_refused_above_the_limit():
    V, F = meshes.grid_cloth(100, 100, 4.5, 4.5, "DOWN")
    e = capi.Engine(-1)
    try:
        e.set_mesh(V, F)
        with pytest.raises(capi.DcError) as info:
            e.set_params(adjoint_mode=2)
        msg = str(info.value)
        assert msg.startswith("code 1:") and str(DENSE_MAX_N) in msg and "adjoint_mode 2" in msg
        # parameters set before the mesh: dc_build refuses
        g = capi.Engine(-1)
        try:
            g.set_params(adjoint_mode=2)
            g.set_mesh(V, F)
            with pytest.raises(capi.DcError) as info2:
                g.build()
            assert str(info2.value).startswith("code 1:") and str(DENSE_MAX_N) in str(info2.value)
        finally:
            g.close()
        # the other modes stay available on the large mesh
        for mode in (0, 1):
            e.set_params(adjoint_mode=mode)
            e.build()
            assert e.N == 10000
    finally:
        e.close()


def test_set_solver_keeps_mode2():
    V, F = meshes.grid_cloth(12, 12, 4.5, 4.5, "DOWN")
    e = host_engine(V, F, adjoint_mode=2)
    try:
        e.build()
        e.set_solver(backward_tol=1e-7)                       # only a tolerance: the mode stays
        assert e.params.adjoint_mode == 2
        e.set_solver(force_direct_adjoint=True)               # a direct solve: the dense one is one
        assert e.params.adjoint_mode == 2
        e.set_solver(force_direct_adjoint=False)
        assert e.params.adjoint_mode == 0
        e.set_solver(force_direct_adjoint=True)
        assert e.params.adjoint_mode == 1
        e.set_solver(backward_tol=1e-6)
        assert e.params.adjoint_mode == 1
    finally:
        e.close()


def test_adjoint_matrix_needs_a_batch_on_a_device():
    V, F = meshes.grid_cloth(12, 12, 4.5, 4.5, "DOWN")
    e = host_engine(V, F, adjoint_mode=2)
    try:
        e.build()
        with pytest.raises(capi.DcError):
            e.adjoint_matrix(1, 0)
        assert np.isfinite(e.vertex_data()[0]).all()
    finally:
        e.close()
