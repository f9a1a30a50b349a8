"""Host-side checks of the contact read-out's gradient entries (dc_set_contact_readout_gradients[_dev], Engine.set_contact_readout_gradients[_dev],
sim_rollout(contact_readout=True)): exports and signatures, the refusals on a host-only context, the argument checks of the Python layer. No
device is touched."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import meshes
from diffcloth_amd import capi
from diffcloth_amd import functional
from diffcloth_amd.functional import BatchedSim, sim_rollout, sim_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DC_ERR_INVALID, DC_ERR_STATE = 1, 3


def header():
    return open(os.path.join(ROOT, "include", "diffcloth_hip.h")).read()


def test_entries_are_exported_with_the_stated_signatures():
    lib = capi.load_library()
    flat = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert "int dc_set_contact_readout_gradients(dc_ctx *ctx, int slot0, int nslots, const double *dL_djn , const double *dL_dwrench );" in flat
    assert ("int dc_set_contact_readout_gradients_dev(dc_ctx *ctx, int slot0, int nslots, const void *d_dL_djn , const void *d_dL_dwrench , "
            "int is_f32);") in flat
    for name in ("dc_set_contact_readout_gradients", "dc_set_contact_readout_gradients_dev"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert hasattr(capi.Engine, "set_contact_readout_gradients") and hasattr(capi.Engine, "set_contact_readout_gradients_dev")
    assert inspect.signature(sim_rollout).parameters["contact_readout"].default is False


def test_header_states_the_rule():
    h = header()
    doc = h[h.index("Gradients of a loss on the contact read-out."):h.index("int dc_set_contact_readout_gradients(")]
    for phrase in ("phi_i = -J^ - tau^ x (x_i - c_g) + (jn^_i + S^) n_i", "take-off: 0, stick: -phi_i", "dL/dv at slot s - 1  += m_i q_i",
                   "y~ = y + q / h", "u_i + phi_i / h", "never modified", "same bits", "enqueues no additional kernel", "DC_ERR_STATE",
                   "dc_clear_schedules and dc_alloc_batch", "7..9"):
        assert phrase in doc, phrase


@pytest.mark.parametrize("built", [False, True])
def test_refusals_on_a_host_only_context(built):
    e = capi.Engine(device=-1)
    if built:
        V, F = meshes.grid_cloth(5, 5, 4.5, 4.5, "DOWN")
        e.set_mesh(V, F)
        e.set_primitives([dict(kind=capi.DC_PRIM_SPHERE, group=0, center=(0, -3, 0), radius=2.0, mu=0.4)])
        e.build()
    lib, h = e.lib, e.h
    buf = np.zeros(16)                     # never dereferenced: a refusal comes before any use of the buffers
    p, i = C.c_void_p(buf.ctypes.data), C.c_int
    for name, extra in (("dc_set_contact_readout_gradients", ()), ("dc_set_contact_readout_gradients_dev", (i(0),))):
        fn = getattr(lib, name)
        for args, msg in (((i(0), i(1), p, p), "slot 0 has no record"), ((i(-2), i(1), p, None), "slot 0 has no record"), ((i(1), i(0), p, p), "nslots < 1")):
            assert fn(h, *args, *extra) == DC_ERR_INVALID, (name, msg)
            assert msg in lib.dc_last_error(h).decode()
        assert fn(h, i(1), i(1), p, p, *extra) == DC_ERR_STATE, name          # well formed: there is no batch on a host-only context
        assert fn(h, i(1), i(1), None, None, *extra) == DC_ERR_STATE, name    # ... and nothing to clear
        assert len(lib.dc_last_error(h)) > 0
    assert np.all(buf == 0)
    e.close()


def test_wrench_weights_without_a_primitive_group_are_refused():
    e = capi.Engine(device=-1)
    V, F = meshes.grid_cloth(5, 5, 4.5, 4.5, "DOWN")
    e.set_mesh(V, F)
    e.set_primitives([])
    e.build()
    buf = np.zeros(16)
    p, i = C.c_void_p(buf.ctypes.data), C.c_int
    assert e.lib.dc_set_contact_readout_gradients(e.h, i(1), i(1), p, p) == DC_ERR_INVALID
    assert "no primitive group" in e.lib.dc_last_error(e.h).decode()
    assert e.lib.dc_set_contact_readout_gradients_dev(e.h, i(1), i(1), None, p, i(1)) == DC_ERR_INVALID
    assert e.lib.dc_set_contact_readout_gradients(e.h, i(1), i(1), p, None) == DC_ERR_STATE
    e.close()


B, N, G, TAPE = 2, 5, 2, 3


def stub_engine():
    e = capi.Engine.__new__(capi.Engine)
    e.B, e.N, e.ngroups, e.tape, e.device, e.h = B, N, G, TAPE, 0, None      # sizes only: a call that reached the library would raise AttributeError
    return e


def test_capi_wrappers_check_their_arguments():
    e = stub_engine()
    with pytest.raises(ValueError, match="slot 0"):
        e.set_contact_readout_gradients(0, np.zeros((1, B, N)))
    with pytest.raises(ValueError, match="covers 1 slot"):
        e.set_contact_readout_gradients(1, np.zeros((1, B, N)), np.zeros((2, B, G, 10)))
    with pytest.raises(ValueError):
        e.set_contact_readout_gradients(1, np.zeros((1, B, N + 1)))
    with pytest.raises(ValueError, match="slot 0"):
        e.set_contact_readout_gradients_dev(0, 1, torch.zeros((1, B, N)))
    with pytest.raises(ValueError, match="CUDA"):
        e.set_contact_readout_gradients_dev(1, 1, torch.zeros((1, B, N)))
    with pytest.raises(AttributeError):                      # valid arguments reach the (missing) library
        e.set_contact_readout_gradients(1, np.zeros((2, B, N)), np.zeros((2, B, G, 10)))


def test_sim_rollout_checks_contact_readout_before_it_touches_a_device():
    sim = BatchedSim.__new__(BatchedSim)
    sim.engine = types.SimpleNamespace(B=B, N=N, Af=0, ngroups=1, nprims=0, tape=TAPE, device=None)
    x = torch.zeros((B, 3 * N))
    with pytest.raises(ValueError, match="True or False"):
        sim_rollout(sim, x, x, steps=2, contact_readout=1)
    with pytest.raises(ValueError, match="no primitive"):
        sim_rollout(sim, x, x, steps=2, contact_readout=True)
    with pytest.raises(ValueError, match="pass steps="):      # the other checks still come first
        sim_rollout(sim, x, x, contact_readout=True)
    doc = sim_rollout.__doc__
    assert "contact_readout=True returns (xs, vs, jn, wrench)" in doc and "`sim_step` has no such output" in doc
    assert "contact_readout" not in inspect.signature(sim_step).parameters
    assert "contact_readout" in inspect.signature(functional.RolloutFunction.forward).parameters
