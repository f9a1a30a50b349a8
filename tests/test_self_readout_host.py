"""Host-side checks of the self-contact read-out (dc_get_self_contact_readout, dc_get_self_contact_readout_dev, Engine.self_contact_readout /
self_contact_readout_dev, BatchedSim.self_contact_readout). No device is touched: the C entries are called on a host-only context, the Python
wrappers on stubs that have sizes but no library.
"""
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
from diffcloth_amd.functional import BatchedSim, sim_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DC_ERR_INVALID, DC_ERR_STATE = 1, 3


def header():
    return open(os.path.join(ROOT, "include", "diffcloth_hip.h")).read()


def test_entries_are_exported_with_the_stated_signatures():
    lib = capi.load_library()
    flat = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert ("int dc_get_self_contact_readout(dc_ctx *ctx, int slot0, int nslots, int cap, int *pairs , double *impulse , double *vertex_impulse , "
            "double *totals );") in flat
    assert ("int dc_get_self_contact_readout_dev(dc_ctx *ctx, int slot0, int nslots, int cap, void *d_pairs , void *d_impulse , "
            "void *d_vertex_impulse , void *d_totals , int is_f32);") in flat
    for name, nargs in (("dc_get_self_contact_readout", 8), ("dc_get_self_contact_readout_dev", 9)):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs and fn.argtypes[1:4] == [C.c_int] * 3
    sig = inspect.signature(capi.Engine.self_contact_readout).parameters
    assert [sig[k].default for k in ("nslots", "cap", "pairs", "impulse", "vertex_impulse", "totals")] == [1, None, True, True, True, True]
    sig = inspect.signature(capi.Engine.self_contact_readout_dev).parameters
    assert list(sig)[1:] == ["slot0", "nslots", "cap", "pairs", "impulse", "vertex_impulse", "totals"]
    sig = inspect.signature(BatchedSim.self_contact_readout).parameters
    assert sig["slot0"].default == 1 and sig["nslots"].default is None and sig["cap"].default is None and sig["dtype"].default is torch.float32
    assert "self_contact" not in " ".join(inspect.signature(sim_step).parameters)          # sim_step has no such output


def test_header_states_the_rule():
    h = header()
    doc = h[h.index("Self-contact read-out: what the cloth's sheets press on each other with"):h.index("int dc_get_self_contact_readout(")]
    for text in ("g_i = f_i + r_p,i", "d_k = g_A / m_A - g_B / m_B", "r_k = r(n_k, d_k, 0.1) / (1/m_A + 1/m_B)", "g_A += r_k, g_B -= r_k",
                 "r_self,i = sum of +-r_k", "walked in record order", "vertex-disjoint", "CURRENT mu[b][group]", "neither read nor written",
                 "dc_set_record", "{id1, id2, layer, state}", "{-1, -1, -1, 0}", "1 = take-off, 2 = stick, 3 = slide", "dc_get_self_contacts",
                 "still enter the sums", "id2 receives -r_k", "bit-reproducible", "NO GRADIENT", "DC_ERR_INVALID", "DC_ERR_STATE",
                 "no allocation"):
        assert text in doc, text
    assert "{contacts evaluated, layers, distinct vertices, sum jn, sum |r_k - jn_k n_k|, take-off, stick, slide}" in doc


@pytest.mark.parametrize("built", [False, True])
def test_refusals_on_a_host_only_context(built):
    e = capi.Engine(device=-1)
    if built:
        V, F = meshes.grid_cloth(5, 5, 4.5, 4.5, "DOWN")
        e.set_mesh(V, F)
        e.set_primitives([dict(kind=capi.DC_PRIM_SPHERE, group=0, center=(0, -3, 0), radius=2.0, mu=0.4)])
        e.build()
    lib, h = e.lib, e.h
    buf = np.zeros(8)                      # never dereferenced: a refusal comes before any use of the buffers
    p = C.c_void_p(buf.ctypes.data)
    for name, extra in (("dc_get_self_contact_readout", ()), ("dc_get_self_contact_readout_dev", (1,))):
        fn = getattr(lib, name)
        for args, msg in (((0, 1, 4, p, p, p, p), "slot 0 has no record"), ((-1, 1, 4, p, p, p, p), "slot 0 has no record"),
                          ((1, 0, 4, p, p, p, p), "nslots < 1"), ((1, 1, 4, None, None, None, None), "all null"),
                          ((1, 1, 0, p, None, None, p), "cap < 1"), ((1, 1, -3, None, p, p, None), "cap < 1")):
            assert fn(h, *args, *extra) == DC_ERR_INVALID, (name, msg)
            assert msg in lib.dc_last_error(h).decode()
        # well-formed arguments: no device, no batch — refused as the neighbouring getters refuse it; cap is not looked at without a list
        assert fn(h, 1, 1, 4, p, p, p, p, *extra) == DC_ERR_STATE, name
        assert fn(h, 1, 1, 0, None, None, p, p, *extra) == DC_ERR_STATE, name
        assert lib.dc_get_contact_readout(h, C.c_int(1), C.c_int(1), p, p, None) == DC_ERR_STATE
        assert len(lib.dc_last_error(h)) > 0
    assert lib.dc_get_self_contact_readout(None, 1, 1, 4, p, p, p, p) == DC_ERR_INVALID
    assert np.all(buf == 0)
    e.close()


# ---- the Python wrappers check their arguments before anything reaches the library ----
B, N, TAPE = 2, 5, 3


def stub_engine(max_self_contacts=0):
    e = capi.Engine.__new__(capi.Engine)
    e.B, e.N, e.ngroups, e.tape, e.device, e.h = B, N, 1, TAPE, 0, None      # sizes only: a call that reached the library would raise AttributeError
    e.params = capi.dc_params()
    e.params.max_self_contacts = max_self_contacts
    return e


def test_cap_none_is_the_contexts_list_size():
    assert stub_engine().max_self_contacts == 2048                  # max(2048, N)
    assert stub_engine(100).max_self_contacts == 100
    assert stub_engine(50000).max_self_contacts == 16000
    e = stub_engine()
    e.N = 5000
    assert e.max_self_contacts == 5000


def test_capi_wrappers_check_their_arguments():
    e = stub_engine()
    with pytest.raises(ValueError, match="slot 0"):
        e.self_contact_readout(0, 1)
    with pytest.raises(ValueError, match="nslots"):
        e.self_contact_readout(1, 0)
    with pytest.raises(ValueError, match="nothing asked for"):
        e.self_contact_readout(1, 1, pairs=False, impulse=False, vertex_impulse=False, totals=False)
    with pytest.raises(ValueError, match="cap must be >= 1"):
        e.self_contact_readout(1, 1, cap=0)
    with pytest.raises(ValueError, match="nothing asked for"):
        e.self_contact_readout_dev(1, 1, 4)
    with pytest.raises(ValueError, match="cap must be >= 1"):
        e.self_contact_readout_dev(1, 1, 0, pairs=torch.zeros((1, B, 0, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match="int32"):
        e.self_contact_readout_dev(1, 1, 4, pairs=torch.zeros((1, B, 4, 4), dtype=torch.int64))
    with pytest.raises(ValueError, match="CUDA"):
        e.self_contact_readout_dev(1, 1, 4, impulse=torch.zeros((1, B, 4, 4)))
    with pytest.raises(ValueError, match="CUDA"):
        e.self_contact_readout_dev(1, 1, 4, vertex_impulse=torch.zeros((1, B, N, 3)))
    with pytest.raises(AttributeError):                      # valid arguments reach the (missing) library
        e.self_contact_readout(1, 2)
    with pytest.raises(AttributeError):                      # no list asked for: cap is not looked at
        e.self_contact_readout(1, 1, cap=0, pairs=False, impulse=False)


def test_batched_sim_checks_its_arguments():
    sim = BatchedSim.__new__(BatchedSim)
    sim.engine = types.SimpleNamespace(B=B, N=N, ngroups=1, tape=TAPE, device=0, max_self_contacts=2048)
    sim.step_num, sim.step_idx, sim._stream = TAPE, 2, None
    with pytest.raises(ValueError, match="slot 0"):
        sim.self_contact_readout(0)
    with pytest.raises(ValueError, match="taken 2 step"):
        sim.self_contact_readout(1, 3)
    with pytest.raises(ValueError, match="taken 2 step"):
        sim.self_contact_readout(3)
    with pytest.raises(ValueError, match="dtype"):
        sim.self_contact_readout(1, 1, dtype=torch.float16)
    with pytest.raises(ValueError, match="nothing asked for"):
        sim.self_contact_readout(1, 1, pairs=False, impulse=False, vertex_impulse=False, totals=False)
    with pytest.raises(ValueError, match="cap must be >= 1"):
        sim.self_contact_readout(1, 1, cap=0)
    assert "NO gradient" in BatchedSim.self_contact_readout.__doc__
