"""Host-side checks of the whole-sweep device-pointer boundary (dc_rollout_*_async, the dc_*_schedule_dev setters, the dc_get_*_dev
getters of a sweep's results) and of the argument checks of diffcloth_amd.functional.sim_rollout. No device is touched: the C entries are
called on a host-only context, which has to refuse every one of them, and sim_rollout on CPU tensors with a stub engine that has sizes
but no methods — anything enqueued would raise AttributeError instead of the expected error.
"""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import meshes
from diffcloth_amd import capi
from diffcloth_amd.functional import BatchedSim, sim_rollout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DC_ERR_STATE = 3

NEW_SYMBOLS = ["dc_rollout_forward_async", "dc_rollout_backward_async", "dc_set_fixed_point_schedule_dev", "dc_set_force_schedule_dev",
               "dc_set_seed_schedule_dev", "dc_set_gradient_dev", "dc_get_gradient_dev", "dc_get_states_dev", "dc_get_dxfixed_dev",
               "dc_get_force_schedule_gradients_dev", "dc_set_mu_dev", "dc_set_vertex_forces_dev"]


def test_new_symbols_are_exported_and_declared():
    lib = capi.load_library()
    header = open(os.path.join(ROOT, "include", "diffcloth_hip.h")).read()
    declared = set(re.findall(r"\bint\s+(dc_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in capi.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    # the header says that the asynchronous rollout calls stay out of dc_kernel_times
    doc = header[header.index("dc_rollout_forward / dc_rollout_backward without the wait"):header.index("int dc_rollout_forward_async")]
    assert "dc_kernel_times" in doc


def host_only_engine(built):
    e = capi.Engine(device=-1)
    if built:
        V, F = meshes.grid_cloth(5, 5, 4.5, 4.5, "DOWN")
        e.set_mesh(V, F)
        e.set_attachments([0, 4])
        e.build()
    return e


@pytest.mark.parametrize("built", [False, True])
def test_host_only_context_refuses_every_new_entry(built):
    e = host_only_engine(built)
    lib, h = e.lib, e.h
    # a pointer that is never dereferenced: a refusal comes before any use of the buffers
    buf = np.zeros(8)
    p = C.c_void_p(buf.ctypes.data)
    i = C.c_int
    calls = {
        "dc_rollout_forward_async": (i(0), i(2)),
        "dc_rollout_backward_async": (i(2), i(2)),
        "dc_set_fixed_point_schedule_dev": (i(0), i(2), p, i(0)),
        "dc_set_force_schedule_dev": (i(0), i(2), p, p, i(0)),
        "dc_set_seed_schedule_dev": (i(0), i(2), p, p, i(0)),
        "dc_set_gradient_dev": (p, p, i(0)),
        "dc_get_gradient_dev": (p, p, p, i(0)),
        "dc_get_states_dev": (i(0), i(2), p, p, i(0)),
        "dc_get_dxfixed_dev": (i(1), i(2), p, i(0)),
        "dc_get_force_schedule_gradients_dev": (i(1), i(2), p, p, p, i(0)),
        "dc_set_mu_dev": (p, i(0)),
        "dc_set_vertex_forces_dev": (p, i(0)),
    }
    assert sorted(calls) == sorted(NEW_SYMBOLS)
    for name, args in calls.items():
        rc =getattr(lib, name)(h, *args)
        assert rc == DC_ERR_STATE, (name, rc)
        assert len(lib.dc_last_error(h)) > 0, name
    assert np.all(buf == 0)
    e.close()


# ---- sim_rollout: argument errors, before anything is enqueued -------------------------------------------------------------------
B, N, AF, G, TAPE = 2, 4, 2, 1, 3


def stub_sim(Af=AF):
    sim = BatchedSim.__new__(BatchedSim)
    sim.engine = types.SimpleNamespace(B=B, N=N, Af=Af, ngroups=G, tape=TAPE, device=0)       # sizes only: every engine call would raise AttributeError
    sim.step_num, sim.step_idx, sim._stream, sim._bwd_slots, sim.strict, sim.unconverged, sim._episode = TAPE, 0, None, set(), False, 0, 0
    return sim


def args(T=TAPE, dtype=torch.float32, Af=AF):
    z = lambda *s: torch.zeros(s, dtype=dtype)
    return dict(x0=z(B, 3 * N), v0=z(B, 3 * N), actions=z(T, B, 3 * Af), uniform_force=z(T, B, 3), vertex_force_scale=z(T, B),
                vertex_forces=z(B, 3 * N), mu=z(B, G))


def call(sim, a, **kw):
    a = dict(a)
    return sim_rollout(sim, a.pop("x0"), a.pop("v0"), a.pop("actions"), **a, **kw)


def test_sim_rollout_accepts_nothing_silently():
    """with valid arguments the stub is reached: the checks above it passed and the first engine call fails for lack of an engine"""
    with pytest.raises(AttributeError):
        call(stub_sim(), args())


def test_sim_rollout_refuses_an_episode_longer_than_the_tape():
    with pytest.raises((RuntimeError, ValueError), match="tape"):
        call(stub_sim(), args(T=TAPE + 1))
    a = args()
    a.update(actions=None, uniform_force=None, vertex_force_scale=None, vertex_forces=None)
    with pytest.raises((RuntimeError, ValueError), match="tape"):
        call(stub_sim(), a, steps=TAPE + 1)
    with pytest.raises(ValueError, match="steps"):
        call(stub_sim(), a)                                   # no schedule and no steps: the length is unknown


def test_sim_rollout_refuses_mixed_dtypes_and_devices():
    a = args()
    a["uniform_force"] = a["uniform_force"].double()
    with pytest.raises(ValueError, match="dtype"):
        call(stub_sim(), a)
    a = args()
    a["mu"] = a["mu"].to("meta")
    with pytest.raises(ValueError, match="device"):
        call(stub_sim(), a)
    a = {k: v.to(torch.int32) for k, v in args().items()}
    with pytest.raises(ValueError, match="float32 or float64"):
        call(stub_sim(), a)


@pytest.mark.parametrize("name,shape", [("x0", (B, 3 * N + 1)), ("v0", (B + 1, 3 * N)), ("actions", (TAPE, B, 3 * AF + 3)), ("uniform_force", (TAPE, B, 2)),
                                        ("uniform_force", (TAPE - 1, B, 3)), ("vertex_force_scale", (TAPE, B, 1)), ("vertex_forces", (B, N, 3)),
                                        ("mu", (B, G + 1))])
def test_sim_rollout_refuses_wrong_shapes(name, shape):
    a = args()
    a[name] = torch.zeros(shape)
    with pytest.raises(ValueError, match="shape"):
        call(stub_sim(), a)


def test_sim_rollout_refuses_actions_without_attachments_and_factors_without_a_field():
    with pytest.raises(ValueError, match="Af == 0"):
        call(stub_sim(Af=0), args(Af=0))
    a = args()
    a["vertex_forces"] = None
    with pytest.raises(ValueError, match="without vertex_forces"):
        call(stub_sim(), a)
