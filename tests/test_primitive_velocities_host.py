"""Host-side checks of the moving-obstacle entries (dc_set_primitive_velocities, dc_set_primitive_velocity_schedule, their _dev forms,
dc_get_primitive_velocities, dc_get_primitive_velocity_gradients and its _dev form) and of sim_rollout's primitive_velocities argument. No
device is touched: the C entries are called on a host-only context, which has to refuse every one of them, and sim_rollout runs on CPU tensors
with a stub engine that has sizes but no methods.
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

NEW_SYMBOLS = ["dc_set_primitive_velocities", "dc_set_primitive_velocity_schedule", "dc_set_primitive_velocities_dev",
               "dc_set_primitive_velocity_schedule_dev", "dc_get_primitive_velocities", "dc_get_primitive_velocity_gradients",
               "dc_get_primitive_velocity_gradients_dev"]


def test_new_symbols_are_exported_and_declared():
    lib = capi.load_library()
    header = open(os.path.join(ROOT, "include", "diffcloth_hip.h")).read()
    declared = set(re.findall(r"\bint\s+(dc_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in capi.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
        assert hasattr(capi.Engine, name[3:]), name
    # the header states the rule next to the centre rule: both places the velocity enters, the gradient and the omission it inherits
    doc = header[header.index("moving obstacles"):header.index("int dc_set_primitive_velocities(")]
    assert "d = (f - v_rot(p, n) m) - w[b][g] m" in doc and "pos + (vel - w[b][g]) h k / 2" in doc
    assert "dL/dw[b][g] = -h * sum" in doc and "adddr_dd = false" in doc
    assert "an obstacle velocity is not modelled" not in header


@pytest.mark.parametrize("built", [False, True])
def test_host_only_context_refuses_every_new_entry(built):
    e = capi.Engine(device=-1)
    if built:
        V, F = meshes.grid_cloth(5, 5, 4.5, 4.5, "DOWN")
        e.set_mesh(V, F)
        e.set_primitives([dict(kind=capi.DC_PRIM_SPHERE, group=0, center=(0, -3, 0), radius=2.0, mu=0.4)])
        e.build()
    lib, h = e.lib, e.h
    buf = np.zeros(8)                      # a pointer that is never dereferenced: a refusal comes before any use of the buffers
    p = C.c_void_p(buf.ctypes.data)
    i = C.c_int
    calls = {
        "dc_set_primitive_velocities": (p,),
        "dc_set_primitive_velocity_schedule": (i(0), i(2), p),
        "dc_set_primitive_velocities_dev": (p, i(0)),
        "dc_set_primitive_velocity_schedule_dev": (i(0), i(2), p, i(0)),
        "dc_get_primitive_velocities": (i(1), p),
        "dc_get_primitive_velocity_gradients": (i(1), i(1), p),
        "dc_get_primitive_velocity_gradients_dev": (i(1), i(1), p, i(0)),
    }
    assert sorted(calls) == sorted(NEW_SYMBOLS)
    for name, args in calls.items():
        rc = getattr(lib, name)(h, *args)
        assert rc == DC_ERR_STATE, (name, rc)
        assert len(lib.dc_last_error(h)) > 0, name
    assert np.all(buf == 0)
    e.close()


# ---- sim_rollout(primitive_velocities=...): argument errors, before anything is enqueued -------------------------------------------
B, N, AF, G, TAPE = 2, 4, 2, 2, 3


def stub_sim():
    sim = BatchedSim.__new__(BatchedSim)
    sim.engine = types.SimpleNamespace(B=B, N=N, Af=AF, ngroups=G, tape=TAPE, device=0)       # sizes only: every engine call would raise AttributeError
    sim.step_num, sim.step_idx, sim._stream, sim._bwd_slots, sim.strict, sim.unconverged, sim._episode = TAPE, 0, None, set(), False, 0, 0
    return sim


def call(pv, actions=True, steps=None, dtype=torch.float32, po=None):
    z = lambda *s: torch.zeros(s, dtype=dtype)
    return sim_rollout(stub_sim(), z(B, 3 * N), z(B, 3 * N), z(TAPE, B, 3 * AF) if actions else None, steps=steps, primitive_offsets=po,
                       primitive_velocities=pv)


@pytest.mark.parametrize("shape", [(TAPE, B, G, 3), (B, G, 3)])
@pytest.mark.parametrize("grad", [False, True])
def test_sim_rollout_takes_a_schedule_or_one_velocity_per_rollout(shape, grad):
    """with a valid tensor — one that requires grad included — the stub is reached: the checks passed and the first engine call fails for
    lack of an engine"""
    with pytest.raises(AttributeError):
        call(torch.zeros(shape, requires_grad=grad))


def test_sim_rollout_takes_the_episode_length_from_the_velocity_schedule():
    with pytest.raises(AttributeError):
        call(torch.zeros(TAPE, B, G, 3), actions=False)
    with pytest.raises(ValueError, match="steps"):
        call(torch.zeros(B, G, 3), actions=False)              # constant velocities say nothing about the length
    with pytest.raises((RuntimeError, ValueError), match="tape"):
        call(torch.zeros(TAPE + 1, B, G, 3), actions=False)


@pytest.mark.parametrize("shape", [(TAPE, B, G, 2), (TAPE - 1, B, G, 3), (TAPE, B, G + 1, 3), (B + 1, G, 3), (B, G * 3), (G, 3)])
def test_sim_rollout_refuses_wrong_velocity_shapes(shape):
    with pytest.raises(ValueError, match="shape.*primitive_velocities"):
        call(torch.zeros(shape))


def test_sim_rollout_refuses_velocities_of_another_dtype_or_device():
    with pytest.raises(ValueError, match="dtype"):
        call(torch.zeros(B, G, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="device"):
        call(torch.zeros(B, G, 3, device="meta"))
    with pytest.raises(ValueError, match="must be a torch tensor"):
        call(np.zeros((B, G, 3)))


def test_sim_rollout_still_refuses_offsets_that_require_grad():
    """a velocity has a gradient, a centre has not: the refusal of primitive_offsets and its message stay"""
    with pytest.raises(ValueError, match="normals.*constant.*reference"):
        call(torch.zeros(B, G, 3, requires_grad=True), po=torch.zeros(TAPE, B, G, 3, requires_grad=True))
    with pytest.raises(AttributeError):
        call(torch.zeros(B, G, 3, requires_grad=True), po=torch.zeros(TAPE, B, G, 3))
