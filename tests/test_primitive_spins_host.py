"""Host-side checks of the spinning-obstacle entries (dc_set_primitive_spins, dc_set_primitive_spin_schedule, their _dev forms,
dc_get_primitive_spins, dc_get_primitive_spin_gradients and its _dev form) and of sim_rollout's primitive_spins argument, on the pattern of
tests/test_primitive_velocities_host.py. No device is touched: the C entries are called on a host-only context, which has to refuse every one
of them, and sim_rollout runs on CPU tensors with a stub engine that has sizes but no methods.
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

NEW_SYMBOLS = ["dc_set_primitive_spins", "dc_set_primitive_spin_schedule", "dc_set_primitive_spins_dev", "dc_set_primitive_spin_schedule_dev",
               "dc_get_primitive_spins", "dc_get_primitive_spin_gradients", "dc_get_primitive_spin_gradients_dev"]


def test_new_symbols_are_exported_declared_and_wrapped():
    lib = capi.load_library()
    header = open(os.path.join(ROOT, "include", "diffcloth_hip.h")).read()
    declared = set(re.findall(r"\bint\s+(dc_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in capi.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
        assert hasattr(capi.Engine, name[3:]), name


def test_header_states_the_rule_and_the_gradient():
    header = open(os.path.join(ROOT, "include", "diffcloth_hip.h")).read()
    doc = header[header.index("spinning obstacles"):header.index("int dc_set_primitive_spins(")]
    assert "v_spin = radius_p (omega[b][g] x n)" in doc and "BUILT radius" in doc
    assert "d = ((f - v_rot(p, n) m) - w[b][g] m) - v_spin m" in doc
    assert "DC_PRIM_SPHERE" in doc and "+-0" in doc and "bit for bit" in doc
    assert "omega = (0, 8 / radius, 0)" in doc and "the two add" in doc
    assert "dL/domega[b][g] = -h * sum" in doc and "m_i radius_p (n_i x g_i)" in doc and "adddr_dd = false" in doc
    assert "r_step / r_built" in doc and "Detection is unchanged" in doc
    assert "holds no DC_PRIM_SPHERE" in doc and "not finite" in doc
    # the velocity paragraph keeps its law, the shape paragraph its statement, and says where a sphere's spin goes
    vel = header[header.index("moving obstacles"):header.index("int dc_set_primitive_velocities(")]
    assert "d = (f - v_rot(p, n) m) - w[b][g] m" in vel
    shp = header[header.index("obstacle shapes per rollout"):header.index("int dc_set_primitive_shapes(")]
    assert "surface velocity of a rotating or growing" in shp and "is not modelled" in shp and "dc_set_primitive_spins" in shp


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
        "dc_set_primitive_spins": (p,),
        "dc_set_primitive_spin_schedule": (i(0), i(2), p),
        "dc_set_primitive_spins_dev": (p, i(0)),
        "dc_set_primitive_spin_schedule_dev": (i(0), i(2), p, i(0)),
        "dc_get_primitive_spins": (i(1), p),
        "dc_get_primitive_spin_gradients": (i(1), i(1), p),
        "dc_get_primitive_spin_gradients_dev": (i(1), i(1), p, i(0)),
    }
    assert sorted(calls) == sorted(NEW_SYMBOLS)
    for name, args in calls.items():
        rc = getattr(lib, name)(h, *args)
        assert rc == DC_ERR_STATE, (name, rc)
        assert len(lib.dc_last_error(h)) > 0, name
    assert np.all(buf == 0)
    e.close()


# ---- sim_rollout(primitive_spins=...): argument errors, before anything is enqueued -------------------------------------------
B, N, AF, G, TAPE = 2, 4, 2, 2, 3


def stub_sim():
    sim = BatchedSim.__new__(BatchedSim)
    sim.engine = types.SimpleNamespace(B=B, N=N, Af=AF, ngroups=G, tape=TAPE, device=0)       # sizes only: every engine call would raise AttributeError
    sim.step_num, sim.step_idx, sim._stream, sim._bwd_slots, sim.strict, sim.unconverged, sim._episode = TAPE, 0, None, set(), False, 0, 0
    return sim


def call(ps, actions=True, steps=None, dtype=torch.float32, po=None, pv=None):
    z = lambda *s: torch.zeros(s, dtype=dtype)
    return sim_rollout(stub_sim(), z(B, 3 * N), z(B, 3 * N), z(TAPE, B, 3 * AF) if actions else None, steps=steps, primitive_offsets=po,
                       primitive_velocities=pv, primitive_spins=ps)


@pytest.mark.parametrize("shape", [(TAPE, B, G, 3), (B, G, 3)])
@pytest.mark.parametrize("grad", [False, True])
def test_sim_rollout_takes_a_schedule_or_one_spin_per_rollout(shape, grad):
    """with a valid tensor — one that requires grad included — the stub is reached: the checks passed and the first engine call fails for
    lack of an engine"""
    with pytest.raises(AttributeError):
        call(torch.zeros(shape, requires_grad=grad))
    with pytest.raises(AttributeError):
        call(torch.zeros(shape, requires_grad=grad), pv=torch.zeros(B, G, 3, requires_grad=True))


def test_sim_rollout_takes_the_episode_length_from_the_spin_schedule():
    with pytest.raises(AttributeError):
        call(torch.zeros(TAPE, B, G, 3), actions=False)
    with pytest.raises(ValueError, match="steps"):
        call(torch.zeros(B, G, 3), actions=False)              # constant spins say nothing about the length
    with pytest.raises((RuntimeError, ValueError), match="tape"):
        call(torch.zeros(TAPE + 1, B, G, 3), actions=False)


@pytest.mark.parametrize("shape", [(TAPE, B, G, 2), (TAPE - 1, B, G, 3), (TAPE, B, G + 1, 3), (B + 1, G, 3), (B, G * 3), (G, 3)])
def test_sim_rollout_refuses_wrong_spin_shapes(shape):
    with pytest.raises(ValueError, match="shape.*primitive_spins"):
        call(torch.zeros(shape))


def test_sim_rollout_refuses_spins_of_another_dtype_or_device():
    with pytest.raises(ValueError, match="dtype.*primitive_spins"):
        call(torch.zeros(B, G, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="device.*primitive_spins"):
        call(torch.zeros(B, G, 3, device="meta"))
    with pytest.raises(ValueError, match="primitive_spins must be a torch tensor"):
        call(np.zeros((B, G, 3)))


def test_sim_rollout_still_refuses_offsets_that_require_grad():
    """a spin has a gradient, a centre has not: the refusal of primitive_offsets and its message stay"""
    with pytest.raises(ValueError, match="normals.*constant.*reference"):
        call(torch.zeros(B, G, 3, requires_grad=True), po=torch.zeros(TAPE, B, G, 3, requires_grad=True))
    with pytest.raises(AttributeError):
        call(torch.zeros(B, G, 3, requires_grad=True), po=torch.zeros(TAPE, B, G, 3))
