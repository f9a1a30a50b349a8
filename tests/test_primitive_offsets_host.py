"""Host-side checks of the movable-obstacle entries (dc_set_primitive_offsets, dc_set_primitive_offset_schedule, their _dev forms,
dc_get_primitive_centers) and of sim_rollout's primitive_offsets argument. No device is touched: the C entries are called on a host-only
context, which has to refuse every one of them, sim_rollout on CPU tensors with a stub engine that has sizes but no methods, and the
rounding rule / group expansion (csrc/dc_primoffset.h, shared by the host path and the conversion kernel) by a small native program.
"""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import meshes
from diffcloth_amd import capi
from diffcloth_amd.functional import BatchedSim, sim_rollout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DC_ERR_STATE = 3

NEW_SYMBOLS = ["dc_set_primitive_offsets", "dc_set_primitive_offset_schedule", "dc_set_primitive_offsets_dev",
               "dc_set_primitive_offset_schedule_dev", "dc_get_primitive_centers"]


def test_new_symbols_are_exported_and_declared():
    lib = capi.load_library()
    header = open(os.path.join(ROOT, "include", "diffcloth_hip.h")).read()
    declared = set(re.findall(r"\bint\s+(dc_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in capi.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    # the header states the one rule and what drops the offsets
    doc = header[header.index("movable obstacles"):header.index("int dc_set_primitive_offsets(")]
    assert "fp32( (double) dc_primitive.center_p + d[b][g] )" in doc and "rounded once" in doc
    assert "dc_alloc_batch, dc_set_primitives and dc_build drop offsets and schedule" in doc
    for name in NEW_SYMBOLS:
        assert hasattr(capi.Engine, name[3:]), name


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
        "dc_set_primitive_offsets": (p,),
        "dc_set_primitive_offset_schedule": (i(0), i(2), p),
        "dc_set_primitive_offsets_dev": (p, i(0)),
        "dc_set_primitive_offset_schedule_dev": (i(0), i(2), p, i(0)),
        "dc_get_primitive_centers": (i(1), p),
    }
    assert sorted(calls) == sorted(NEW_SYMBOLS)
    for name, args in calls.items():
        rc = getattr(lib, name)(h, *args)
        assert rc == DC_ERR_STATE, (name, rc)
        assert len(lib.dc_last_error(h)) > 0, name
    assert np.all(buf == 0)
    e.close()


# ---- sim_rollout(primitive_offsets=...): argument errors, before anything is enqueued ----------------------------------------------
B, N, AF, G, TAPE = 2, 4, 2, 2, 3


def stub_sim():
    sim = BatchedSim.__new__(BatchedSim)
    sim.engine = types.SimpleNamespace(B=B, N=N, Af=AF, ngroups=G, tape=TAPE, device=0)       # sizes only: every engine call would raise AttributeError
    sim.step_num, sim.step_idx, sim._stream, sim._bwd_slots, sim.strict, sim.unconverged, sim._episode = TAPE, 0, None, set(), False, 0, 0
    return sim


def call(po, actions=True, steps=None, dtype=torch.float32):
    z = lambda *s: torch.zeros(s, dtype=dtype)
    return sim_rollout(stub_sim(), z(B, 3 * N), z(B, 3 * N), z(TAPE, B, 3 * AF) if actions else None, steps=steps, primitive_offsets=po)


@pytest.mark.parametrize("shape", [(TAPE, B, G, 3), (B, G, 3)])
def test_sim_rollout_takes_a_schedule_or_one_offset_per_rollout(shape):
    """with a valid tensor the stub is reached: the checks passed and the first engine call fails for lack of an engine"""
    with pytest.raises(AttributeError):
        call(torch.zeros(shape))


def test_sim_rollout_takes_the_episode_length_from_the_offset_schedule():
    with pytest.raises(AttributeError):
        call(torch.zeros(TAPE, B, G, 3), actions=False)
    with pytest.raises(ValueError, match="steps"):
        call(torch.zeros(B, G, 3), actions=False)              # constant offsets say nothing about the length
    with pytest.raises((RuntimeError, ValueError), match="tape"):
        call(torch.zeros(TAPE + 1, B, G, 3), actions=False)


@pytest.mark.parametrize("shape", [(TAPE, B, G, 2), (TAPE - 1, B, G, 3), (TAPE, B, G + 1, 3), (B + 1, G, 3), (B, G * 3), (G, 3)])
def test_sim_rollout_refuses_wrong_offset_shapes(shape):
    with pytest.raises(ValueError, match="shape.*primitive_offsets"):
        call(torch.zeros(shape))


def test_sim_rollout_refuses_offsets_of_another_dtype_or_device():
    with pytest.raises(ValueError, match="dtype"):
        call(torch.zeros(B, G, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="device"):
        call(torch.zeros(B, G, 3, device="meta"))


def test_sim_rollout_refuses_offsets_that_require_grad_and_says_why():
    po = torch.zeros(TAPE, B, G, 3, requires_grad=True)
    with pytest.raises(ValueError, match="normals.*constant.*reference"):
        call(po)
    with pytest.raises(AttributeError):                        # detached, as the message advises
        call(po.detach())


# ---- the one rule, as the host path and the conversion kernel compile it -----------------------------------------------------------
def test_rounding_rule_and_group_expansion(tmp_path):
    """csrc/dc_primoffset.h (tests/native/prim_offsets_check.cpp): the fp64 sum is rounded once — a case where rounding the centre first gives
    another fp32 number —, equals what a context built at the moved centre rounds, and one offset moves every child of a group."""
    csrc = os.path.join(ROOT, "diffcloth_amd", "csrc")
    exe = str(tmp_path / "prim_offsets_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "native", "prim_offsets_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ALL OK"), r.stdout + r.stderr


def test_both_paths_include_the_one_rule():
    """the host path (dc_engine.hip) and the conversion kernel (dc_boundary.hip) call dc_primoffset.h; neither restates the sum"""
    csrc = os.path.join(ROOT, "diffcloth_amd", "csrc")
    for name, fn in (("dc_engine.hip", "expand_centres("), ("dc_boundary.hip", "offset_centre(")):
        src = open(os.path.join(csrc, name)).read()
        assert '#include "dc_primoffset.h"' in src and fn in src, name
