"""Host-side checks of the obstacle-shape entries (dc_set_primitive_shapes, dc_set_primitive_shape_schedule, their _dev forms,
dc_get_primitive_shapes), of Engine.built_primitive_shapes, of rotated_primitive_shapes and of sim_rollout's primitive_shapes argument. No
device is touched: the C entries are called on a host-only context, which has to refuse every one of them, sim_rollout runs on CPU tensors
with a stub engine that has sizes but no methods, and the dc_primitive -> row -> device-primitive conversion (csrc/dc_primshape.h, shared by
dc_build and the host setters) is checked by a small native program.
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
from diffcloth_amd.functional import BatchedSim, rotated_primitive_shapes, sim_rollout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DC_ERR_STATE = 3

NEW_SYMBOLS = ["dc_set_primitive_shapes", "dc_set_primitive_shape_schedule", "dc_set_primitive_shapes_dev",
               "dc_set_primitive_shape_schedule_dev", "dc_get_primitive_shapes"]


def test_new_symbols_are_exported_and_declared():
    lib = capi.load_library()
    header = open(os.path.join(ROOT, "include", "diffcloth_hip.h")).read()
    declared = set(re.findall(r"\bint\s+(dc_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in capi.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
        assert hasattr(capi.Engine, name[3:]), name
    assert hasattr(capi.Engine, "built_primitive_shapes")
    # the header states the rule, what the shape does not carry, and what the _dev forms cannot check
    doc = header[header.index("obstacle shapes per rollout and step"):header.index("int dc_set_primitive_shapes(")]
    assert "s[b][p] = {top_offset[3], corner2[3], radius, length}" in doc and "rounded once" in doc
    assert "surface velocity of a rotating or growing" in doc and "is not modelled" in doc
    assert "no gradient with" in doc and "world-up" in doc
    assert "degenerate shape" in doc and "context built with it would give" in doc
    assert "DC_PRIM_SPHERE_DISCRETIZED" in doc


@pytest.mark.parametrize("built", [False, True])
def test_host_only_context_refuses_every_new_entry(built):
    e = capi.Engine(device=-1)
    if built:
        V, F = meshes.grid_cloth(5, 5, 4.5, 4.5, "DOWN")
        e.set_mesh(V, F)
        e.set_primitives([dict(kind=capi.DC_PRIM_SPHERE, group=0, center=(0, -3, 0), radius=2.0, mu=0.4)])
        e.build()
    lib, h = e.lib, e.h
    buf = np.zeros(16)                     # a pointer that is never dereferenced: a refusal comes before any use of the buffers
    p = C.c_void_p(buf.ctypes.data)
    i = C.c_int
    calls = {
        "dc_set_primitive_shapes": (p,),
        "dc_set_primitive_shape_schedule": (i(0), i(2), p),
        "dc_set_primitive_shapes_dev": (p, i(0)),
        "dc_set_primitive_shape_schedule_dev": (i(0), i(2), p, i(0)),
        "dc_get_primitive_shapes": (i(1), p),
    }
    assert sorted(calls) == sorted(NEW_SYMBOLS)
    for name, args in calls.items():
        rc = getattr(lib, name)(h, *args)
        assert rc == DC_ERR_STATE, (name, rc)
        assert len(lib.dc_last_error(h)) > 0, name
    assert np.all(buf == 0)
    e.close()


def test_built_primitive_shapes_are_the_rows_of_the_dicts():
    e = capi.Engine(device=-1)
    assert e.built_primitive_shapes().shape == (0, 8)
    prims = [dict(kind=capi.DC_PRIM_SPHERE, group=0, center=(0, -3, 0), radius=2.125 + 1e-9, mu=0.4),
             dict(kind=capi.DC_PRIM_CAPSULE, group=1, center=(1, 2, 3), radius=0.5, length=3.0, top_offset=(0.1, 3.0, -0.7)),
             dict(kind=capi.DC_PRIM_PLANE, group=2, center=(0, 0, 0), radius=0.0, top_offset=(-1.5, 0.3, -1.5), corner2=(1.5, 0.3 + 1e-12, -1.5))]
    e.set_primitives(prims)
    rows = e.built_primitive_shapes()
    assert rows.shape == (3, 8) and rows.dtype == np.float64
    want = np.array([[0, 0, 0, 0, 0, 0, 2.125 + 1e-9, 0.0],
                     [0.1, 3.0, -0.7, 0, 0, 0, 0.5, 3.0],
                     [-1.5, 0.3, -1.5, 1.5, 0.3 + 1e-12, -1.5, 0.0, 0.0]])
    np.testing.assert_array_equal(rows, want)               # fp64, unrounded
    rows[0, 6] = 99.0                                       # a copy: the engine's own rows are not the caller's to change
    np.testing.assert_array_equal(e.built_primitive_shapes(), want)
    e.set_primitives(prims[:1])
    np.testing.assert_array_equal(e.built_primitive_shapes(), want[:1])
    e.close()


# ---- rotated_primitive_shapes against numpy ----------------------------------------------------------------------------------------
def rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_rotated_primitive_shapes_against_numpy(dtype):
    rng = np.random.default_rng(3)
    P = 3
    shapes = rng.standard_normal((P, 8))
    R = np.stack([np.stack([rot("xyz"[(b + p) % 3], 0.3 * (b + 1) - 0.2 * p) for p in range(P)]) for b in range(4)])       # [4][P][3][3]
    got = rotated_primitive_shapes(torch.as_tensor(shapes, dtype=dtype), torch.as_tensor(R, dtype=dtype))
    assert got.dtype == dtype and tuple(got.shape) == (4, P, 8)
    sh = shapes.astype(np.float32 if dtype == torch.float32 else np.float64)
    want = np.empty((4, P, 8))
    for b in range(4):
        for p in range(P):
            want[b, p, 0:3] = R[b, p] @ sh[p, 0:3]
            want[b, p, 3:6] = R[b, p] @ sh[p, 3:6]
            want[b, p, 6:8] = sh[p, 6:8]
    # the rotation is computed in the tensors' dtype: a few ulp of it on vectors of norm ~2
    np.testing.assert_allclose(got.numpy(), want, atol=(4e-6 if dtype == torch.float32 else 1e-14), rtol=0)
    np.testing.assert_array_equal(got.numpy()[..., 6:8], np.broadcast_to(sh[:, 6:8], (4, P, 2)))      # radius and length are kept, bit for bit
    # the identity keeps dyadic rows bit for bit, and leading dimensions broadcast both ways: shapes [T, B, P, 8] with one R per primitive
    dy = torch.as_tensor(np.round(shapes * 16) / 16, dtype=dtype)
    eye = torch.eye(3, dtype=dtype).expand(P, 3, 3)
    np.testing.assert_array_equal(rotated_primitive_shapes(dy.expand(2, 5, P, 8), eye).numpy(), dy.expand(2, 5, P, 8).numpy())
    assert tuple(rotated_primitive_shapes(dy, torch.as_tensor(R, dtype=dtype)[None].expand(2, 4, P, 3, 3)).shape) == (2, 4, P, 8)
    with pytest.raises(ValueError, match="rotated_primitive_shapes"):
        rotated_primitive_shapes(torch.zeros(P, 7), eye)
    with pytest.raises(ValueError, match="rotated_primitive_shapes"):
        rotated_primitive_shapes(torch.zeros(P, 8), torch.zeros(P, 3, 2))


# ---- sim_rollout(primitive_shapes=...): argument errors, before anything is enqueued -----------------------------------------------
B, N, AF, G, P, TAPE = 2, 4, 2, 2, 3, 3


def stub_sim(nprims=P):
    sim = BatchedSim.__new__(BatchedSim)
    sizes = dict(B=B, N=N, Af=AF, ngroups=G, tape=TAPE, device=0)       # sizes only: every engine call would raise AttributeError
    if nprims is not None:
        sizes["nprims"] = nprims
    sim.engine = types.SimpleNamespace(**sizes)
    sim.step_num, sim.step_idx, sim._stream, sim._bwd_slots, sim.strict, sim.unconverged, sim._episode = TAPE, 0, None, set(), False, 0, 0
    return sim


def call(ps, actions=True, steps=None, dtype=torch.float32, sim=None):
    z = lambda *s: torch.zeros(s, dtype=dtype)
    return sim_rollout(sim or stub_sim(), z(B, 3 * N), z(B, 3 * N), z(TAPE, B, 3 * AF) if actions else None, steps=steps, primitive_shapes=ps)


@pytest.mark.parametrize("shape", [(TAPE, B, P, 8), (B, P, 8)])
def test_sim_rollout_takes_a_schedule_or_one_shape_per_rollout(shape):
    """with a valid tensor the stub is reached: the checks passed and the first engine call fails for lack of an engine"""
    with pytest.raises(AttributeError, match="set_trajectory_start"):
        call(torch.zeros(shape))


def test_sim_rollout_takes_the_episode_length_from_the_shape_schedule():
    with pytest.raises(AttributeError, match="set_trajectory_start"):
        call(torch.zeros(TAPE, B, P, 8), actions=False)
    with pytest.raises(ValueError, match="steps"):
        call(torch.zeros(B, P, 8), actions=False)              # constant shapes say nothing about the length
    with pytest.raises((RuntimeError, ValueError), match="tape"):
        call(torch.zeros(TAPE + 1, B, P, 8), actions=False)
    with pytest.raises(ValueError, match="steps"):
        call(torch.zeros(TAPE, B, P, 8), actions=False, steps=TAPE - 1)     # steps= contradicts the schedule's length


@pytest.mark.parametrize("shape", [(TAPE, B, P, 7), (TAPE - 1, B, P, 8), (TAPE, B, P + 1, 8), (TAPE, B, G, 8), (B + 1, P, 8), (B, P * 8), (P, 8)])
def test_sim_rollout_refuses_wrong_shape_shapes(shape):
    with pytest.raises(ValueError, match="shape.*primitive_shapes"):
        call(torch.zeros(shape))


def test_sim_rollout_refuses_shapes_of_another_dtype_or_device():
    with pytest.raises(ValueError, match="dtype"):
        call(torch.zeros(B, P, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match="device"):
        call(torch.zeros(B, P, 8, device="meta"))
    with pytest.raises(ValueError, match="must be a torch tensor"):
        call(np.zeros((B, P, 8)))


def test_sim_rollout_refuses_shapes_that_require_grad_and_says_why():
    ps = torch.zeros(TAPE, B, P, 8, requires_grad=True)
    with pytest.raises(ValueError, match=r"adjoint.*does not see an obstacle's shape.*\.detach\(\)"):
        call(ps)
    with pytest.raises(AttributeError, match="set_trajectory_start"):      # detached, as the message advises
        call(ps.detach())


def test_sim_rollout_without_shapes_needs_no_primitive_count():
    """an engine object without `nprims` still runs an episode that passes no shapes; with shapes, the missing count is what fails"""
    sim = stub_sim(nprims=None)
    with pytest.raises(AttributeError, match="set_trajectory_start"):
        call(None, sim=sim)
    with pytest.raises(AttributeError, match="nprims"):
        call(torch.zeros(B, P, 8), sim=sim)


# ---- the one conversion, as dc_build and the host setters compile it ---------------------------------------------------------------
def test_primitive_to_row_to_device_fields(tmp_path):
    """csrc/dc_primshape.h (tests/native/prim_shapes_check.cpp): the row is the dc_primitive fields of the same names, each rounded once, lands
    in the shape fields of the device primitive and nowhere else, and a row given by a caller equals what dc_build stores"""
    csrc = os.path.join(ROOT, "diffcloth_amd", "csrc")
    exe = str(tmp_path / "prim_shapes_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "native", "prim_shapes_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ALL OK"), r.stdout + r.stderr


def test_build_and_setters_share_the_one_conversion():
    """dc_build's DevPrim fill and the host setters call dc_primshape.h; dc_build no longer casts the shape fields itself"""
    src = open(os.path.join(ROOT, "diffcloth_amd", "csrc", "dc_engine.hip")).read()
    assert '#include "dc_primshape.h"' in src
    assert "primitive_shape_to_prim(q, d)" in src and "round_shape_row(in, out)" in src
    assert "(float) q.radius" not in src and "(float) q.top_offset" not in src and "(float) q.corner2" not in src
