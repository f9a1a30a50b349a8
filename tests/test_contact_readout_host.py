"""Host-side checks of the contact read-out (dc_get_contact_readout, dc_get_contact_readout_dev, Engine.contact_readout / contact_readout_dev,
BatchedSim.contact_readout) and the oracle-only conditions of the scenes tests/test_gpu_contact_readout.py compares on. No device is touched:
the C entries are called on a host-only context, the Python wrappers on stubs that have sizes but no library.
"""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import contact_readout_scenes as cs
import meshes
from diffcloth_amd import capi
from diffcloth_amd.functional import BatchedSim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DC_ERR_INVALID, DC_ERR_STATE = 1, 3


def header():
    return open(os.path.join(ROOT, "include", "diffcloth_hip.h")).read()


def test_entries_are_exported_with_the_stated_signatures():
    lib = capi.load_library()
    flat = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert "int dc_get_contact_readout(dc_ctx *ctx, int slot0, int nslots, int *state , double *normal_impulse , double *wrench );" in flat
    assert ("int dc_get_contact_readout_dev(dc_ctx *ctx, int slot0, int nslots, void *d_state , void *d_normal_impulse , void *d_wrench , "
            "int is_f32);") in flat
    for name in ("dc_get_contact_readout", "dc_get_contact_readout_dev"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert hasattr(capi.Engine, "contact_readout") and hasattr(capi.Engine, "contact_readout_dev") and hasattr(BatchedSim, "contact_readout")


def test_header_states_the_rule():
    h = header()
    doc = h[h.index("Contact read-out: what the obstacles feel"):h.index("int dc_get_contact_readout(")]
    assert "0 = vertex i not in primitive contact, 1 = take-off, 2 = stick, 3 = slide" in doc and "CollisionType + 1" in doc
    assert "sd = d.n >= 0 -> take-off, else |dT| <= mu |sd| -> stick, else slide" in doc
    assert "J / time_step" in doc and "FIRST" in doc and "bit-reproducible" in doc and "no derivative" in doc
    assert "dc_set_record" in doc and "DC_ERR_INVALID" in doc


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
    p, i = C.c_void_p(buf.ctypes.data), C.c_int
    forms = (("dc_get_contact_readout", ()), ("dc_get_contact_readout_dev", (i(1),)))
    for name, extra in forms:
        fn = getattr(lib, name)
        for args, msg in (((i(0), i(1), p, p, p), "slot 0 has no record"), ((i(-1), i(1), p, p, p), "slot 0 has no record"), ((i(1), i(0), p, p, p), "nslots < 1"),
                          ((i(1), i(1), None, None, None), "all null")):
            assert fn(h, *args, *extra) == DC_ERR_INVALID, (name, msg)
            assert msg in lib.dc_last_error(h).decode()
        # well-formed arguments: no device, no batch — refused as the neighbouring getters refuse it
        assert fn(h, i(1), i(1), p, p, p, *extra) == DC_ERR_STATE, name
        assert lib.dc_get_states_dev(h, i(1), i(1), p, p, i(1)) == DC_ERR_STATE
        assert len(lib.dc_last_error(h)) > 0
    assert np.all(buf == 0)
    e.close()


def test_wrench_without_a_primitive_group_is_refused_before_the_batch_is_looked_at():
    e = capi.Engine(device=-1)
    V, F = meshes.grid_cloth(5, 5, 4.5, 4.5, "DOWN")
    e.set_mesh(V, F)
    e.set_primitives([])
    e.build()
    buf = np.zeros(8)
    p, i = C.c_void_p(buf.ctypes.data), C.c_int
    assert e.lib.dc_get_contact_readout(e.h, i(1), i(1), p, p, p) == DC_ERR_INVALID
    assert "no primitive group" in e.lib.dc_last_error(e.h).decode()
    assert e.lib.dc_get_contact_readout_dev(e.h, i(1), i(1), None, None, p, i(0)) == DC_ERR_INVALID
    assert e.lib.dc_get_contact_readout(e.h, i(1), i(1), p, p, None) == DC_ERR_STATE          # without the wrench: the host-only refusal
    e.close()


# ---- the Python wrappers check their arguments before anything reaches the library ----
B, N, G, TAPE = 2, 5, 2, 3


def stub_engine():
    e = capi.Engine.__new__(capi.Engine)
    e.B, e.N, e.ngroups, e.tape, e.device, e.h = B, N, G, TAPE, 0, None      # sizes only: a call that reached the library would raise AttributeError
    return e


def test_capi_wrappers_check_their_arguments():
    e = stub_engine()
    with pytest.raises(ValueError, match="slot 0"):
        e.contact_readout(0, 1)
    with pytest.raises(ValueError, match="nslots"):
        e.contact_readout(1, 0)
    with pytest.raises(ValueError, match="nothing asked for"):
        e.contact_readout(1, 1, state=False, normal_impulse=False, wrench=False)
    with pytest.raises(ValueError, match="nothing asked for"):
        e.contact_readout_dev(1, 1)
    with pytest.raises(ValueError, match="int32"):
        e.contact_readout_dev(1, 1, state=torch.zeros((1, B, N), dtype=torch.int64))
    with pytest.raises(ValueError, match="CUDA"):
        e.contact_readout_dev(1, 1, normal_impulse=torch.zeros((1, B, N)))
    with pytest.raises(AttributeError):                      # valid arguments reach the (missing) library
        e.contact_readout(1, 2)


def test_batched_sim_checks_its_arguments():
    sim = BatchedSim.__new__(BatchedSim)
    sim.engine = types.SimpleNamespace(B=B, N=N, ngroups=G, tape=TAPE, device=0)
    sim.step_num, sim.step_idx, sim._stream = TAPE, 2, None
    with pytest.raises(ValueError, match="slot 0"):
        sim.contact_readout(0)
    with pytest.raises(ValueError, match="taken 2 step"):
        sim.contact_readout(1, 3)
    with pytest.raises(ValueError, match="taken 2 step"):
        sim.contact_readout(3)
    with pytest.raises(ValueError, match="dtype"):
        sim.contact_readout(1, 1, dtype=torch.float16)
    with pytest.raises(ValueError, match="nothing asked for"):
        sim.contact_readout(1, 1, state=False, normal_impulse=False, wrench=False)
    assert "NO gradient" in BatchedSim.contact_readout.__doc__


# ---- oracle-only conditions of the GPU file's scenes ----
@pytest.mark.parametrize("name", cs.STATE_SCENES)
def test_state_scenes_hold_every_kind_of_contact_outside_the_margin(name):
    sc = cs.scene(name)
    c = sc.census(cs.MARGIN_RECORD)
    wide = sc.census(cs.MARGIN_STEP)
    print(f"\n[{name}] {c}; inside MARGIN_STEP = {cs.MARGIN_STEP}: {wide['unsafe']} of {wide['contacts']}")
    assert all(sc.ref[s][b]["converged"] for s in range(sc.steps) for b in range(sc.nb))
    assert c["stick"] >= 5 and c["slide"] >= 5 and c["takeoff"] >= 1, c
    assert c["unsafe"] <= cs.MAX_UNSAFE_SHARE * c["contacts"], c
    # the state comparison on an own record still sees every kind
    kinds = np.zeros(4, dtype=int)
    for s in range(sc.steps):
        for b in range(sc.nb):
            ex = sc.expected(s, b)
            kinds += np.bincount(ex["state"][ex["safe_step"]], minlength=4)
    assert np.all(kinds[1:] >= 5), kinds
    # what prim_contacts reports is the friction law's decision on its own d
    for s in range(sc.steps):
        for b in range(sc.nb):
            pc = sc.ref[s][b]["pc"]
            np.testing.assert_array_equal(cs.classify(pc["normal"], pc["d"], sc.mu_of(b, pc)), pc["type"] + 1)


def test_the_moving_scene_needs_the_motion_row():
    """classifying with d = f (no motion term) changes the state of at least 5 contacts of the moving and spinning scene: the GPU test can
    only pass if the kernel reads the row"""
    sc = cs.scene("moving_spinning")
    changed = 0
    for s in range(sc.steps):
        for b in range(sc.nb):
            pc, f = sc.ref[s][b]["pc"], sc.ref[s][b]["f"].reshape(-1, 3)
            changed += int(np.sum(cs.classify(pc["normal"], f[pc["particle"]], sc.mu_of(b, pc)) != pc["type"] + 1))
    assert changed >= 5, changed


def test_the_flap_scene_separates_the_primitive_part():
    """on the oracle alone: in at least one step the record's TOTAL r, summed over the vertices in primitive contact, misses the sum of the
    primitive contacts' r by more than 100 gates"""
    sc = cs.scene("flap")
    worst = 0.0
    for s in range(sc.steps):
        ref = sc.ref[s][0]
        pc = ref["pc"]
        assert ref["nself"] >= 10 and len(pc["particle"]) >= 5
        miss = np.linalg.norm(ref["r"].reshape(-1, 3)[pc["particle"]].sum(axis=0) - pc["r"].sum(axis=0))
        worst = max(worst, miss / (cs.SUM_RTOL * np.linalg.norm(pc["r"], axis=1).sum()))
    assert worst > 100, worst


def test_the_offset_schedule_moves_the_reference_point_by_100_gates():
    sc = cs.scene("offset_schedule")
    built = cs.f32(np.asarray(sc.prims[0]["center"]))
    for s in range(1, sc.steps):
        for b in range(sc.nb):
            ex, wrong = sc.expected(s, b), sc.expected(s, b, centre=[built])
            assert np.linalg.norm(wrong["rows"][0, 3:6] - ex["rows"][0, 3:6]) > 100 * cs.SUM_RTOL * ex["scales"][0, 1]
