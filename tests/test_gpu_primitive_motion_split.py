"""Obstacle motion tables (centres, velocities w, spins omega, shapes) on the kernels the four obstacle test files never hold to the oracle:
the SPLIT kernels (k_pd_step_cl, k_adjoint_step_cl_moving: K workgroups per rollout, dL/dw and dL/domega summed across the parts), both
block-preconditioner values of the moving adjoint instances, the deflated / coarse-level split instances, and the fp64 BiCGSTAB fall-back.

Scenes, partner and gates are those of tests/test_gpu_primitive_velocities.py (pv) and tests/test_gpu_primitive_spins.py (ps), whose helpers
this file imports: the fp64 oracle's static / `rotates` sphere in the frame that moves at w, every step teacher-forced from the ORACLE's state,
so the oracle side of a scene does not depend on the engine and is computed once (functools.lru_cache) for every K and switch value. B = 3
rollouts (b0: w = 0, b1 and b2 moving; pv.W1[:3], pv.D1[:3], dyadic), 2 steps, h = 1/180, spheres of radius 2 with mu 0.4.

Mesh: the 29 x 29 grid (N = 841). A forced DC_CLUSTER waives the plan's 256-rows-per-part rule, so the smallest grid is not the 48 x 48 one
the engine splits by itself. Meshes of up to 768 vertices (28 x 28 and smaller) are served by the explicit-inverse kernels and never split
unless forced; of the larger ones 28 x 28 is the first (ClusterPlan::fit accepts K = 2 and 4 from there on), and with the scenes as they stand
it fails condition 3 below (the static group of split_rotating_two has its step-1 contacts of K = 4 in one part); 29 x 29 holds all of them.
The parts are uneven there: K = 2 gives R = 448 rows per part (448 + 393), K = 4 gives R = 256 (256 + 256 + 256 + 73), halo 64 rows; the
bandwidth (57) is far under the renumbering rule, so vertex i belongs to part i // R (asserted). K = 8 is refused on this mesh
(7 x round64(ceil(841 / 8)) = 896 >= 841: a part would be empty), so there is no K = 8 case. The deflated split FORWARD instances exist for
packet shapes of 512 threads x >= 4 rows only (more than 1536 vertices, csrc/dc_kernelplan.h: kPkShapes), so the deflation test alone runs
the same base scene on the 40 x 40 grid (N = 1600, the smallest such grid; K = 4: R = 448).

Conditions a scene has to satisfy, checked on the oracle alone (CPU) before the engine is touched (check_scene_conditions):
  1. every reachable group has >= 10 contacts per step and rollout, an unreachable one none; b1 has sticking AND sliding contacts in at least
     one step (the rule of pv.check_base_scene_is_not_vacuous);
  2. for K = 2 and 4 the contact vertices of every reachable group lie in at least two parts, in every rollout and step;
  3. the oracle's per-vertex terms c_i (pv.Scene.expected_dw) summed over ANY single part miss the full sum by more than 10 x the dL/dw gate
     (1e-4 sum |c_i|), and the same for radius n_i x c_i and dL/domega: a wrong cross-part sum cannot pass;
  4. without the term the step misses the oracle by more than 100 x GATE_X on b1 and b2: measured on the oracle alone (its static sphere fed
     the engine's frame-shifted state; its static against its rotating sphere from the same state) and on the split engine with the table unset.
The file fixes no number of its own: pv.GATE_X forward, ps.GATE_B = 1e-4 backward (end to end, the engine's record adopted by the oracle, the
oracle's record injected), ps.DW_RTOL for dL/dw and dL/domega. Every backward step asserts dc_bwd_stats::workgroups == K.

Measured on an MI355X, K = 4, worst over the three rollouts per step (dx = max|x - w h - x_oracle|; e2e / adopted / injected = the three
gradient statements; dL/dw, dL/domega as |diff| / sum |c_i|; PD iteration counts equal to the oracle's in every rollout and step):
  split_base          step 0: contacts 64 / 93 / 64,    dx 1.2e-7, e2e 1.8e-6, adopted 1.2e-6, injected 3.0e-8, dL/dw 1.8e-7
                      step 1: contacts 64 / 93 / 64,    dx 1.2e-7, e2e 1.6e-6, adopted 3.1e-7, injected 3.0e-7, dL/dw 5.3e-7
  split_three_groups  step 0: contacts 123 / 170 / 123, dx 1.2e-7, e2e 1.7e-5, adopted 3.0e-6, injected 4.6e-7, dL/dw 6.5e-7
                      step 1: contacts 124 / 171 / 124, dx 1.2e-7, e2e 5.2e-5 (dL_dmu), adopted 2.1e-6, injected 3.1e-7, dL/dw 4.8e-7
  split_rotating      step 0: contacts 79 / 106 / 79,   dx 1.2e-7, e2e 3.1e-7, adopted 4.3e-8, injected 5.3e-7, dL/dw 1.2e-8, dL/domega 2.0e-8
                      step 1: contacts 75 / 106 / 75,   dx 1.2e-7, e2e 2.9e-7, adopted 1.4e-7, injected 3.4e-7, dL/dw 2.9e-7, dL/domega 5.4e-7
  split_rotating_two  step 0: contacts 155 each,        dx 1.2e-7, e2e 6.5e-7, adopted 1.5e-7, injected 5.3e-7, dL/dw 1.1e-8, dL/domega 2.7e-8
                      step 1: contacts 144 each,        dx 1.2e-7, e2e 3.6e-6, adopted 1.3e-7, injected 3.7e-6, dL/dw 8.8e-7, dL/domega 1.8e-6
K = 2 stays inside the same bounds (worst: e2e 5.0e-5 on three groups, dL/dw 6.6e-7, dL/domega 1.3e-6). Deflated (40 x 40): dx 1.2e-7, e2e 4.6e-5, adopted 9.9e-6,
injected 8.9e-7, dL/dw 1.1e-6. The oracle's single-part sums miss by >= 100 gates (121 / 161 / 209 / 100 / 149 per scene). Without the term:
velocities unset 7.1e-3 ... 8.0e-3 on b1 and b2 (oracle alone: the same figures; b0 5.9e-8), spins unset 8.3e-3 ... 1.04e-2 in every rollout
and step (oracle alone: the same), against 100 x GATE_X = 5e-3. No end-to-end sample exceeded 1e-4: the sensitivity rule of DESIGN section 5
is not used and nothing is added to the ledger. DC_BLOCK_PRE=0 / 1 on the split scene: 28 CG iterations / 15 BiCGSTAB iterations per solve.
"""
import functools

import numpy as np
import pytest
import torch          # before the engine's library: both must share ONE HIP runtime (torch's), see tests/test_gpu_functional.py

import orc
import test_gpu_primitive_spins as ps
import test_gpu_primitive_velocities as pv          # Scene, make_engine, step helpers and gates (helpers, not tests)

pytestmark = pytest.mark.gpu
H, GATE_X, f32 = pv.H, pv.GATE_X, pv.f32
NX, NX_DEFL = 29, 40
NB, STEPS = 3, 2
W3, D3 = pv.W1[:NB], pv.D1[:NB]
SCENES = ("split_base", "split_three_groups", "split_rotating", "split_rotating_two")
REACHABLE = {"split_base": (0,), "split_base_defl": (0,), "split_three_groups": (0, 1), "split_rotating": (0,), "split_rotating_two": (0, 1)}


@functools.lru_cache(maxsize=None)
def scene(name):
    kw = dict(nx=NX_DEFL if name == "split_base_defl" else NX, threads=16)
    if name in ("split_base", "split_base_defl"):          # one group; b0 has w = 0, b1 and b2 move
        return pv.Scene([((0, 0, 0), 0)], W3, D3, steps=STEPS, **kw)
    if name == "split_three_groups":
        # two spheres side by side under the cloth, both moving at the rollout's w (what the Galilean partner needs), a third 6 below that nothing
        # touches, with another velocity. b1's two spheres stand at the offset of pv.D1's b1 relative to b0, so that b1 slides as well as sticks
        D = np.zeros((NB, 3, 3))
        D[1, :2] = D3[1, 0] - D3[0, 0]
        return pv.Scene([((-1.0, 0.125, 0), 0), ((1.0, 0.125, 0), 0), ((0, -6, 0), 0)], np.concatenate([W3, W3, W3[::-1]], axis=1), D, steps=STEPS, **kw)
    if name == "split_rotating":
        return ps.LandingScene([((0, 0, 0), 1)], W3, D3, steps=STEPS, **kw)
    if name == "split_rotating_two":                       # group 0 rotates, group 1 beside it does not; both reachable
        return ps.LandingScene([((-1.0, 0.125, 0), 1), ((1.0, 0.125, 0), 0)], np.concatenate([W3, W3], axis=1), np.zeros((NB, 2, 3)), steps=STEPS, **kw)
    raise KeyError(name)


def rows_per_part(N, K):
    """ClusterPlan::fit with one element window per part: rows of a part = ceil(N / K) rounded up to a multiple of 64"""
    return 64 * -(-(-(-N // K)) // 64)


def spins_of(sc):
    """[B][G][3] for a scene the oracle rotates a sphere of, else None (no spin table: the velocity table alone)"""
    return ps.spins_for(sc) if any(rot for _, rot in sc.spheres) else None


def static_oracle(sc, b):
    """the oracle of rollout b with every sphere STATIC (no rotates flag), at the same fp32 centres"""
    o = orc.Oracle(sc.V, sc.F, h=H, fwd_tol=1e-9, bwd_tol=1e-9, selfcollision=False, gradient_clipping=False, threads=16, **pv.FABRIC)
    for g, (c, rot) in enumerate(sc.spheres):
        o.add_sphere(f32(c + sc.D[b, g]), sc.prims[g]["radius"], sc.prims[g]["mu"], rotates=False)
    o.build()
    return o


@functools.lru_cache(maxsize=None)
def oracle_miss_without_the_term(name):
    """[steps][B] max|x - x_ref| of the oracle's own step WITHOUT the term from the same state: for a rotating scene its static spheres in the
    moving frame; else its static sphere fed the engine's state (x, v + w) as a step that ignores w would see it, shifted back by w h"""
    sc = scene(name)
    rotating = spins_of(sc) is not None
    miss = np.zeros((sc.steps, sc.nb))
    for b in range(sc.nb):
        o = static_oracle(sc, b)
        wt = np.tile(sc.wf[b], sc.N)
        for s in range(sc.steps):
            r = o.step(sc.Xe[s, b], sc.Ve[s, b] - wt) if rotating else o.step(sc.Xe[s, b], sc.Ve[s, b])
            miss[s, b] = np.abs(r["x"] - (0.0 if rotating else 1.0) * wt * H - sc.ref[s][b]["x"]).max()
    return miss


@functools.lru_cache(maxsize=None)
def check_scene_conditions(name):
    """conditions 1 - 3 of the module docstring, on the oracle alone; returns the smallest single-part miss in units of the gate"""
    sc = scene(name)
    reach = REACHABLE[name]
    both, worst = False, np.inf
    for s in range(sc.steps):
        ty = sc.ref[s][1]["pc"]["type"]
        both = both or ((ty == 1).sum() > 0 and (ty == 2).sum() > 0)
        for b in range(sc.nb):
            pc = sc.ref[s][b]["pc"]
            want, ci = sc.expected_dw(s, b)
            dom = ps.expected_dom(sc, s, b)
            for g in range(sc.G):
                sel = pc["prim"] == g
                ids = pc["particle"][sel]
                if g not in reach:
                    assert len(ids) == 0 and want[g][1] == 0.0, (name, s, b, g)
                    continue
                assert len(ids) >= 10, (name, s, b, g, len(ids))                                    # 1.
                gate = ps.DW_RTOL * want[g][1]
                cn = sc.prims[g]["radius"] * np.cross(pc["normal"][sel], ci[ids])
                for K in (2, 4):
                    part = ids // rows_per_part(sc.N, K)
                    assert len(np.unique(part)) >= 2, (name, s, b, g, K, np.unique(part))         # 2.
                    for p in range(K):                                                              # 3.
                        mw = np.linalg.norm(ci[ids][part == p].sum(axis=0) - want[g][0])
                        mo = np.linalg.norm(cn[part == p].sum(axis=0) - dom[g][0])
                        assert mw > 10 * gate and mo > 10 * gate, (name, s, b, g, K, p, mw / gate, mo / gate)
                        worst = min(worst, mw / gate, mo / gate)
    assert both, name
    return worst


def split_engine(sc, K, monkeypatch, mode=1):
    """the scene's PLAIN spheres (a spin comes through dc_set_primitive_spins), pv's tight solver settings, K workgroups per rollout"""
    monkeypatch.setenv("DC_CLUSTER", str(K))
    e = pv.make_engine(sc.V, sc.F, ps.plain_prims(sc), att=sc.att, mode=mode, cg_max_iter=3000)
    sc.m3 = pv.mass3(e)
    ps.start(sc, e, spins_of(sc))
    assert e.cluster() == K
    assert not e.layout()["renumbered"]                                  # vertex i belongs to part i // R
    assert e.cluster_rows()[0] == rows_per_part(sc.N, K) and e.cluster_rows()[1] >= 64
    return e


def run_split_parity(name, sc, e, K, lines, steps=None, pd_iters=True, inject=True):
    """the loop of ps.run_parity (the same helpers, the same gates) with the workgroup count of every backward step asserted"""
    om = spins_of(sc)
    for s in range(sc.steps if steps is None else steps):
        got = pv.forward_step(sc, e, s)
        np.testing.assert_array_equal(e.get_primitive_velocities(s + 1), f32(sc.W))
        if om is not None:
            np.testing.assert_array_equal(e.get_primitive_spins(s + 1), f32(om))
        pv.check_forward(sc, got, s, lines)
        if pd_iters:
            for b in range(sc.nb):
                assert abs(int(got["st"]["pd_iters"][b]) - sc.ref[s][b]["iters"]) <= 1, lines[-sc.nb + b]
        for is_start in (s % 2, 1 - s % 2):
            gb, _ = pv.check_backward(sc, e, got, s, is_start, lines, gate=ps.GATE_B)
            assert np.all(gb["workgroups"] == K), (gb["workgroups"], K)
            assert np.all(gb["converged"] == 1), gb["converged"]
            lines.append(f"    workgroups {gb['workgroups'].tolist()} adjoint iterations {gb['adjoint_iters'].tolist()} CG iterations {gb['cg_iters'].tolist()}")
            if is_start and om is not None:
                ps.check_dom(sc, e.get_primitive_spin_gradients(s + 1, 1)[0], s, lines)
        if inject:
            if om is not None:
                e.set_primitive_spin_schedule(s, om[None])
            pv.check_injected(sc, e, s, s % 2, lines)
            assert np.all(e.get_stats(s + 1)[1]["workgroups"] == K)
            if s % 2 and om is not None:
                ps.check_dom(sc, e.get_primitive_spin_gradients(s + 1, 1)[0], s, lines, tag="injected ")


def parity_case(name, K, monkeypatch, tag="", **kw):
    margin = check_scene_conditions(name)
    sc = scene(name)
    e = split_engine(sc, K, monkeypatch)
    lines = [f"smallest single-part miss of dL/dw, dL/domega on the oracle: {margin:.0f} x the gate"]
    try:
        run_split_parity(name, sc, e, K, lines, **kw)
    finally:
        print(f"\n[motion tables, split K={K}, scene {name}{tag}, N={sc.N}, R={e.cluster_rows()[0]}]\n" + "\n".join(lines))
        e.close()


# ---- 1. split parity under motion ----
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("K", [2, 4])
def test_split_parity_under_motion(K, name, monkeypatch):
    parity_case(name, K, monkeypatch)


# ---- condition 4: without the term the split step misses the oracle ----
@pytest.mark.parametrize("name", ["split_base", "split_rotating"])
def test_without_the_term_the_split_step_misses_the_oracle(name, monkeypatch):
    """K = 4 counterparts of pv.test_the_scene_can_see_the_term (velocities unset) and ps.test_without_the_spin_the_step_misses_the_oracle (spins
    unset); the same miss measured on the oracle alone first"""
    check_scene_conditions(name)
    sc = scene(name)
    rotating = spins_of(sc) is not None
    alone = oracle_miss_without_the_term(name)
    moving = (0, 1, 2) if rotating else (1, 2)          # (a spin acts on every rollout, a velocity on those that have one)
    lines = [f"oracle alone, step {s} rollout {b}: {alone[s, b]:.2e}" for s in range(sc.steps) for b in range(sc.nb)]
    try:
        for s in range(sc.steps):
            for b in moving:
                assert alone[s, b] > 100 * GATE_X, (s, b, alone[s, b])
        monkeypatch.setenv("DC_CLUSTER", "4")
        e = pv.make_engine(sc.V, sc.F, ps.plain_prims(sc), cg_max_iter=3000)
        ps.start(sc, e, None, velocities=rotating)      # the table under test stays unset
        assert e.cluster() == 4
        for s in range(sc.steps):
            got = pv.forward_step(sc, e, s)
            for b in range(sc.nb):
                miss = np.abs(got["x"][b] - np.tile(sc.wf[b], sc.N) * H - sc.ref[s][b]["x"]).max()
                lines.append(f"split engine K=4, step {s} rollout {b}: without the term max|x - w h - x_oracle| {miss:.2e}")
                if b in moving:
                    assert miss > 100 * GATE_X, lines[-1]
                else:
                    assert miss <= GATE_X, lines[-1]
        e.close()
    finally:
        print(f"\n[motion tables, split K=4, scene {name}, the term unset]\n" + "\n".join(lines))


# ---- 2. both block-preconditioner values of the moving adjoint instances, both families ----
@pytest.mark.parametrize("block_pre", ["0", "1"])
def test_block_preconditioner_values_split(block_pre, monkeypatch):
    """DC_BLOCK_PRE is read at every backward step: k_adjoint_step_cl_moving with and without the block preconditioner"""
    monkeypatch.setenv("DC_BLOCK_PRE", block_pre)
    parity_case("split_base", 4, monkeypatch, tag=f", DC_BLOCK_PRE={block_pre}")


@pytest.mark.parametrize("block_pre", ["0", "1"])
def test_block_preconditioner_values_one_workgroup(block_pre, monkeypatch):
    """the one-workgroup moving instances on pv's 17 x 17 base scene: adjoint mode 1, two steps, backward and injected checks"""
    monkeypatch.setenv("DC_BLOCK_PRE", block_pre)
    pv.run_parity("base", mode=1, steps=2)


# ---- 3. the deflated split forward kernel and the coarse-level split adjoint instance ----
def test_deflated_split_instances(monkeypatch):
    """DC_DEFLATION=1 at dc_build: 16 vectors; the 40 x 40 grid has the packet shape (512 threads x 4 rows) the deflated forward instances exist
    for, and cl_adjoint_choice takes the coarse-level twin whenever a space exists. Projection changes the PD / PCG iteration counts: not asserted."""
    monkeypatch.setenv("DC_DEFLATION", "1")
    name, K = "split_base_defl", 4
    margin = check_scene_conditions(name)
    sc = scene(name)
    e = split_engine(sc, K, monkeypatch)
    lines = [f"smallest single-part miss on the oracle: {margin:.0f} x the gate"]
    try:
        assert e.deflation()[0] == 16
        run_split_parity(name, sc, e, K, lines, pd_iters=False)
    finally:
        print(f"\n[motion tables, split K={K}, deflated, N={sc.N}, R={e.cluster_rows()[0]}]\n" + "\n".join(lines))
        e.close()


# ---- 4. the fp64 BiCGSTAB fall-back with motion ----
@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("which", ["base", "rotating"])
def test_fp64_fallback_with_motion(which, mode, monkeypatch):
    """DC_DENSE_FLAG=1 marks rollout 1 (the one with sticking and sliding contacts) as if its factorisation had failed: bicgstab64 from u = 0
    through apply_K64 / contact_JT_d with the w and omega terms; the other rollouts take the direct solve. 17 x 17 scenes of pv and ps."""
    monkeypatch.setenv("DC_DENSE_FLAG", "1")
    sc = pv.scene("base") if which == "base" else ps.scene("rotating")
    om = ps.spins_for(sc) if which == "rotating" else None
    e = pv.make_engine(sc.V, sc.F, ps.plain_prims(sc), mode=mode)
    sc.m3 = pv.mass3(e)
    ps.start(sc, e, om)
    lines = []
    try:
        for s in range(2):
            got = pv.forward_step(sc, e, s)
            pv.check_forward(sc, got, s, lines)
            for is_start in (s % 2, 1 - s % 2):
                gb, _ = pv.check_backward(sc, e, got, s, is_start, lines, gate=ps.GATE_B)
                lines.append(f"    fp64 iterations {gb['fp64_iters'].tolist()} refine cycles {gb['refine_cycles'].tolist()} used_direct {gb['used_direct'].tolist()}")
                assert gb["fp64_iters"][1] > 0 and gb["refine_cycles"][1] == 0 and gb["converged"][1] == 1, lines[-1]
                others = [b for b in range(sc.nb) if b != 1]
                assert np.all(gb["fp64_iters"][others] == 0) and np.all(gb["used_direct"][others] == mode), lines[-1]
                if is_start and om is not None:
                    ps.check_dom(sc, e.get_primitive_spin_gradients(s + 1, 1)[0], s, lines)
    finally:
        print(f"\n[motion tables, fp64 fall-back, scene {which}, adjoint_mode {mode}]\n" + "\n".join(lines))
        e.close()


# ---- 6. given = built on the split path, bit for bit ----
def test_offset_velocity_shape_and_spin_together_equal_the_moved_build_split(monkeypatch):
    """K = 4 counterpart of tests/test_gpu_primitive_shapes.py::test_offset_velocity_and_shape_together_equal_the_moved_build: rollout b of a
    context GIVEN an offset, a velocity, a shape row (another radius) and a spin against rollout b of a context BUILT at the moved centre with
    that radius and given the same velocity — two fused steps and the backward sweep, everything they leave behind, with assert_array_equal.

    The spin of the built context: include/diffcloth_hip.h defines v_spin = radius_p (omega x n) with the BUILT radius of the sphere, whatever
    its shape row says. With the SAME omega the two contexts therefore do not describe one obstacle once the radius is changed (measured on an
    MI355X with radii 2.125 / 2.25 / 2.19 given to a sphere built with 2.0: states 3e-7 apart after one step, on 16 % of the coordinates — the
    contacts slide, so only the direction of the friction force sees the surface speed). The identity that holds under that rule, and bit for
    bit, is: built radius R_A, given radius R_A / 2^k and omega, against built radius R_A / 2^k and 2^k omega — a power of two scales every
    intermediate of (omega x n) radius exactly. It pins the rule itself on the split path: the shape row moves the geometry, the built radius
    carries the spin. dL/domega of the given context is then 2^k times the built context's (d omega_built / d omega = 2^k), exactly."""
    K = 4
    monkeypatch.setenv("DC_CLUSTER", str(K))
    sc = scene("split_base")                                             # (its mesh and sphere centre; no oracle is involved)
    N = sc.N
    c = np.asarray(sc.prims[0]["center"], dtype=np.float64)
    R_A = 4.5 + 2e-9                                                     # (no fp32 number, nor are its halves: the rounding happens once)
    scale = np.array([2.0, 4.0, 2.0])
    radii = R_A / scale                                                  # 2.25, 1.125 (its centre 1 higher: the same top), 2.25
    D = np.array([[[0.0, 0.0625, 0.0]], [[0.125, 1.03125 + 1e-9, -0.0625]], [[-0.0625, 0.125, 0.03125]]])
    W = W3 * 0.25
    OM = np.array([[[0.0, 2.0, 0.0]], [[0.5, -1.0, 0.25]], [[0.0, 0.0, 0.0]]])
    X0 = np.tile(f32(sc.V.reshape(-1)), (NB, 1))
    V0 = np.stack([f32(np.tile(W[b, 0], N)) for b in range(NB)])
    rng = np.random.default_rng(12)
    gx = f32(rng.standard_normal((NB, 3 * N))); gv = f32(0.01 * rng.standard_normal((NB, 3 * N)))

    def run(prims, om, shapes=None, offsets=None):
        e = pv.make_engine(sc.V, sc.F, prims, cg_max_iter=3000)
        e.alloc_batch(NB, STEPS)
        assert e.cluster() == K
        if shapes is not None:
            SH = np.tile(e.built_primitive_shapes()[None], (NB, 1, 1))
            SH[:, 0, 6] = shapes
            e.set_primitive_shapes(SH)
        if offsets is not None:
            e.set_primitive_offsets(offsets)
        e.set_primitive_velocities(W)
        e.set_primitive_spins(om)
        e.set_state(0, X0, V0)
        e.rollout_forward(0, STEPS)
        out = pv.collect(e, STEPS)
        out["centres"] = np.stack([e.get_primitive_centers(s + 1) for s in range(STEPS)])
        out["contacts"] = np.stack([e.get_stats(s + 1)[0]["prim_contacts"] for s in range(STEPS)])
        e.set_gradient(gx, gv)
        e.rollout_backward(STEPS, STEPS)
        out["dx"], out["dv"], out["dmu"] = e.get_gradient()
        out["dw"], out["dom"] = e.get_primitive_velocity_gradients(1, STEPS), e.get_primitive_spin_gradients(1, STEPS)
        out["wg"] = np.stack([e.get_stats(s + 1)[1]["workgroups"] for s in range(STEPS)])
        e.close()
        return out

    given = run([dict(pv.sphere(c), radius=R_A)], OM, shapes=radii, offsets=D)
    assert np.all(given["wg"] == K) and given["contacts"].min() >= 10, (given["wg"], given["contacts"])
    assert np.abs(given["dw"][:, 1:]).max() > 0 and np.abs(given["dom"]).max() > 0
    differ = []

    def cmp(a, b_, what):
        if not np.array_equal(a, b_):
            differ.append(f"{what}: {int((np.asarray(a) != np.asarray(b_)).sum())} of {np.asarray(a).size} values, max |diff| "
                          f"{np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b_, dtype=np.float64)).max():.2e}")

    for b in range(NB):
        built = run([dict(pv.sphere(c + D[b, 0]), radius=float(radii[b]))], OM * scale[b])
        cmp(given["centres"][:, b, 0], np.broadcast_to(f32(c + D[b, 0]), (STEPS, 3)), f"rollout {b} centre")
        for key in ("x", "v", "centres", "contacts", "dw", "wg"):
            cmp(given[key][:, b], built[key][:, b], f"rollout {b} {key}")
        cmp(given["dom"][:, b], built["dom"][:, b] * scale[b], f"rollout {b} dom")
        for key in ("grp", "nrm", "f", "r"):
            for s in range(STEPS):
                cmp(given[key][s][b], built[key][s][b], f"rollout {b} step {s} {key}")
        for key in ("dx", "dv", "dmu"):
            cmp(given[key][b], built[key][b], f"rollout {b} {key}")
    assert not differ, "\n".join(differ)
