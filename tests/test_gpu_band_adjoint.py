"""adjoint_mode 3, the banded direct adjoint solve (csrc/dc_adjoint_band.hip), through the C-ABI: the scenes, the oracle's sparse-LU chain
and the gates of tests/test_gpu_dense_adjoint.py (mode 2), whose builders and helpers this module imports.

  1. the matrix: dc_get_adjoint_matrix under mode 3 (the band-assembled K, expanded) is held to the oracle gate of mode 2's
     test_matrix_matches_oracle on the hat (extra = 0) and on flap24 with the whole matrix as the band (kl = n - 1, where the panel kernel
     works in global memory); it has mode 2's non-zero pattern, and on flap24 with extra = 0 (not renumbered: device = caller's numbering)
     it is exactly zero outside the band. Not asserted on the hat itself: its vertices are renumbered on the device and the C-ABI does not
     hand out that permutation, so the band cannot be located in the caller's numbering; there the pattern must equal mode 2's (nothing
     lost, nothing added) and the zero-outside-band property of the getter's expansion is pinned on flap24.
     The largest difference from mode 2's matrix is printed (bitwise equality is expected, not gated).
  2. exact-solve parity: hat (extra = 0), flap24 (kl = n - 1) and a 32 x 32 cloth on the sphere (1 024 vertices, above the dense limit: mode 2
     is refused there) against the oracle's sparse-LU chain at EXACT_TOL; every step used_direct = 3, no fall-back iteration, 1 ... 3
     substitutions, fp64 residual <= 1e-10; agreement with mode 1 within GRAD_TOL.
  3. the out-of-band rule on flap24: the width every record needs is computed here from P's pattern (dc_get_system_matrix; the layout says
     the mesh is not renumbered, and its bandwidth is that pattern's) and the record's self contacts as dc_get_self_contacts returns them
     from the engine after the upload (asserted to be the oracle's pairs), in layer order: a contact (a, b) couples row i to both
     vertices as soon as it reaches one of them; with extra = 0 and
     with extra widened up to that width, a rollout-step reports the fall-back (fp64_iters > 0, no substitution) exactly when its width
     exceeds bw + extra, and its gradients still pass GRAD_TOL against the LU chain (EXACT_TOL where the factors were used).
  4. determinism and plumbing on the 10 x 10 cloth (B = 3) and flap24: bitwise run-to-run, DC_DENSE_CHUNK = 1 and 2 (a partial last chunk),
     DC_DENSE_FLAG, clipping, a zero-gradient rollout, dc_rollout_backward over 4 steps bitwise equal to the step loop.

Measured on an MI355X (12 tests, 23 s): K against the oracle hat 6.1e-14, flap24 3.5e-16 (self-contact columns 3.3e-10); the largest
difference from mode 2's matrix is 0.0 on both (bitwise equal). Against the LU chain: hat 3.8e-8, flap24 (kl = n - 1) 7.4e-7 (dL_dk; others
<= 5.5e-8), the 1 024-vertex cloth 4.2e-8; one substitution per step, residuals <= 1.3e-13; against mode 1: 3.2e-7 / 1.0e-6 / 1.2e-6.
Out-of-band rule on flap24: matrix bandwidth 47, every record needs 239;
extra = 0 and 191 flag all 8 rollout-steps, extra = 192 none; the flagged runs stay 7.4e-7 from the LU chain.
"""
import copy

import numpy as np
import pytest

import records
from diffcloth_amd import capi, workloads
from test_gpu_adjoint_options import cluster_env, f32, rel
from test_gpu_dense_adjoint import (EXACT_TOL, GRAD_TOL, MATRIX_TOL, SELF_MU_TOL, assert_bitwise, assert_direct_stats, env_var, errors, flap24, hat,  # noqa: F401
                                    lu_chain, mid, run_chain, scene, sphere_cloth)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def big():
    yield sphere_cloth(32, 32, (0.0, -0.04, 0.0))


def banded(sc, extra):
    """the scene with engines that widen the band by `extra` vertices"""
    out = copy.copy(sc)

    def make_engine(**opts):
        e = sc.make_engine(**opts)
        e.set_adjoint_band(extra)
        return e
    out.make_engine = make_engine
    return out


def assert_band_stats(gb, rollouts=None):
    """assert_direct_stats of mode 2, with used_direct = 3"""
    q = slice(None) if rollouts is None else rollouts
    assert (gb["used_direct"][q] == 3).all(), gb["used_direct"]
    g2 = dict(gb)
    g2["used_direct"] = np.where(gb["used_direct"] == 3, 2, -1)
    assert_direct_stats(g2, rollouts)


CASES = {"hat": ("hat", 0), "flap24_full": ("flap24", 10 ** 6), "big": ("big", 0)}


def case(request, name):
    fixture, extra = CASES[name]
    sc = scene(request, fixture)
    return sc, banded(sc, extra)


def matrices(sc, mode, b_list):
    e = sc.make_engine(adjoint_mode=mode)
    try:
        B = sc.MU.shape[0]
        with cluster_env(1):
            e.alloc_batch(B, 2)
        e.set_mu(sc.MU)
        s = len(sc.refs) - 1
        e.set_state(0, *sc.starts[s])
        records.upload_oracle_records(e, 1, sc.recs[s], x_fixed=None if sc.xf is None else sc.xf[s])
        return [e.adjoint_matrix(1, b) for b in b_list], e.adjoint_band(), e.layout()
    finally:
        e.close()


@pytest.mark.parametrize("name", ["hat", "flap24_full"])
def test_matrix_matches_oracle(request, name):
    sc, scb = case(request, name)
    B, s = sc.MU.shape[0], len(sc.refs) - 1
    K3, band, _ = matrices(scb, 3, range(B))
    K2, _, _ = matrices(sc, 2, range(B))
    n = K3[0].shape[0]
    assert band["kl"] == (218 if name == "hat" else n - 1)
    worst = worst_self = diff = 0.0
    for b in range(B):
        sc.o.set_mu(0, float(sc.MU[b, 0]))
        Ko = sc.o.adjoint_matrix(sc.refs[s][b]["id"]).toarray()
        selfv = np.zeros(n // 3, dtype=bool)
        selfv[sc.recs[s][b]["self"]["pairs"].reshape(-1)] = True
        cols = np.repeat(selfv, 3)
        worst = max(worst, float(np.linalg.norm(K3[b][:, ~cols] - Ko[:, ~cols]) / np.linalg.norm(Ko[:, ~cols])))
        if cols.any():
            worst_self = max(worst_self, float(np.linalg.norm(K3[b][:, cols] - Ko[:, cols]) / np.linalg.norm(Ko[:, cols])))
        diff = max(diff, float(np.abs(K3[b] - K2[b]).max()))
        assert np.array_equal(K3[b] != 0, K2[b] != 0), "mode 3's K has another non-zero pattern than mode 2's"
    print(f"[{name}] |K_band - K_oracle|_F / |K_oracle|_F: {worst:.2e}, self-contact columns {worst_self:.2e}; max |K_band - K_dense| {diff:.2e}")
    assert worst <= MATRIX_TOL and worst_self <= SELF_MU_TOL


def test_matrix_is_zero_outside_the_band(request):
    sc = scene(request, "flap24")
    K3, band, lay = matrices(banded(sc, 0), 3, [0, 1])
    K2, _, _ = matrices(sc, 2, [0, 1])
    assert not lay["renumbered"] and band["kl"] == 3 * lay["bandwidth"] + 2
    n = K3[0].shape[0]
    d = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])
    for b in range(2):
        assert not K3[b][d > band["kl"]].any()
        w = (band["kl"] - 2) // 3                      # inside the block window the two assemblies see the same couplings until one leaves it
        print(f"[flap24, extra 0] rollout {b}: non-zeros of mode 2's K outside the band {int(np.count_nonzero(K2[b][d > band['kl']]))}, vertex window {w}")


@pytest.mark.parametrize("name", sorted(CASES))
def test_exact_solve_parity_and_mode1_agreement(request, name):
    sc, scb = case(request, name)
    if name == "big":
        assert sc.starts[0][0].shape[1] == 3 * 1024
        with pytest.raises(capi.DcError) as info:
            sc.make_engine(adjoint_mode=2)
        assert "adjoint_mode 2" in str(info.value)
    got3 = run_chain(scb, sc.lu_chain, adjoint_mode=3)
    for slot, gb, _ in got3:
        print(f"[{name} mode 3] slot {slot}: refine {gb['refine_cycles'].tolist()} fp64 {gb['fp64_iters'].tolist()} last_udiff {np.array2string(gb['last_udiff'], precision=2)}")
        assert_band_stats(gb)
    w3 = errors(sc, sc.lu_chain, got3)
    print(f"[{name}] mode 3 vs the oracle's sparse LU: " + " ".join(f"{k} {v:.1e}" for k, v in w3.items()))
    assert max(w3.values()) <= EXACT_TOL
    got1 = run_chain(sc, sc.lu_chain, adjoint_mode=1)
    worst = 0.0
    for (slot, g3, p3), (_, g1, p1) in zip(got3, got1):
        for b in range(sc.MU.shape[0]):
            worst = max(worst, rel(g3["dL_dx"][b], g1["dL_dx"][b]), rel(g3["dL_dv"][b], g1["dL_dv"][b]), records.mu_err(g3["dL_dmu"][b], g1["dL_dmu"][b]))
    print(f"[{name}] mode 3 vs mode 1: {worst:.1e}")
    assert worst <= GRAD_TOL


def needed_width(P_rows, pairs, layer):
    """the vertex half-width K of a record needs: row i starts from P's pattern; a self contact (a, b), in layer order, couples the row to both
    vertices as soon as the row reaches one of them"""
    order = np.argsort(layer, kind="stable")
    width = 0
    for i, row in enumerate(P_rows):
        nz = set(row)
        for k in order:
            a, b = int(pairs[k][0]), int(pairs[k][1])
            if a in nz or b in nz:
                nz.add(a); nz.add(b)
        width = max(width, max(abs(j - i) for j in nz))
    return width


def test_out_of_band_rule(request):
    sc = scene(request, "flap24")
    steps, B = len(sc.refs), sc.MU.shape[0]
    e = sc.make_engine(adjoint_mode=1)
    try:
        lay = e.layout()
        ptr, col, _ = e.system_matrix()
        with cluster_env(1):
            e.alloc_batch(B, steps + 1)
        e.set_mu(sc.MU)
        contacts = []
        for s in range(steps):
            e.set_state(s, *sc.starts[s])
            records.upload_oracle_records(e, s + 1, sc.recs[s], x_fixed=None if sc.xf is None else sc.xf[s])
            contacts.append([e.get_self_contacts(s + 1, b) for b in range(B)])
    finally:
        e.close()
    assert not lay["renumbered"]
    bw = lay["bandwidth"]
    P_rows = [col[ptr[i]:ptr[i + 1]].tolist() for i in range(len(ptr) - 1)]
    assert bw == max(abs(j - i) for i, row in enumerate(P_rows) for j in row)
    for s in range(steps):
        for b in range(B):
            got, want = contacts[s][b], sc.recs[s][b]["self"]
            assert got["count"] == len(want["pairs"]) and got["layers"] == int(np.max(want["layer"])) + 1
            assert sorted(tuple(sorted(p)) for p in got["pairs"].tolist()) == sorted(tuple(sorted(p)) for p in np.asarray(want["pairs"]).tolist()), (s, b)
    need = np.array([[needed_width(P_rows, contacts[s][b]["pairs"], contacts[s][b]["layer"]) for b in range(B)] for s in range(steps)])
    print(f"[flap24] matrix bandwidth {bw}, width needed per (step, rollout) {need.tolist()}")
    assert need.max() > bw, "no record couples outside the matrix band: the scene does not reach the rule"
    extras = sorted({0, max(int(need.min()) - bw - 1, 0), max(int(need.min()) - bw, 0), int(need.max()) - bw - 1, int(need.max()) - bw})
    for extra in extras:
        got = run_chain(banded(sc, extra), sc.lu_chain, adjoint_mode=3)
        flagged = 0
        for slot, gb, pg in got:
            s = slot - 1
            for b in range(B):
                out = need[s, b] > bw + extra
                flagged += int(out)
                assert gb["converged"][b] == 1 and gb["used_direct"][b] == 3 and gb["residual_verified"][b] == 1
                assert (gb["fp64_iters"][b] > 0) == out and (gb["refine_cycles"][b] == 0) == out, (extra, slot, b, need[s, b], gb["fp64_iters"][b], gb["refine_cycles"][b])
                if not out:
                    assert_band_stats(gb, [b])
        w = errors(sc, sc.lu_chain, got)
        print(f"[flap24, extra {extra}] flagged rollout-steps {flagged} of {steps * B}; vs the LU chain: " + " ".join(f"{k} {v:.1e}" for k, v in w.items()))
        assert max(w.values()) <= (GRAD_TOL if flagged else EXACT_TOL)
        assert (flagged == 0) == (bw + extra >= need.max())


def test_bitwise_determinism_and_chunking(request):
    sc = banded(scene(request, "flap24"), 10 ** 6)
    a = run_chain(sc, sc.lu_chain, adjoint_mode=3)
    b = run_chain(sc, sc.lu_chain, adjoint_mode=3)
    with env_var("DC_DENSE_CHUNK", 1):
        c = run_chain(sc, sc.lu_chain, adjoint_mode=3)
    for other, what in ((b, "second run"), (c, "DC_DENSE_CHUNK=1")):
        assert_bitwise(a, other, slice(None), what)
    m = scene(request, "mid")
    whole = run_chain(m, m.lu_chain, adjoint_mode=3)
    with env_var("DC_DENSE_CHUNK", 2):
        parts = run_chain(m, m.lu_chain, adjoint_mode=3)
    assert_bitwise(whole, parts, slice(None), "DC_DENSE_CHUNK=2, B = 3")
    for slot, gb, _ in parts:
        assert_band_stats(gb)
    assert max(errors(m, m.lu_chain, parts).values()) <= EXACT_TOL


def test_flagged_rollout_takes_the_fp64_fallback(request):
    sc = scene(request, "mid")
    base = run_chain(sc, sc.lu_chain, adjoint_mode=3)
    with env_var("DC_DENSE_FLAG", 1):
        got = run_chain(sc, sc.lu_chain, adjoint_mode=3)
    for slot, gb, _ in got:
        assert gb["converged"][1] == 1 and gb["refine_cycles"][1] == 0 and gb["fp64_iters"][1] > 0 and gb["last_udiff"][1] <= 1e-6
        assert gb["used_direct"][1] == 3 and gb["residual_verified"][1] == 1
        assert_band_stats(gb, [0, 2])
    assert_bitwise(base, got, [0, 2], "DC_DENSE_FLAG=1")
    assert max(errors(sc, sc.lu_chain, got).values()) <= GRAD_TOL


def test_clipping(request):
    sc = scene(request, "mid")
    N, thr = sc.starts[0][0].shape[1] // 3, 0.05
    gx0 = sc.chain[-1]["gx"] * np.array([1.0, 0.01, 1.0])[:, None]
    chain = lu_chain(sc, gx0=gx0, gv0=sc.chain[-1]["gv"], clip_thr=thr)
    assert chain[-1]["clipped"][0] == 1 and chain[-1]["clipped"][1] == 0
    for c in chain:
        assert all(abs(nrm - thr * N) > 1e-3 * thr * N for nrm in c["norms"])
    got = run_chain(sc, chain, adjoint_mode=3, gradient_clipping=1, gradient_clipping_threshold=thr)
    for slot, gb, _ in got:
        assert gb["clipped"].tolist() == chain[slot - 1]["clipped"], (slot, gb["clipped"])
        assert_band_stats(gb)
    w = errors(sc, chain, got)
    print("[clipping] mode 3 vs the LU chain on the pre-scaled gradient: " + " ".join(f"{k} {v:.1e}" for k, v in w.items()))
    assert max(w.values()) <= EXACT_TOL


def test_zero_gradient_rollout(request):
    sc = scene(request, "mid")
    base = run_chain(sc, sc.lu_chain, adjoint_mode=3)
    chain = []
    for c in sc.lu_chain:
        gx, gv = c["gx"].copy(), c["gv"].copy()
        gx[1] = 0.0; gv[1] = 0.0
        chain.append(dict(gx=gx, gv=gv, out=c["out"]))
    got = run_chain(sc, chain, adjoint_mode=3)
    for slot, gb, pg in got:
        for k in ("dL_dx", "dL_dv", "dL_dmu"):
            assert not np.any(gb[k][1]), (slot, k)
        assert np.asarray(pg["dL_ddensity"])[1] == 0.0 and not np.any(np.asarray(pg["dL_dk"])[1])
        assert gb["converged"][1] == 1 and gb["used_direct"][1] == 0 and gb["refine_cycles"][1] == 0 and gb["fp64_iters"][1] == 0
        assert_band_stats(gb, [0, 2])
    assert_bitwise(base, got, [0, 2], "zero gradient in rollout 1")


def test_rollout_backward_matches_step_loop():
    w = workloads.hat_workload()
    B, K = 4, 4
    X0, V0, lead_xf, timed, MU = w["start"](B, np.random.default_rng(1))
    L = len(lead_xf)
    e = capi.Engine(0)
    try:
        e.set_mesh(w["P"], w["F"]); e.set_attachments(w["att"])
        e.set_params(forward_tol=w["fwd_tol"], backward_tol=5e-4, cg_rel_tol=1e-4, cg_max_iter=2000, gradient_clipping=0, adjoint_mode=3, **w["params"])
        e.set_primitives(w["prims"]); e.build()
        e.alloc_batch(B, L + K)
        e.set_mu(MU)
        e.set_state(0, X0, V0)
        e.set_fixed_point_schedule(0, np.concatenate([lead_xf, timed(K)]))
        e.rollout_forward(0, L + K)
        rng = np.random.default_rng(5)
        gx0 = f32(rng.standard_normal((B, 3 * w["P"].shape[0]))); gv0 = f32(0.01 * rng.standard_normal(gx0.shape))
        e.set_gradient(gx0, gv0)
        e.kernel_times(reset=True)
        e.rollout_backward(L + K, K)
        kt = e.kernel_times()
        rx, rv, _ = e.get_gradient()
        st = e.get_stats(L + 1)[1]
        assert (st["used_direct"] == 3).all() and (st["converged"] == 1).all() and (st["fp64_iters"] == 0).all(), st
        assert kt["bwd_launches"] > K and kt["bwd_ms"] > 0
        gx, gv = gx0, gv0
        for s in range(L + K, L, -1):
            gb = e.step_backward(s, gx, gv, is_start=False)
            gx, gv = gb["dL_dx"], gb["dL_dv"]
        assert np.array_equal(rx, gx) and np.array_equal(rv, gv)
    finally:
        e.close()
