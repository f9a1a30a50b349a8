"""CPU companion of tests/test_gpu_selfdetect_cases.py and tests/test_gpu_self_layers.py: what those tests take for granted about their
inputs (tests/selfdetect_cases.py) is asserted here, on the fp64 oracle and on the plain numpy / Python model of the same decisions.

  * the model's pair set and layering are the oracle's (two independent statements of the reference's detection and contactSorting);
  * every decision of the detection keeps its margin (check_conditions), so fp32 and fp64 must decide alike;
  * the branch a case was built for is live, counted on the model and on the oracle;
  * each term switched off IN THE MODEL changes the answer on the case built for it — the GPU test's equality with the oracle would
    fail the same way if the kernel lacked that term.
"""
import numpy as np
import pytest

import selfdetect_cases as sc


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(name):
        if name not in cache:
            case = sc.reference(name)[0]
            cache[name] = sc.detect_model(case["X"], case["Vel"], case["V"], case["F"], case["h"])
        return cache[name]
    return get


def prim_set(case, m):
    if case["sphere"] is None:
        return set()
    return sc.sphere_model(case["X"], m["Vg"], case["h"], case["sphere"]["center"], case["sphere"]["radius"])[0]


def only_through_d1(m):
    c = m["cand"]
    return int((c["accepted"] & (c["d0"] >= c["thresh"])).sum())


@pytest.mark.parametrize("name", sc.ALL)
def test_model_is_the_oracle_and_the_conditions_hold(name, models):
    case, o, ref, layered, contacts = sc.reference(name)
    m = models(name)
    N = len(case["X"])
    np.testing.assert_allclose(m["radii"], o.vertex_data()[2], rtol=0, atol=1e-12)
    want = {(a, b) for _, a, b in layered}
    assert len(want) == ref["nself"] == len(layered)
    assert m["pairs"] == want
    fig, bad = sc.check_conditions(case, m)
    g = sc.graph_stats(want, N)
    print(f"\n[{name}] N {N} contacts {ref['nself']} layers {ref['nlayers']} max degree {g['max_degree']} cycles {g['cycles']} "
          f"through d1 only {only_through_d1(m)} axis {m['axis']} cells {m['cellNum']} window {m['window']} prim {ref['nprim']} margins {fig}")
    assert not bad, bad
    assert 1 <= ref["nself"] <= 600                          # the layering walk is one thread
    # primitive contacts and the layering, restated
    prim = prim_set(case, m)
    assert prim == set(o.prim_contacts(ref["id"])["particle"].tolist())
    lay = sc.layering_model(want, prim)
    assert sorted((l, a, b) for (a, b), l in lay.items()) == layered
    assert max(lay.values()) + 1 == ref["nlayers"]
    for l in range(ref["nlayers"]):
        ids = [v for ll, a, b in layered if ll == l for v in (a, b)]
        assert len(ids) == len(set(ids))                     # no vertex twice in a layer


def test_cloud_hubs_branches_are_live(models):
    case, o, ref, layered, _ = sc.reference("cloud_hubs")
    m = models("cloud_hubs")
    pairs = {(a, b) for _, a, b in layered}
    g = sc.graph_stats(pairs, len(case["X"]))
    assert only_through_d1(m) >= 5
    assert g["max_degree"] >= 6 and g["cycles"] >= 1
    # the d1 term: without it the model loses exactly those contacts
    off = sc.detect_model(case["X"], case["Vel"], case["V"], case["F"], case["h"], use_d1=False)
    assert len(pairs - off["pairs"]) == only_through_d1(m) and off["pairs"] < pairs
    # hub ordering: a hub's neighbours walked in the other order give another layering
    walk = {}
    assert sc.layering_model(pairs, neighbours_ascending=False) != sc.layering_model(pairs, stats=walk)
    # both restarts of the walk: from a chain head, and from a loop when no vertex of degree 1 is left
    assert walk["head_picks"] >= 2 and walk["loop_picks"] >= 2


def test_cloud_hubs_velocity_widens_the_neighbourhood(models):
    """The kernel's 2-D grid: cs = max(reach_max, dim / 64) >= reach_max, so K = ceil(reach_max / cs) is 1 for every input — the K > 1
    arm of the neighbourhood loop cannot be reached, and asserting K >= 2 (as first planned) cannot hold. What velocity does widen is
    reach_max and with it the cell size: the statement held here is that the widening is live, i.e. accepted pairs exist that the 3 x 3
    neighbourhood of a grid sized at rest (vmax = 0) would not hold."""
    case = sc.reference("cloud_hubs")[0]
    m = models("cloud_hubs")
    k = sc.kernel_grid_fp64(m, case["h"])
    assert k["K"] == 1
    assert k["reach_max"] >= 2 * k["cs_rest"]
    c = m["cand"]
    acc = c["accepted"]
    dims = np.argsort(-m["dim"])[:2]
    mn = np.minimum(case["X"].min(0), case["X"][0] + m["Vg"][0] * case["h"])
    cells = np.floor((case["X"][:, dims] - mn[dims]) / k["cs_rest"]).astype(int)
    apart = np.abs(cells[c["i"][acc]] - cells[c["j"][acc]]).max(axis=1)
    print(f"\n[cloud_hubs] reach_max {k['reach_max']:.3f} cs {k['cs']:.3f} cs at rest {k['cs_rest']:.3f} K {k['K']}: "
          f"{int((apart >= 2).sum())} accepted pairs lie outside the 3 x 3 cells of the grid at rest")
    assert (apart >= 2).sum() >= 2


def test_planted_window_branches_are_live(models):
    case, o, ref, layered, _ = sc.reference("planted_window")
    m = models("planted_window")
    c = m["cand"]
    pairs = {(a, b) for _, a, b in layered}
    only_window = c["near"] & ~c["inwin"]
    only_unit = ~c["near"] & c["inwin"]
    assert only_window.sum() >= 2 and only_unit.sum() >= 2 and only_through_d1(m) >= 2
    cand = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(c["i"], c["j"]))}
    for p in case["planted"]["window"]:
        assert only_window[cand[p]] and p not in pairs       # the reference never tests them
    for p in case["planted"]["unit"]:
        assert only_unit[cand[p]] and p not in pairs
    for p in case["planted"]["d1"]:
        k = cand[p]
        assert p in pairs and c["d0"][k] >= c["thresh"][k] > c["d1"][k]
    # each term switched off in the model reports exactly the pairs that term leaves out
    args = (case["X"], case["Vel"], case["V"], case["F"], case["h"])
    no_window = sc.detect_model(*args, window_reject=False)["pairs"]
    no_unit = sc.detect_model(*args, unit_cut=False)["pairs"]
    assert no_window - pairs >= set(case["planted"]["window"]) and len(no_window - pairs) == only_window.sum()
    assert no_unit - pairs >= set(case["planted"]["unit"]) and len(no_unit - pairs) == only_unit.sum()
    assert m["maxR"] < 0.125                                 # from there on the window is wider than 1.0 and cannot reject


def test_axis_and_cell_cap_are_live(models):
    assert models("cloud_axis_y")["axis"] == 1
    m = models("cloud_512_cells")
    assert m["cellNum"] == 512 and m["cells_f"] > 513
    assert models("cloud_hubs")["axis"] == 0 and models("stack4")["axis"] == 2


def test_kernel_instances_are_reached(models):
    """the detection kernel's instances switch at N = 1536 and N = 6144 (256 / 512 / 1024 threads)"""
    assert len(sc.reference("cloud_hubs")[0]["X"]) < 1536 <= len(sc.reference("cloud_512_threads")[0]["X"]) < 6144
    assert len(sc.reference("cloud_1024_threads")[0]["X"]) >= 6144
    for name in ("cloud_512_threads", "cloud_1024_threads"):
        assert 200 <= sc.reference(name)[2]["nself"] <= 600


def test_batched_clouds_have_different_contact_counts():
    counts = [sc.reference(n)[2]["nself"] for n in ("cloud_hubs", "cloud_hubs_b", "cloud_hubs_c")]
    assert len(set(counts)) == 3
    counts = [sc.reference(n)[2]["nself"] for n in ("planted_window", "cloud_window_b", "cloud_window_c")]
    assert len(set(counts)) == 3
    assert len({sc.reference(n)[0]["h"] for n in ("planted_window", "cloud_window_b", "cloud_window_c")}) == 1     # one engine, one h


def test_with_sphere_seeds_the_frontier(models):
    case, o, ref, layered, _ = sc.reference("with_sphere")
    plain = sc.reference("cloud_hubs")[3]
    pairs = {(a, b) for _, a, b in layered}
    assert pairs == {(a, b) for _, a, b in plain}            # the sphere changes no self contact ...
    deg = sc.graph_stats(pairs, len(case["X"]))["deg"]
    prim = prim_set(case, models("with_sphere"))
    seeds = [p for p in prim if deg[p] > 0]
    print(f"\n[with_sphere] {len(prim)} primitive contacts, {len(seeds)} of them frontier seeds; layers {ref['nlayers']} against "
          f"{sc.reference('cloud_hubs')[2]['nlayers']} without the sphere")
    assert len(seeds) >= 10
    assert layered != plain                                  # ... but their layers
    assert sc.layering_model(pairs, prim, seed_frontier=False) != sc.layering_model(pairs, prim)


@pytest.mark.parametrize("name", ["stack3", "stack4", "stack4_29"])
def test_stacks_are_deep_and_the_sphere_changes_their_layers(name):
    _, _, ref, layered, _ = sc.reference(name)
    _, _, ref_s, layered_s, _ = sc.reference(name + "_sphere")
    print(f"\n[{name}] contacts {ref['nself']} layers {ref['nlayers']} PD iterations {ref['iters']}; with the sphere: contacts {ref_s['nself']} "
          f"layers {ref_s['nlayers']} primitive contacts {ref_s['nprim']} PD iterations {ref_s['iters']}")
    assert ref["converged"] and ref_s["converged"]
    assert ref["nlayers"] >= 150 and ref_s["nlayers"] >= 150
    assert ref_s["nprim"] > 0
    assert [(a, b) for _, a, b in sorted(layered, key=lambda t: t[1:])] == [(a, b) for _, a, b in sorted(layered_s, key=lambda t: t[1:])]
    assert layered != layered_s


def test_which_deep_cases_fit_the_lds_of_the_one_workgroup_forward_kernel():
    """7 M + 8 C + layers + 2 floats against the 3 NP the packet forward kernel offers: only zigzag40 fits (its layered passes run in LDS,
    241 layers on a single wave); the stacks on 256 and 841 vertices run the global-memory passes on one workgroup whatever DC_SELF_LDS says"""
    fits = {}
    for name in ("stack3", "stack4_sphere", "stack4_29", "zigzag40"):
        case, _, ref, layered, _ = sc.reference(name)
        M = len({v for _, a, b in layered for v in (a, b)})
        need, offered = sc.self_lds_need(M, ref["nself"], ref["nlayers"]), sc.forward_lds_floats(len(case["X"]))
        print(f"\n[{name}] N {len(case['X'])} M {M} contacts {ref['nself']} layers {ref['nlayers']}: needs {need} floats, offered {offered}")
        fits[name] = need <= offered
    assert fits == dict(stack3=False, stack4_sphere=False, stack4_29=False, zigzag40=True)
    assert sc.reference("zigzag40")[2]["nlayers"] >= 150 and sc.reference("zigzag40")[2]["converged"]
    assert [sc.forward_lds_floats(n) for n in (256, 841, 1600, 6241)] == [1536, 3072, 6144, 24576]
