"""Register / scratch budget of the contact read-out's adjoint kernels (csrc/dc_readout_adjoint.hip: k_readout_adjoint<0>, the seed pass, and
k_readout_adjoint<1>, the parameter pass), read from the cross-compiled gfx950 code object. The figures were measured
when the kernels were written — 79 and 110 VGPRs, no scratch, no spilled VGPR, 512 threads (at 1024 the parameter pass spills) — and the budget is those figures with the margin of
tests/test_kernel_resources_moving.py: the same scratch, the same VGPR allocation (128: what 110 registers occupy at the next granule of
occupancy), a tenth more spilled VGPRs (of none: none). The kernels inline the fp64 element operator of dc_adjoint64.h, so a change there
that pushes them into scratch shows here. No GPU needed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# instance -> (max scratch bytes per lane, max spilled VGPRs, VGPR allocation, threads)
BUDGET = {
    "dc::k_readout_adjoint<0>": (0, 0, 128, 512),
    "dc::k_readout_adjoint<1>": (0, 0, 128, 512),
}


@pytest.fixture(scope="module")
def resources():
    import kernel_resources as kr
    if not os.path.isdir(kr.OBJDIR) or not any(f.endswith(".o") for f in os.listdir(kr.OBJDIR)):
        pytest.skip("engine objects not built (python -c 'import __graft_entry__ as g; g.build()')")
    return kr, kr.collect()


def test_readout_adjoint_kernels_stay_inside_their_budget(resources):
    kr, res = resources
    lines = []
    for prefix, (scratch, spills, vgprs, threads) in BUDGET.items():
        f, k = kr.find(res, prefix)
        assert k is not None, f"kernel instance not found in the code objects: {prefix}"
        assert f == "dc_readout_adjoint.hip.o", f
        lines.append(f"{prefix}: {k['private_segment_fixed_size']} B/lane scratch (budget {scratch}), {k['vgpr_spill_count']} spilled VGPRs "
                     f"(budget {spills}), {k['vgpr_count']} VGPRs, {k['sgpr_spill_count']} spilled SGPRs [{f}]")
        assert k["private_segment_fixed_size"] <= scratch, lines[-1]
        assert k["vgpr_spill_count"] <= spills, lines[-1]
        assert k["vgpr_count"] <= vgprs and k["agpr_count"] == 0, lines[-1]
        assert k["max_flat_workgroup_size"] == threads, lines[-1]
    print("\n" + "\n".join(lines))
