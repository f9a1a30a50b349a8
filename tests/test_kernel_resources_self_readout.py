"""Register / scratch budget of the self-contact read-out's kernel (csrc/dc_self_readout.hip: k_self_readout, ONE instance for fp32 and fp64
outputs), read from the cross-compiled gfx950 code object. The figures were measured when the kernel was written —
77 VGPRs, no scratch, no spilled VGPR, 256 threads, 160 B of static LDS — and the budget is those figures with the margin of
tests/test_kernel_resources_readout.py: the same scratch, the VGPR allocation (80: what 77 registers occupy at the next granule of eight),
no spilled VGPR. No GPU needed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# instance -> (max scratch bytes per lane, max spilled VGPRs, VGPR allocation, threads)
BUDGET = {
    "dc::k_self_readout": (0, 0, 80, 256),
}


@pytest.fixture(scope="module")
def resources():
    import kernel_resources as kr
    if not os.path.isdir(kr.OBJDIR) or not any(f.endswith(".o") for f in os.listdir(kr.OBJDIR)):
        pytest.skip("engine objects not built (python -c 'import __graft_entry__ as g; g.build()')")
    return kr, kr.collect()


def test_self_readout_kernels_stay_inside_their_budget(resources):
    kr, res = resources
    lines = []
    for prefix, (scratch, spills, vgprs, threads) in BUDGET.items():
        f, k = kr.find(res, prefix)
        assert k is not None, f"kernel instance not found in the code objects: {prefix}"
        assert f == "dc_self_readout.hip.o", f
        lines.append(f"{prefix}: {k['private_segment_fixed_size']} B/lane scratch (budget {scratch}), {k['vgpr_spill_count']} spilled VGPRs "
                     f"(budget {spills}), {k['vgpr_count']} VGPRs (allocation {vgprs}), {k['sgpr_spill_count']} spilled SGPRs, "
                     f"{k['group_segment_fixed_size']} B static LDS [{f}]")
        assert k["private_segment_fixed_size"] <= scratch, lines[-1]
        assert k["vgpr_spill_count"] <= spills, lines[-1]
        assert k["vgpr_count"] <= vgprs and k["agpr_count"] == 0, lines[-1]
        assert k["max_flat_workgroup_size"] == threads, lines[-1]
        assert k["group_segment_fixed_size"] <= 256, lines[-1]          # kLdsReserveBytes: what the dynamic LDS plan leaves for it
    print("\n" + "\n".join(lines))
