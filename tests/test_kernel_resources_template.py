"""Register / scratch budget of the forward kernel the headline launches since the packet matrix has its template layout
(k_pd_step_pk_tpl, csrc/dc_forward_pk_tpl.hip), read from the gfx950 code objects as tests/test_kernel_resources.py reads the others'.
The budget is the one that file gives the byte-offset instance this kernel replaces on the headline's mesh — 448 B of scratch per lane,
128 spilled VGPRs, 256 VGPRs (two waves per SIMD) — not a value taken from this kernel's own code object (416 B / 109 when it was written)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNEL = "dc::k_pd_step_pk_tpl<512, 20, 12, true>"
SCRATCH, SPILLS, VGPRS, THREADS = 448, 128, 256, 512


def test_template_forward_kernel_stays_inside_the_headline_budget():
    import kernel_resources as kr
    if not os.path.isdir(kr.OBJDIR) or not any(f.endswith(".o") for f in os.listdir(kr.OBJDIR)):
        pytest.skip("engine objects not built (python -c 'import __graft_entry__ as g; g.build()')")
    res = kr.collect()
    f, k = kr.find(res, KERNEL)
    assert k is not None, f"kernel instance not found in the code objects: {KERNEL}"
    line = (f"{KERNEL}: {k['private_segment_fixed_size']} B/lane scratch (budget {SCRATCH}), {k['vgpr_spill_count']} spilled VGPRs (budget {SPILLS}), "
            f"{k['vgpr_count']} VGPRs, {k['sgpr_spill_count']} spilled SGPRs [{f}]")
    print("\n" + line)
    assert f == "dc_forward_pk_tpl.hip.o", line
    assert k["private_segment_fixed_size"] <= SCRATCH, line
    assert k["vgpr_spill_count"] <= SPILLS, line
    assert k["vgpr_count"] <= VGPRS and k["agpr_count"] == 0, line      # occupancy: 2 waves per SIMD
    assert k["max_flat_workgroup_size"] == THREADS, line
    assert kr.HOT["bench forward 256x1"] == KERNEL, "tools/kernel_resources.py must name the instance the headline launches"
