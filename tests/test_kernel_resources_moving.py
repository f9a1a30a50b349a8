"""Register / scratch budget of the adjoint step kernels that run once a context holds an obstacle-velocity table (dc_set_primitive_velocities):
k_adjoint_step_moving / k_adjoint_step_cl_moving, the sources of dc_adjoint.hip / dc_adjoint_cl.hip compiled with the velocity rows and the
dL/dw block. tests/test_kernel_resources.py pins the instances without the table under their own names; these match none
of its prefixes, so their allocation would drift unnoticed.

The budgets are those of the same shapes in tests/test_kernel_resources.py — the same scratch per lane, the same VGPR allocation (occupancy) and
thread count — with a tenth more spilled VGPRs: the moving kernels carry the velocity row, the gradient row and their stride through the
whole solve (five more uniform registers live; spilled SGPRs take VGPR lanes), and a kernel at the 256-register cap answers any further live
value with spills. No GPU needed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# moving instance -> (max scratch bytes per lane, max spilled VGPRs = 1.1 x the static shape's budget, VGPR allocation, threads)
BUDGET = {
    "dc::k_adjoint_step_moving<1024, true, false, false, false>": (512, 176, 128, 1024),
    "dc::k_adjoint_step_moving<1024, true, false, true, false>": (384, 143, 128, 1024),
    "dc::k_adjoint_step_cl_moving<512, false, false>": (608, 286, 256, 512),
    "dc::k_adjoint_step_cl_moving<512, true, false>": (560, 236, 256, 512),
}


@pytest.fixture(scope="module")
def resources():
    import kernel_resources as kr
    if not os.path.isdir(kr.OBJDIR) or not any(f.endswith(".o") for f in os.listdir(kr.OBJDIR)):
        pytest.skip("engine objects not built (python -c 'import __graft_entry__ as g; g.build()')")
    return kr, kr.collect()


def test_moving_adjoint_kernels_stay_inside_their_budget(resources):
    kr, res = resources
    lines = []
    for prefix, (scratch, spills, vgprs, threads) in BUDGET.items():
        f, k = kr.find(res, prefix)
        assert k is not None, f"kernel instance not found in the code objects: {prefix}"
        lines.append(f"{prefix}: {k['private_segment_fixed_size']} B/lane scratch (budget {scratch}), {k['vgpr_spill_count']} spilled VGPRs "
                     f"(budget {spills}), {k['vgpr_count']} VGPRs, {k['sgpr_spill_count']} spilled SGPRs [{f}]")
        assert k["private_segment_fixed_size"] <= scratch, lines[-1]
        assert k["vgpr_spill_count"] <= spills, lines[-1]
        assert k["vgpr_count"] <= vgprs and k["agpr_count"] == 0, lines[-1]
        assert k["max_flat_workgroup_size"] == threads, lines[-1]
    print("\n" + "\n".join(lines))


def test_every_static_adjoint_instance_has_its_moving_twin(resources):
    """the launchers hand a launch with a velocity table to the instance of the same template arguments"""
    kr, res = resources
    names = {k["demangled"] for ks in res.values() for k in ks}
    for base in ("dc::k_adjoint_step<", "dc::k_adjoint_step_cl<"):
        static = sorted(n for n in names if n.startswith(base))
        assert static, base
        for n in static:
            twin = n.replace(base, base[:-1] + "_moving<", 1)
            assert any(m.startswith(twin.split("(")[0]) for m in names), twin
