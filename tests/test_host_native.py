"""Host-side table builders of the HIP kernels (packet-ELL matrix, element windows, RCM renumbering, explicit inverse of small systems, the table plan
of dc_build: wave-sliced ELL matrix, planar and high / low rest-shape tables, diagonal scalings), checked on the
CPU by a small C++ harness (tests/native/host_tables_check.cpp) against the plain constraint system."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_packet_window_and_rcm_tables(tmp_path):
    csrc = os.path.join(ROOT, "diffcloth_amd", "csrc")
    exe = str(tmp_path / "host_tables_check")
    srcs = [os.path.join(ROOT, "tests", "native", "host_tables_check.cpp")] + [os.path.join(csrc, f) for f in ("dc_system.cpp", "dc_windows.cpp", "dc_packets.cpp", "dc_dense.cpp", "dc_tables.cpp")]
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", csrc, "-o", exe] + srcs)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ALL OK"), r.stdout + r.stderr


def test_record_import_lays_out_the_callers_self_contacts(tmp_path):
    """csrc/dc_record.cpp, the host part of dc_set_record, on 8 vertices, max_self_contacts = 4 and two rollouts against answers written out by
    hand (tests/native/record_import_check.cpp): layer offsets and tail of the meta block, working-set ranks bit-for-bit in nrm.w, pairs, verts
    and primitive indices in device numbering under a renumbering, the running offset into the concatenated lists, every rejection."""
    csrc = os.path.join(ROOT, "diffcloth_amd", "csrc")
    exe = str(tmp_path / "record_import_check")
    srcs = [os.path.join(ROOT, "tests", "native", "record_import_check.cpp"), os.path.join(csrc, "dc_record.cpp")]
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", csrc, "-o", exe] + srcs)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ALL OK"), r.stdout + r.stderr


def test_cluster_plan_keeps_every_workgroup_resident_and_refuses_what_does_not_fit(tmp_path):
    """csrc/dc_clusterplan.cpp, the host-side plan of the split execution (tests/native/cluster_plan_check.cpp): for every batch size 1 ... 300 on
    256, 304 and 64 CUs the workgroups of a launch fit one XCD's CUs and the launches cover the batch; every rejection of the per-K search on the
    smallest grid that triggers it; the shape of an accepted plan; the K walk, the early returns and the switches — against answers worked out by
    hand or written down from the engine before the plan was moved out of it."""
    csrc = os.path.join(ROOT, "diffcloth_amd", "csrc")
    exe = str(tmp_path / "cluster_plan_check")
    srcs = [os.path.join(ROOT, "tests", "native", "cluster_plan_check.cpp")] + [os.path.join(csrc, f) for f in ("dc_clusterplan.cpp", "dc_system.cpp", "dc_windows.cpp", "dc_packets.cpp")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-Wall", "-I", csrc, "-o", exe] + srcs)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ALL OK"), r.stdout + r.stderr


def test_launch_plan_sizes_offsets_and_limits_of_the_dynamic_lds(tmp_path):
    """csrc/dc_launchplan.h, the host-side plan of every step kernel's dynamic LDS (tests/native/launch_plan_check.cpp): byte counts, offsets, the
    y list's room and the refusals at the workgroup's limit against figures written out by hand; the split plan's bounds cover every instance
    the launchers choose, on a sweep of part shapes and for every plan ClusterPlan::fit accepts with K = 2 ... 8 on three grids."""
    csrc = os.path.join(ROOT, "diffcloth_amd", "csrc")
    exe = str(tmp_path / "launch_plan_check")
    srcs = [os.path.join(ROOT, "tests", "native", "launch_plan_check.cpp")] + [os.path.join(csrc, f) for f in ("dc_clusterplan.cpp", "dc_system.cpp", "dc_windows.cpp", "dc_packets.cpp")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", csrc, "-o", exe] + srcs)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ALL OK"), r.stdout + r.stderr


def test_kernel_plan_names_a_compiled_instance_for_every_mesh_size_and_switch(tmp_path):
    """csrc/dc_kernelplan.h, the host-side plan of which kernel instance runs a step (tests/native/kernel_plan_check.cpp): the forward choice
    (family, threads, rows, XL, halves, offsets, inverse, deflated, fusable) against answers written out by hand at every mesh size where it
    changes, on the decisions HostTables::build takes on generated meshes, under the switches that move it; the adjoint's five conditions in
    every combination; for every N up to 13 000 and every switch combination the choice names an entry of the instance tables, fusable <=> a
    packet family, pk_ofs <=> the instance reads byte offsets, fwd_defl => a deflated instance; every accepted split plan has its instances."""
    csrc = os.path.join(ROOT, "diffcloth_amd", "csrc")
    exe = str(tmp_path / "kernel_plan_check")
    srcs = [os.path.join(ROOT, "tests", "native", "kernel_plan_check.cpp")] + [os.path.join(csrc, f) for f in ("dc_tables.cpp", "dc_clusterplan.cpp", "dc_system.cpp", "dc_windows.cpp", "dc_packets.cpp", "dc_dense.cpp")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", csrc, "-o", exe] + srcs)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ALL OK"), r.stdout + r.stderr


def test_deflation_builder_finds_the_lowest_eigenvectors(tmp_path):
    """csrc/dc_deflate.cpp on a synthetic badly graded strip (cells shrinking 100 x across the sheet): the Chebyshev-filtered subspace
    iteration returns orthonormal vectors whose eigen-residuals |A u - theta u| are small, (U^T A U)^-1 is consistent, in well under a
    second (tests/native/deflation_check.cpp)."""
    csrc = os.path.join(ROOT, "diffcloth_amd", "csrc")
    exe = str(tmp_path / "deflation_check")
    srcs = [os.path.join(ROOT, "tests", "native", "deflation_check.cpp")] + [os.path.join(csrc, f) for f in ("dc_system.cpp", "dc_deflate.cpp")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", csrc, "-o", exe] + srcs)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr


def test_discretised_sphere_face_table_is_the_reference_mesh(tmp_path):
    """DC_PRIM_SPHERE_DISCRETIZED: the engine's face table (csrc/dc_spheremesh.cpp, written from the structure of the mesh) against the oracle's
    loop-by-loop restatement of Sphere::Sphere (Primitive.cpp:133-216): same faces, same ORDER (the contact code keeps the last face that
    qualifies), same corner order (it fixes the sign of the normal), bit-equal coordinates. A closed surface with outward normals."""
    import ctypes as C
    import numpy as np
    import orc
    csrc = os.path.join(ROOT, "diffcloth_amd", "csrc")
    exe = str(tmp_path / "spheremesh_dump")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "native", "spheremesh_dump.cpp"), os.path.join(csrc, "dc_spheremesh.cpp")])
    L = orc.lib()
    L.orc_sphere_mesh.restype = C.c_int
    for radius, res in ((15.0, 40), (2.5, 7)):
        got = np.frombuffer(subprocess.run([exe, repr(radius), str(res)], capture_output=True, timeout=60, check=True).stdout, dtype=np.float64).reshape(-1, 12)
        want = np.zeros(12 * (2 * res * res + 16))
        n = L.orc_sphere_mesh(C.c_double(radius), C.c_int(res), want.ctypes.data_as(C.POINTER(C.c_double)), C.c_int(want.size // 12))
        want = want[:12 * n].reshape(n, 12)
        assert got.shape == want.shape and n == 2 * res * (res - 1)
        np.testing.assert_array_equal(got[:, :9], want[:, :9])
        np.testing.assert_allclose(got[:, 9:], want[:, 9:], rtol=0, atol=1e-15)
        cen = got[:, :9].reshape(n, 3, 3).mean(axis=1)
        assert ((got[:, 9:] * cen).sum(axis=1) > 0.9 * np.linalg.norm(cen, axis=1)).all()
