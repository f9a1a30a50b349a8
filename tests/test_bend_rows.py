"""Flat-rest bending as per-vertex matrix rows (csrc/dc_windows.h: HostWindows::rows), the host tables, on the CPU
(tests/native/bend_rows_check.cpp): a 12 x 9 flat grid in two windows and the 100 x 100 grid get the rows — no window carries a flap, every
entry position lies in its window's span, window count / size / spans are those of the build without rows, and the decoded fp32 rows
reproduce the per-flap evaluation for a random fp64 vector within the one rounding of each coefficient (2^-24 of the sum of the terms'
magnitudes, + 1e-15 of it for the fp64 summation orders). A grid with one vertex lifted out of plane and the hat of
tests/golden/meshes.npz are refused and get the tables of DC_BEND_ROWS=0 byte for byte. The device side is tests/test_gpu_bend_rows.py."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rows_equal_the_per_flap_sums_and_curved_meshes_keep_their_tables(tmp_path):
    csrc = os.path.join(ROOT, "diffcloth_amd", "csrc")
    exe = str(tmp_path / "bend_rows_check")
    srcs = [os.path.join(ROOT, "tests", "native", "bend_rows_check.cpp")] + [os.path.join(csrc, f) for f in ("dc_system.cpp", "dc_windows.cpp", "dc_packets.cpp", "dc_dense.cpp", "dc_tables.cpp")]
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", csrc, "-o", exe] + srcs)
    m = np.load(os.path.join(ROOT, "tests", "golden", "meshes.npz"))
    V, F = np.ascontiguousarray(m["hat_v"], dtype=np.float64), np.ascontiguousarray(m["hat_f"], dtype=np.int32)
    mesh = tmp_path / "hat.bin"
    mesh.write_bytes(struct.pack("<ii", V.shape[0], F.shape[0]) + V.tobytes() + F.tobytes())
    r = subprocess.run([exe, str(mesh)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ALL OK"), r.stdout + r.stderr
    for line in ("ok grid 12 x 9, windows of 64", "ok grid 12 x 9 jittered in plane, windows of 64", "ok grid 100 x 100", "ok refused grid 12 x 9, one vertex lifted", "ok refused grid 100 x 100, one vertex lifted",
                 "ok refused mesh 1", "ok plan decisions"):
        assert line in r.stdout, line
