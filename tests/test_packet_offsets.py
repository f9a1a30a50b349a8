"""The byte-offset layout of the packet matrix (csrc/dc_packets.h: HostPackets::to_offsets), which the forward kernel instances that hold
the search direction as halves read: decoded on the CPU (tests/native/packet_offsets_check.cpp) for the 100 x 100 grid and for the
irregular 7 742-vertex dress of tests/golden/meshes.npz (rows of more than 12 off-diagonals, i.e. more than one batch). Every decoded
(row, column, value) triple equals the CSR's and the first layout's, in the same per-row order; padding entries are zero on the row itself;
every offset stays inside the direction array; the table plan chooses the layout exactly for the instances that read it."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_byte_offset_stream_decodes_to_the_csr_in_row_order(tmp_path):
    csrc = os.path.join(ROOT, "diffcloth_amd", "csrc")
    exe = str(tmp_path / "packet_offsets_check")
    srcs = [os.path.join(ROOT, "tests", "native", "packet_offsets_check.cpp")] + [os.path.join(csrc, f) for f in ("dc_system.cpp", "dc_windows.cpp", "dc_packets.cpp", "dc_dense.cpp", "dc_tables.cpp")]
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", csrc, "-o", exe] + srcs)
    m = np.load(os.path.join(ROOT, "tests", "golden", "meshes.npz"))
    V, F = np.ascontiguousarray(m["dress7k_v"], dtype=np.float64), np.ascontiguousarray(m["dress7k_f"], dtype=np.int32)
    mesh = tmp_path / "dress7k.bin"
    mesh.write_bytes(struct.pack("<ii", V.shape[0], F.shape[0]) + V.tobytes() + F.tobytes())
    r = subprocess.run([exe, str(mesh)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ALL OK"), r.stdout + r.stderr
    assert "ok grid 100 x 100" in r.stdout and "ok mesh 1" in r.stdout and "ok plan decisions" in r.stdout
