"""The fp64 rows of flat-rest bending in the fp64 adjoint operator (csrc/dc_adjoint64.h: apply_K64 with S.win_rows), on the CPU
(tests/native/bend_rows64_check.cpp): for the 12 x 9 grid in two windows and the 100 x 100 grid, the host evaluation of
sum_k brow_val[k] (y_col - y_i) equals the per-flap fp64 pass of element_pass64's formula summed over the corners, for a random fp64 vector,
to 1e-13 of the sum of the terms' magnitudes; with one coefficient dropped the same comparison fails. Built plainly and once more with
-fsanitize=address,undefined (a stand-alone program). The device side is tests/test_gpu_adjoint_own_slot.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_fp64_rows_equal_the_per_flap_fp64_pass(tmp_path, flags):
    csrc = os.path.join(ROOT, "diffcloth_amd", "csrc")
    exe = str(tmp_path / "bend_rows64_check")
    srcs = [os.path.join(ROOT, "tests", "native", "bend_rows64_check.cpp")] + [os.path.join(csrc, f) for f in ("dc_system.cpp", "dc_windows.cpp", "dc_packets.cpp", "dc_dense.cpp", "dc_tables.cpp")]
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-I", csrc, "-o", exe] + srcs)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ALL OK"), r.stdout + r.stderr
    for line in ("ok grid 12 x 9", "ok grid 100 x 100"):
        assert line in r.stdout, line
    assert "one coefficient dropped" in r.stdout
