"""The arithmetic the adjoint's step-resident contact tables share between kernel and host (csrc/dc_launchplan.h: adj_mask_words, adj_rank,
adj_tables_floats, adj_tables_fit), checked on the CPU by tests/native/resident_rank_check.cpp: a contact vertex's slot — per-word count plus
popcount below its bit — against a brute-force count on empty, full, single-bit and random masks (set bits at 0, 31, 32 and N - 1, N not a
multiple of 64), and the "fits / does not fit" rule against the layout the kernel derives from it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rank_of_a_contact_vertex_and_the_fit_rule_of_the_tables(tmp_path):
    csrc = os.path.join(ROOT, "diffcloth_amd", "csrc")
    exe = str(tmp_path / "resident_rank_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "native", "resident_rank_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ALL OK"), r.stdout + r.stderr
