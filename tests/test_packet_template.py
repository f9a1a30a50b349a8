"""The template layout of the packet matrix (csrc/dc_packets.h: HostPackets::to_template), which the forward kernel k_pd_step_pk_tpl reads
on regularly numbered meshes: values only, one set of at most twelve column offsets for the whole matrix. Decoded on the CPU
(tests/native/packet_template_check.cpp): on the headline's 100 x 100 grid the template is the twelve offsets of its triangulation, every
row decodes to the CSR's (row, column, value) triples in row order with zeros only where the row lacks the neighbour, it agrees with the
byte-offset decode entry by entry, and the guard rows fit the LDS; the plan falls back to the byte-offset layout, byte for byte, under
DC_PK_TPL=0, for a deflated solve, for the renumbered grid and for the 7 742-vertex dress (rows of more than one batch); on the 96 x 96 slope
fabric it decides what the rule, computed from the CSR alone, says. The same program is built once more with the address and
undefined-behaviour sanitizers (host code, stand-alone)."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "diffcloth_amd", "csrc")
SRCS = [os.path.join(ROOT, "tests", "native", "packet_template_check.cpp")] + [os.path.join(CSRC, f) for f in ("dc_system.cpp", "dc_windows.cpp", "dc_packets.cpp", "dc_dense.cpp", "dc_tables.cpp")]


@pytest.fixture(scope="module")
def mesh_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("packet_template")
    m = np.load(os.path.join(ROOT, "tests", "golden", "meshes.npz"))
    out = []
    for name in ("perf96", "dress7k"):
        V, F = np.ascontiguousarray(m[name + "_v"], dtype=np.float64), np.ascontiguousarray(m[name + "_f"], dtype=np.int32)
        p = d / (name + ".bin")
        p.write_bytes(struct.pack("<ii", V.shape[0], F.shape[0]) + V.tobytes() + F.tobytes())
        out.append(str(p))
    return d, out


def run(exe, meshes):
    r = subprocess.run([exe] + meshes, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ALL OK"), r.stdout + r.stderr
    assert "ok grid 100 x 100" in r.stdout and "ok plan: template, guards 1600 bytes" in r.stdout and "ok plan: fall-backs by switch and deflation" in r.stdout
    assert "ok plan: renumbered grid falls back" in r.stdout and "ok mesh 1 N=9216" in r.stdout
    assert "ok mesh 2 N=7742" in r.stdout and r.stdout.count("plan=fall-back") >= 1
    return r.stdout


def test_template_stream_decodes_to_the_csr_and_the_plan_follows_the_rule(mesh_files):
    d, meshes = mesh_files
    exe = str(d / "packet_template_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", CSRC, "-o", exe] + SRCS)
    run(exe, meshes)


def test_template_check_is_clean_under_the_host_sanitizers(mesh_files):
    d, meshes = mesh_files
    exe = str(d / "packet_template_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, "-o", exe] + SRCS)
    run(exe, meshes)
