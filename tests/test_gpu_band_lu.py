"""The band adjoint solve's LU and substitution kernels (csrc/dc_adjoint_band.hip: k_band_panel, k_band_trsm, k_band_update through
launch_band_factor, and band_substitute<1024>) on band matrices a scene cannot produce, against scipy.linalg.lu_factor / lu_solve on the
dense embedding in fp64, with residuals accumulated in numpy.longdouble.

The kernels run through the check library tests/native/band_lu_check.hip, which includes the product's translation unit as text (no copy)
and is cross-compiled by diffcloth_amd/build.py (build_kernel_checks); this module loads it and does not compile. Inputs and layouts:
tests/band_lu_cases.py; the checkers are those of tests/dense_lu_cases.py, fed the device's band factors expanded to the dense device layout;
tests/test_band_lu_companion.py runs the same on scipy's factors on the CPU and checks the conditions on the inputs.

Every call: 3 different matrices, (n, kl) in band_lu_cases.SIZES with ku = kl (and (700, 650) for the far-edge, control and exact classes:
the panel kernel's global-memory variant), ldab = 3 kl + 1 rounded up to 16; every entry of the buffer
that belongs to no matrix element (the band's corners, the padding rows) is NaN on entry and asserted bitwise unchanged, piv's tail a sentinel.
Classes: Gaussian inside the band, far-edge (pivot = the band's last row in every column), diagonally dominant control (no swap), exact dyadic
P L U with ties. Gates: |L| <= 1 exactly; |P A - L U|_F / |A|_F and |b - A x| / (|A|_F |x| + |b|) at most 8 x scipy's own figure on the
same matrix, or n 2^-53 where that is larger; the exact class bit for bit (piv, L, U, x). Flag cases (n = 97, kl = 32: zero column at 0, 31,
32, n - 1; one NaN, one Inf entry): flag == 1 for that matrix alone, the two other matrices of the call bitwise as without it; a matrix
flagged on entry comes back untouched.

Measured on an MI355X, worst over the sizes and the 3 matrices (62 tests, 18 s; (700, 650) included, which changes no worst figure):
  class      swapped columns    factor error / scipy's   factor error / gate   solve error / gate
  gaussian   75.0 ... 98.5 %    1.13                     0.052                 0.018
  far_edge   85.0 ... 99.7 %    2.07                     0.001                 0.014
  control    0                  3.35                     0.048                 0.020
  exact      every error exactly 0; piv, L, U, x bit for bit, ties in every case
"""
import ctypes
import os

import numpy as np
import pytest

import band_lu_cases as B
import dense_lu_cases as C
from diffcloth_amd import build as dcbuild

pytestmark = pytest.mark.gpu
_lib = None

def check_library():
    global _lib
    if _lib is None:
        path = dcbuild.kernel_check_path("libdc_band_lu_check.so")
        if not os.path.exists(path):
            pytest.fail(f"{path} is missing: build it with `python -m diffcloth_amd.build` (or __graft_entry__.build()); this test does not compile")
        _lib = ctypes.CDLL(path)
        _lib.dc_check_band_lu.restype = ctypes.c_int
        _lib.dc_check_band_lu.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_char_p, ctypes.c_int]
    return _lib


def device_lu(mats, kl, rhs, flags_in=None):
    """One call of the check library on the band matrices `mats` [nb] (n x n, zero outside the band) with right-hand sides rhs [nb][3][n].
    Returns the factors expanded to the dense device layout [nb], piv [nb][n], flag [nb], x [nb][3][n] (NaN where the kernel wrote
    nothing) and the raw band buffers (after, before). Asserts that no entry outside the band's elements and piv[:n] was written."""
    lib = check_library()
    nb, n = len(mats), mats[0].shape[0]
    ldab, npiv = B.ldab_of(kl), B.npiv_of(n)
    AB = np.stack([B.to_band(A, kl) for A in mats])
    AB0 = AB.copy()
    piv = np.full((nb, npiv), B.PIV_SENTINEL, dtype=np.int32)
    flag = np.zeros(nb, dtype=np.int32) if flags_in is None else np.array(flags_in, dtype=np.int32)
    rhs = np.ascontiguousarray(rhs, dtype=np.float64)
    x = np.full_like(rhs, np.nan)
    err = ctypes.create_string_buffer(512)
    rc = lib.dc_check_band_lu(nb, n, kl, ldab, npiv, AB.ctypes.data, piv.ctypes.data, flag.ctypes.data, rhs.shape[1], rhs.ctypes.data, x.ctypes.data, err, 512)
    assert rc == 0, err.value.decode()
    pad = ~B.band_valid(n, kl)
    assert np.array_equal(AB.view(np.uint64)[:, pad], AB0.view(np.uint64)[:, pad]), "an entry outside the band's elements was written"
    assert (piv[:, n:] == B.PIV_SENTINEL).all(), "piv was written beyond n"
    F = [B.expand(AB[m], piv[m, :n], n, kl) if flag[m] == 0 else None for m in range(nb)]
    return F, piv[:, :n].copy(), flag, x, (AB, AB0)


@pytest.mark.parametrize("cls,n,kl", B.CASES)
def test_factor_and_solve_against_scipy(cls, n, kl):
    mats = B.matrices(cls, n, kl)
    rhs = np.stack([B.rhs_for(n, m) for m in range(B.NB)])
    F, piv, flag, X, _ = device_lu(mats, kl, rhs)
    assert (flag == 0).all()
    worst_f = worst_s = 0.0
    fails = []
    for m, A in enumerate(mats):
        label = f"{cls} n={n} kl={kl} m={m}"
        err, ref, swaps = C.check_factors(A, F[m], piv[m], label)
        solves = C.check_solves(A, X[m], rhs[m], label)
        print(f"[{label}] swaps {swaps}/{n} factor {err:.3e} (scipy {ref:.3e}, gate {C.gate(ref, n):.3e}) solves " +
              " ".join(f"{e:.2e}/{r:.2e}" for e, r in solves))
        worst_f = max(worst_f, err / C.gate(ref, n))
        if not err <= C.gate(ref, n):
            fails.append((label, "factor", err, ref))
        for k, (e, r) in enumerate(solves):
            worst_s = max(worst_s, e / C.gate(r, n))
            if not e <= C.gate(r, n):
                fails.append((label, f"solve {k}", e, r))
    print(f"[{cls} n={n} kl={kl}] worst ratio to the gate: factor {worst_f:.3f} solve {worst_s:.3f}")
    assert not fails, fails


@pytest.mark.parametrize("n,kl", B.SIZES + B.WIDE_SIZES)
def test_exact_class_bit_for_bit(n, kl):
    cases = [B.exact_case(n, kl, np.random.default_rng([B.seed_of("exact", n, kl), m])) for m in range(B.NB)]
    F, piv, flag, X, _ = device_lu([c[0] for c in cases], kl, np.stack([c[5] for c in cases]))
    assert (flag == 0).all()
    for m, (A, Fx, px, tie, Xx, Bv) in enumerate(cases):
        label = f"exact n={n} kl={kl} m={m}"
        C.check_exact(A, C.to_lapack(B.pure_to_device(Fx, px), px), px, Xx, F[m], piv[m], X[m], label)
        err, ref, swaps = C.check_factors(A, F[m], piv[m], label)
        print(f"[{label}] swaps {swaps}/{n} tie columns {int(tie.sum())} factor error {err}")
        assert err == 0.0


@pytest.mark.parametrize("name", sorted(B.FLAG_CASES))
@pytest.mark.parametrize("where", [0, 1, 2])
def test_flag_cases(name, where):
    bad = B.flag_case(name)
    n, kl = B.FLAG_N, B.FLAG_KL
    good = B.matrices("gaussian", n, kl, seed=991)
    rhs = np.stack([B.rhs_for(n, m) for m in range(B.NB)])
    Fg, pg, flg, Xg, _ = device_lu(good, kl, rhs)
    assert (flg == 0).all()
    mats = list(good)
    mats[where] = bad
    F, piv, flag, X, _ = device_lu(mats, kl, rhs)
    assert flag.tolist() == [int(m == where) for m in range(B.NB)], (name, flag)
    assert np.isnan(X[where]).all()             # the substitution of a flagged matrix writes nothing
    for m in range(B.NB):
        if m != where:
            assert np.array_equal(F[m], Fg[m]) and np.array_equal(piv[m], pg[m]) and np.array_equal(X[m], Xg[m]), (name, m)


def test_flagged_on_entry_comes_back_untouched():
    n, kl = B.FLAG_N, B.FLAG_KL
    mats = B.matrices("gaussian", n, kl, seed=992)
    rhs = np.stack([B.rhs_for(n, m) for m in range(B.NB)])
    Fg, pg, _, Xg, _ = device_lu(mats, kl, rhs)
    F, piv, flag, X, (AB, AB0) = device_lu(mats, kl, rhs, flags_in=[0, 1, 0])
    assert flag.tolist() == [0, 1, 0]
    assert np.array_equal(AB[1].view(np.uint64), AB0[1].view(np.uint64)) and (piv[1] == B.PIV_SENTINEL).all() and np.isnan(X[1]).all()
    for m in (0, 2):
        assert np.array_equal(F[m], Fg[m]) and np.array_equal(piv[m], pg[m]) and np.array_equal(X[m], Xg[m])
