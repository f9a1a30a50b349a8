"""The dense adjoint solve's LU and substitution kernels (csrc/dc_adjoint_dense.hip: k_lu_panel, k_lu_trsm, k_lu_update through
launch_dense_factor, and lu_substitute<1024>) on matrices a scene cannot produce, against scipy.linalg.lu_factor / lu_solve in fp64 with
residuals accumulated in numpy.longdouble. The physical K of the tested scenes hardly swaps a row (tests/test_gpu_dense_adjoint.py), so the
pivot search, the swaps inside a panel and right of it, the layout lu_substitute mirrors and the tie rule are pinned here.

The kernels run through the check library tests/native/dense_lu_check.hip, which includes the product's translation unit as text (no copy)
and is cross-compiled by diffcloth_amd/build.py (build_kernel_checks); this module loads it and does not compile. Inputs, layout
conversion and checkers: tests/dense_lu_cases.py; tests/test_dense_lu_companion.py runs the same checkers on scipy's factors on the CPU.

Every call: 3 different matrices, n in SIZES (below one panel, one panel +- 1, trailing matrices that are no multiple of the 64 x 64 tile,
1737 and the limit 2304), ld = n rounded up to 16, every entry outside the leading n x n block NaN (piv's tail a sentinel) and asserted
bitwise unchanged afterwards; no output NaN. Classes: Gaussian, reversed identity + 1e-3 noise (pivot = the furthest row that is left,
floor(n / 2) swaps), cyclic + 1e-3 noise (pivot = the last row in n - 1 columns), K-like control (no swap), exact dyadic P L U with ties.

The premise that the Gaussian and the reversed class swap in >= 90 % of their columns was wrong: a reversed identity cannot swap more than
floor(n / 2) columns (the swap of column j brings the pivot of column n - 1 - j onto the diagonal), and a Gaussian matrix reaches 90 % only
from n of about 129 (column j keeps its diagonal with probability 1 / (n - j)). The cyclic class was added to carry that condition; the
reversed class is held to its exact pattern, the Gaussian one to its expectation (tests/test_dense_lu_companion.py).

Gates: |L| <= 1 exactly; |P A - L U|_F / |A|_F and |b - A x| / (|A|_F |x| + |b|) at most 8 x scipy's own figure on the same matrix, or
n 2^-53 where that is larger; the exact class bit for bit (piv, L, U, x). Flag cases (zero column at 0, 31, 32, n - 1; an integer matrix
with a repeated row; one NaN, one Inf entry): flag == 1 for that matrix alone, the two other matrices of the call bitwise as without it;
a matrix flagged on entry comes back untouched.

Measured on an MI355X, worst over the sizes and the 3 matrices (101 tests, 47 s, of which the kernels take well under a second: the rest is
the longdouble residuals):
  class      swapped columns (n >= 27)   factor error / scipy's (n >= 27)   factor error / gate   solve error / gate
  gaussian   70.4 ... 99.8 %             1.23                               0.112                 0.157
  reversed   48.1 ... 50.0 %             4.05                               0.125                 0.125
  cyclic     96.3 ... 100 %              3.48                               0.125                 0.125
  control    0                           3.26                               0.111                 0.125
  exact      about 90 % (2077 of 2304), a third of the columns with ties; every error exactly 0, piv / L / U / x bit for bit
No class needs more than 8 x scipy's own error even before the n 2^-53 floor; from n = 63 up the floor is the larger term of the gate.
Mutation check (scratch copies of the check library, not committed; each run once, sizes up to 129): removing k_lu_trsm's swap loop turns
34 of these tests red, `r2 > r` in amax_merge 13 (the exact class and its ties), dropping lu_substitute's piv swap 44, swapping only the
panel columns from j on in k_lu_panel 46.
The first two also as engine builds against tests/test_gpu_dense_adjoint.py (without its n = 2304 case), once each: without k_lu_trsm's swap
loop test_exact_solve_parity_and_mode1_agreement[hat] goes red (the hat's K pivots in about 5 % of its columns) and the other 11 tests stay
green, the flap's included; with `r2 > r` all 12 stay green: only the exact class here sees the tie rule.
"""
import ctypes
import os

import numpy as np
import pytest

import dense_lu_cases as C
from diffcloth_amd import build as dcbuild

pytestmark = pytest.mark.gpu
PIV_SENTINEL = -7
_lib = None


def check_library():
    global _lib
    if _lib is None:
        path = dcbuild.kernel_check_path()
        if not os.path.exists(path):
            pytest.fail(f"{path} is missing: build it with `python -m diffcloth_amd.build` (or __graft_entry__.build()); this test does not compile")
        _lib = ctypes.CDLL(path)
        _lib.dc_check_dense_lu.restype = ctypes.c_int
        _lib.dc_check_dense_lu.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_char_p, ctypes.c_int]
    return _lib


def device_lu(mats, rhs, flags_in=None):
    """One call of the check library on the matrices `mats` [nb] (n x n) with right-hand sides rhs [nb][3][n]. Returns the device-layout
    factors [nb] (row, column), piv [nb][n], flag [nb], x [nb][3][n] (NaN where the kernel wrote nothing), and the raw K buffer.
    Asserts that nothing outside the leading n x n blocks and piv[:n] was written."""
    lib = check_library()
    nb, n = len(mats), mats[0].shape[0]
    ld = C.ld_of(n)
    K = np.full((nb, ld, ld), np.nan)
    for m, A in enumerate(mats):
        K[m, :n, :n] = A.T                      # column-major: K[m][column][row]
    K0 = K.copy()
    piv = np.full((nb, ld), PIV_SENTINEL, dtype=np.int32)
    flag = np.zeros(nb, dtype=np.int32) if flags_in is None else np.array(flags_in, dtype=np.int32)
    rhs = np.ascontiguousarray(rhs, dtype=np.float64)
    x = np.full_like(rhs, np.nan)
    err = ctypes.create_string_buffer(512)
    rc = lib.dc_check_dense_lu(nb, n, ld, K.ctypes.data, piv.ctypes.data, flag.ctypes.data, rhs.shape[1], rhs.ctypes.data, x.ctypes.data, err, 512)
    assert rc == 0, err.value.decode()
    pad = np.ones((ld, ld), dtype=bool)
    pad[:n, :n] = False
    assert np.array_equal(K.view(np.uint64)[:, pad], K0.view(np.uint64)[:, pad]), "an entry outside the leading n x n block was written"
    assert (piv[:, n:] == PIV_SENTINEL).all(), "piv was written beyond n"
    return [K[m, :n, :n].T.copy() for m in range(nb)], piv[:, :n].copy(), flag, x, (K, K0)


@pytest.mark.parametrize("n", C.SIZES)
@pytest.mark.parametrize("cls", [c for c in C.CLASSES if c != "exact"])
def test_factor_and_solve_against_scipy(cls, n):
    mats = C.matrices(cls, n)
    rhs = np.stack([C.rhs_for(n, m) for m in range(C.NB)])
    F, piv, flag, X, _ = device_lu(mats, rhs)
    assert (flag == 0).all()
    worst_f = worst_s = 0.0
    fails = []
    for m, A in enumerate(mats):
        label = f"{cls} n={n} m={m}"
        err, ref, swaps = C.check_factors(A, F[m], piv[m], label)
        solves = C.check_solves(A, X[m], rhs[m], label)
        print(f"[{label}] swaps {swaps}/{n} factor {err:.3e} (scipy {ref:.3e}, gate {C.gate(ref, n):.3e}) solves " +
              " ".join(f"{e:.2e}/{r:.2e}" for e, r in solves))
        worst_f = max(worst_f, err / (C.gate(ref, n) / C.GATE_FACTOR))
        if not err <= C.gate(ref, n):
            fails.append((label, "factor", err, ref))
        for k, (e, r) in enumerate(solves):
            worst_s = max(worst_s, e / (C.gate(r, n) / C.GATE_FACTOR))
            if not e <= C.gate(r, n):
                fails.append((label, f"solve {k}", e, r))
    print(f"[{cls} n={n}] worst ratio to the gate's unit: factor {worst_f:.2f} solve {worst_s:.2f} (gate {C.GATE_FACTOR})")
    assert not fails, fails


@pytest.mark.parametrize("n", C.SIZES)
def test_exact_class_bit_for_bit(n):
    cases = [C.exact_case(n, np.random.default_rng([C.CLASSES.index("exact") * 100003 + n, m])) for m in range(C.NB)]
    F, piv, flag, X, _ = device_lu([c[0] for c in cases], np.stack([c[5] for c in cases]))
    assert (flag == 0).all()
    for m, (A, Fx, px, tie, Xx, Bv) in enumerate(cases):
        label = f"exact n={n} m={m}"
        C.check_exact(A, Fx, px, Xx, F[m], piv[m], X[m], label)
        err, ref, swaps = C.check_factors(A, F[m], piv[m], label)
        print(f"[{label}] swaps {swaps}/{n} tie columns {int(tie.sum())} factor error {err}")
        assert err == 0.0


@pytest.mark.parametrize("name", sorted(C.FLAG_CASES))
@pytest.mark.parametrize("where", [0, 1, 2])
def test_flag_cases(name, where):
    bad, _ = C.flag_case(name)
    n = bad.shape[0]
    good = C.matrices("gaussian", n, seed=991)
    rhs = np.stack([C.rhs_for(n, m) for m in range(C.NB)])
    Fg, pg, flg, Xg, _ = device_lu(good, rhs)
    assert (flg == 0).all()
    mats = list(good)
    mats[where] = bad
    F, piv, flag, X, _ = device_lu(mats, rhs)
    assert flag.tolist() == [int(m == where) for m in range(C.NB)], (name, flag)
    assert np.isnan(X[where]).all()             # the substitution of a flagged matrix writes nothing
    for m in range(C.NB):
        if m != where:
            assert np.array_equal(F[m], Fg[m]) and np.array_equal(piv[m], pg[m]) and np.array_equal(X[m], Xg[m]), (name, m)


def test_flagged_on_entry_comes_back_untouched():
    n = 97
    mats = C.matrices("gaussian", n, seed=992)
    rhs = np.stack([C.rhs_for(n, m) for m in range(C.NB)])
    Fg, pg, _, Xg, _ = device_lu(mats, rhs)
    F, piv, flag, X, (K, K0) = device_lu(mats, rhs, flags_in=[0, 1, 0])
    assert flag.tolist() == [0, 1, 0]
    assert np.array_equal(K[1].view(np.uint64), K0[1].view(np.uint64)) and (piv[1] == PIV_SENTINEL).all() and np.isnan(X[1]).all()
    for m in (0, 2):
        assert np.array_equal(F[m], Fg[m]) and np.array_equal(piv[m], pg[m]) and np.array_equal(X[m], Xg[m])
