"""CPU companion of tests/test_gpu_band_lu.py: the same generators (tests/band_lu_cases.py) and the checkers of tests/dense_lu_cases.py with
scipy's own factors, converted to the device's band layout and expanded again as the GPU test expands the device's, standing in for the
device. It proves on the CPU, with scipy alone, that the inputs do what the GPU test needs them to do:

  * every matrix is zero outside its band, and scipy's factors stay inside kl sub-diagonals and kl + ku super-diagonals (what the band
    storage holds); band storage -> dense -> LAPACK layout gives scipy's factors back bit for bit;
  * far-edge class: the pivot of every column c < n - kl is row c + kl, and U reaches offset kl + ku exactly;
  * control class: zero swaps; Gaussian class: swaps in >= 75 % of the columns;
  * the solves are well conditioned: scipy's scaled residual is <= 2e-16;
  * exact class: scipy returns the constructed pivots, L, U and integer solutions bit for bit (LAPACK's tie rule is the lowest row), with ties
    in some columns and swaps at every size;
  * the zero-column flag cases give a zero pivot at that column in getrf.
"""
import warnings

import numpy as np
import pytest
import scipy.linalg

import band_lu_cases as B
import dense_lu_cases as C


@pytest.mark.parametrize("cls,n,kl", B.CASES)
def test_checkers_accept_scipy_and_inputs_pivot(cls, n, kl):
    for m, A in enumerate(B.matrices(cls, n, kl)):
        label = f"{cls} n={n} kl={kl} m={m}"
        assert not A[~B.band_mask(n, kl, kl)].any(), label
        AB, piv = B.scipy_as_band(A, kl)
        assert np.array_equal(np.isnan(AB), ~B.band_valid(n, kl))
        F = B.expand(AB, piv, n, kl)
        lu = scipy.linalg.lu_factor(A, check_finite=False)
        assert np.array_equal(C.to_lapack(F, piv), lu[0]), label
        err, ref, swaps = C.check_factors(A, F, piv, label)
        assert err <= C.gate(ref, n) and err == ref
        Bv = B.rhs_for(n, m)
        X = np.stack([scipy.linalg.lu_solve(lu, b, check_finite=False) for b in Bv])
        for e, r in C.check_solves(A, X, Bv, label):
            assert e <= C.gate(r, n) and r <= 2e-16, (label, r)
        if cls == "far_edge":
            c = np.arange(max(n - kl, 0))
            assert (piv[:len(c)] == c + kl).all(), label
            U = np.triu(lu[0])
            reach = max(int(np.max(np.nonzero(U[r])[0]) - r) for r in range(n))
            assert reach == min(2 * kl, n - 1), (label, reach)
        if cls == "control":
            assert swaps == 0, label
        if cls == "gaussian":
            assert swaps >= B.MIN_GAUSSIAN_SWAPS * n, (label, swaps)


@pytest.mark.parametrize("n,kl", B.SIZES + B.WIDE_SIZES)
def test_exact_class_scipy_returns_the_constructed_factors(n, kl):
    ties = swaps = 0
    for m in range(B.NB):
        A, F, piv, tie, X, Bv = B.exact_case(n, kl, np.random.default_rng([B.seed_of("exact", n, kl), m]))
        assert np.array_equal(A, B.matrices("exact", n, kl)[m])
        assert not A[~B.band_mask(n, kl, kl)].any() and not F[~B.band_mask(n, kl, 2 * kl)].any()
        lu = scipy.linalg.lu_factor(A, check_finite=False)
        assert np.array_equal(lu[1], piv), (n, kl, m)
        assert np.array_equal(B.lapack_to_pure(lu[0], lu[1]), F), (n, kl, m)
        assert np.array_equal(C.to_lapack(B.pure_to_device(F, piv), piv), lu[0])
        assert np.array_equal(np.stack([scipy.linalg.lu_solve(lu, b, check_finite=False) for b in Bv]), X)
        assert np.abs(np.tril(F, -1)).max() <= 1.0
        ties += int(tie.sum()); swaps += int(np.count_nonzero(piv != np.arange(n)))
    assert ties > 0 and swaps > 0, (n, kl, ties, swaps)


@pytest.mark.parametrize("name", sorted(B.FLAG_CASES))
def test_flag_cases_are_what_they_say(name):
    A = B.flag_case(name)
    assert not np.nan_to_num(A, nan=1.0, posinf=1.0)[~B.band_mask(B.FLAG_N, B.FLAG_KL, B.FLAG_KL)].any()
    if name.startswith("zero_col"):
        c = {"0": 0, "31": 31, "32": 32, "last": B.FLAG_N - 1}[name.split("_")[-1]]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            lu, piv, info = scipy.linalg.lapack.dgetrf(A)
        assert info == c + 1, (name, info)
    else:
        assert np.count_nonzero(~np.isfinite(A)) == 1
