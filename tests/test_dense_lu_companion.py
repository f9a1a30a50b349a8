"""CPU companion of tests/test_gpu_dense_lu.py: the same generators and the same checker functions (tests/dense_lu_cases.py) with scipy's
own factors, converted to the device's layout, standing in for the device. It proves on the CPU that the inputs do what the GPU test needs
them to do and that the checkers accept a correct factorisation:

  * every assertion of the GPU test passes on scipy's factors (so a red GPU test is the kernels' doing);
  * the cyclic class swaps in >= 90 % of its columns at every size from 27 up ((n - 1) / n), the Gaussian class from 129 up (column j
    of a Gaussian matrix keeps its diagonal with probability 1 / (n - j), so n - H_n columns swap on average, H_n = 1 + 1/2 + ... + 1/n:
    85 % at n = 27, 93 % at n = 64; every size is held to three standard deviations below that mean, dense_lu_cases.min_gaussian_swaps);
    n = 1 cannot swap and n = 2 swaps at most its first column; the reversed identity swaps in exactly
    floor(n / 2) columns, each time with the furthest row that is left (the second half of its columns find their pivot already on the
    diagonal, so 90 % is out of that class's reach: the cyclic class is the one that keeps swapping to the end); the control class swaps 0;
  * the exact class: scipy returns the constructed pivots, L and U bit for bit (so LAPACK's tie rule is the lowest row, as the kernels')
    and the constructed integer solutions; about a third of its columns hold two or three equal maxima;
  * every singular flag case gives info > 0 from getrf at the intended column;
  * the sliced longdouble product equals the plain longdouble product.
"""
import numpy as np
import pytest
import scipy.linalg

import dense_lu_cases as C


def stand_in(A, Bv):
    """scipy as the device: factors in the device's layout, piv, flag, solutions"""
    F, piv = C.scipy_as_device(A)
    lu = scipy.linalg.lu_factor(A, check_finite=False)
    return F, piv, np.stack([scipy.linalg.lu_solve(lu, b, check_finite=False) for b in Bv])


@pytest.mark.parametrize("n", C.SIZES)
@pytest.mark.parametrize("cls", [c for c in C.CLASSES if c != "exact"])
def test_checkers_accept_scipy_and_inputs_pivot(cls, n):
    mats = C.matrices(cls, n)
    for m, A in enumerate(mats):
        Bv = C.rhs_for(n, m)
        F, piv, X = stand_in(A, Bv)
        assert np.array_equal(C.to_lapack(F, piv), scipy.linalg.lu_factor(A, check_finite=False)[0])
        err, ref, swaps = C.check_factors(A, F, piv, f"{cls} n={n} m={m}")
        assert err <= C.gate(ref, n) and err == ref
        for e, r in C.check_solves(A, X, Bv, f"{cls} n={n} m={m}"):
            assert e <= C.gate(r, n)
        if cls == "cyclic" and n >= 27 or cls == "gaussian" and n >= 129:
            assert swaps >= 0.9 * n, (cls, n, swaps)
        if cls == "gaussian":
            assert swaps >= C.min_gaussian_swaps(n), (cls, n, swaps)
        if cls == "cyclic":
            assert swaps == n - 1 and (piv[:-1] == n - 1).all()
        if cls == "reversed":
            assert swaps == n // 2 and (piv[:n // 2] == n - 1 - np.arange(n // 2)).all()
        if cls == "control":
            assert swaps == 0


@pytest.mark.parametrize("n", C.SIZES)
def test_exact_class_scipy_returns_the_constructed_factors(n):
    ties = 0
    for m in range(C.NB):
        A, F, piv, tie, X, Bv = C.exact_case(n, np.random.default_rng([C.CLASSES.index("exact") * 100003 + n, m]))
        assert np.array_equal(A, C.matrices("exact", n)[m])
        Fd, pd, Xd = stand_in(A, Bv)
        C.check_exact(A, F, piv, X, Fd, pd, Xd, f"exact n={n} m={m}")
        err, ref, swaps = C.check_factors(A, Fd, pd, f"exact n={n} m={m}")
        assert err == 0.0 and ref == 0.0
        for e, r in C.check_solves(A, Xd, Bv, f"exact n={n} m={m}"):
            assert e == 0.0
        ties += int(tie.sum())
        if n >= 27:
            assert swaps >= n // 3, (n, swaps)
    if n >= 27:
        assert ties >= 0.2 * C.NB * n


@pytest.mark.parametrize("name", sorted(C.FLAG_CASES))
def test_flag_cases_are_singular_where_intended(name):
    A, col = C.flag_case(name)
    if col is None:
        assert np.count_nonzero(~np.isfinite(A)) == 1
        return
    lu, piv, info = scipy.linalg.lapack.dgetrf(A)
    assert info == col + 1, (name, info, col)


def test_layout_round_trip_and_sliced_product():
    rng = np.random.default_rng(5)
    for n in (97, 129):
        A = rng.standard_normal((n, n))
        F, piv = scipy.linalg.lu_factor(A)
        D = C.from_lapack(F, piv)
        assert np.array_equal(C.to_lapack(D, piv), F)
        assert not np.array_equal(D, F)          # the layouts differ as soon as a later panel swaps
    n = 150
    L = np.tril(rng.standard_normal((n, n)), -1) + np.eye(n)
    U = np.triu(rng.standard_normal((n, n))) * 10.0 ** rng.integers(-3, 4, size=(n, 1))
    plain = L.astype(C.LD) @ U.astype(C.LD)
    sliced = C.matmul_ld(L, U)
    assert float(C.fro(plain - sliced) / C.fro(plain)) <= 2.0 ** -58
