"""Inputs and checkers of the dense-LU kernel tests, shared by the GPU test (tests/test_gpu_dense_lu.py: the device's factors) and its CPU
companion (tests/test_dense_lu_companion.py: scipy's factors standing in for the device, through the same functions).

Storage convention of the device (csrc/dc_adjoint_dense.h): factors in place, column-major, panels of PANEL = 32 columns; the row swaps of a
panel are applied inside the panel and to the columns right of it, not to the factored columns left of it (LINPACK across panels, LAPACK
inside one); piv[j] is the absolute row swapped with row j at column j. to_lapack() / from_lapack() convert between that layout and
LAPACK's (every swap applied to the whole row); piv is the same vector in both.

Residuals are accumulated in numpy.longdouble. A longdouble matrix product has no BLAS behind it (53 s at n = 2304), so above n = 129 the
product L U is formed from error-free slices: both factors are cut into pieces of 20 significant bits relative to their row / column
maximum, every piece-by-piece product is then exact in an fp64 GEMM (2 x 20 + log2(n) <= 53 bits), and the products are summed in
longdouble; the dropped remainder is below 2^-70 of the row maximum. test_dense_lu_companion.py checks it against the plain longdouble
product.
"""
import numpy as np
import scipy.linalg

PANEL = 32
SIZES = [1, 2, 27, 31, 32, 33, 63, 64, 65, 96, 97, 129, 1737, 2304]
NB = 3
CLASSES = ["gaussian", "reversed", "cyclic", "control", "exact"]
U53 = 2.0 ** -53
GATE_FACTOR = 8.0
LD = np.longdouble


def ld_of(n):
    return (n + 15) // 16 * 16


# ---------------------------------------------------------------------------------------------------------------- generators
def gaussian(n, rng):
    return rng.standard_normal((n, n))


def reversed_identity(n, rng):
    """the pivot of column j < n / 2 is row n - 1 - j, the furthest row that is left; the columns of the second half find their pivot on
    the diagonal (their row was brought there by the swap of column n - 1 - j): floor(n / 2) swaps"""
    return np.eye(n)[::-1] + 1e-3 * rng.standard_normal((n, n))


def cyclic(n, rng):
    """ones at (i, i + 1) and (n - 1, 0): the pivot of every column but the last is the LAST row (each swap parks the next pivot there), so
    every swap spans all the panels and tiles that are left: n - 1 swaps"""
    A = 1e-3 * rng.standard_normal((n, n))
    A[np.arange(n - 1), np.arange(1, n)] += 1.0
    A[n - 1, 0] += 1.0
    return A


def control(n, rng):
    """like the physical K: symmetric positive definite, diagonally dominant, plus a 5 % non-symmetric part; no swaps"""
    G = rng.standard_normal((n, n)) / np.sqrt(n)
    S = G @ G.T + 4.0 * np.eye(n)
    return S + 0.05 * rng.standard_normal((n, n)) / np.sqrt(n)


def exact_plu(n, rng, repeat=None):
    """A with P A = L U, every intermediate of the elimination exact in fp64: L unit lower with entries in {0, +-1/4, +-1/2}, and +-1 in
    about a third of the columns (two equal maxima), U upper with integers in -2 .. 2 and +-1, +-2, +-4 on the diagonal. The swap
    vector is built from the last column to the first so that partial pivoting with ties to the lowest row picks exactly the constructed
    pivots: in a column with ties the pivot is parked above every tying row. Returns A, the LAPACK-layout factors and piv.
    repeat = (i1, i2), i1 < i2, makes row i2 of L U a copy of row i1 (L's row i2 = its row i1 with a 1 in column i1, U's row i2 zero): the
    elimination cancels it exactly against its twin and meets an exact zero pivot at column i2."""
    L = rng.choice([0.0, 0.25, -0.25, 0.5, -0.5], size=(n, n))
    U = rng.integers(-2, 3, size=(n, n)).astype(np.float64)
    d = rng.choice([1.0, -1.0, 2.0, -2.0, 4.0, -4.0], size=n)
    L = np.tril(L, -1)
    U = np.triu(U, 1) + np.diag(d)
    tie = np.zeros(n, dtype=bool)
    for j in range(n - 1):
        if rng.random() < 1.0 / 3:
            rows = rng.choice(np.arange(j + 1, n), size=min(2, n - 1 - j), replace=False)
            L[rows, j] = rng.choice([1.0, -1.0], size=len(rows))
            tie[j] = True
    if repeat is not None:
        i1, i2 = repeat
        L[i2, :i1] = L[i1, :i1]; L[i2, i1] = 1.0; L[i2, i1 + 1:i2] = 0.0
        U[i2, i2:] = 0.0
        tie[i1] = True
    F = L + U
    B = (L + np.eye(n)) @ U                       # exact: sums of at most n multiples of 1/4 below 2 n
    piv = np.arange(n)
    pos = np.arange(n)                            # pos[i] = where the row of final position i sits before the swap of the current column
    at = np.arange(n)                             # at[p] = the final position of the row that sits at p
    for j in range(n - 1, -1, -1):
        hi = n                                    # the pivot may be parked at j .. hi - 1
        if tie[j]:
            hi = int(pos[np.nonzero(np.abs(L[:, j]) == 1.0)[0]].min())
        p = j if hi <= j + 1 else int(rng.integers(j + 1, hi)) if rng.random() < 0.9 else j
        piv[j] = p
        a, b = at[j], at[p]                       # the swap of column j: positions j and p trade rows
        at[j], at[p] = b, a
        pos[a], pos[b] = p, j
    A = B.copy()
    for j in range(n - 1, -1, -1):
        if piv[j] != j:
            A[[j, piv[j]]] = A[[piv[j], j]]
    return A, F, piv, tie


def exact_case(n, rng):
    """exact_plu with an integer solution and its exact right-hand sides"""
    A, F, piv, tie = exact_plu(n, rng)
    X = rng.integers(-4, 5, size=(3, n)).astype(np.float64)
    return A, F, piv, tie, X, X @ A.T             # exact: multiples of 1/4 far below 2^53


GENERATORS = dict(gaussian=gaussian, reversed=reversed_identity, cyclic=cyclic, control=control)


def matrices(cls, n, seed=None):
    """the NB matrices of one call (fixed seeds)"""
    seed = CLASSES.index(cls) * 100003 + n if seed is None else seed
    out = []
    for m in range(NB):
        rng = np.random.default_rng([seed, m])
        out.append(exact_plu(n, rng)[0] if cls == "exact" else GENERATORS[cls](n, rng))
    return out


def rhs_for(n, seed):
    """the three right-hand sides of a matrix: Gaussian, a unit vector, all ones"""
    rng = np.random.default_rng([seed, 77])
    e = np.zeros(n)
    e[int(rng.integers(0, n))] = 1.0
    return np.stack([rng.standard_normal(n), e, np.ones(n)])


# flag cases: name -> (n, builder returning the bad matrix and, where getrf defines one, the column of the zero pivot)
def zero_column(n, c, rng):
    A = rng.standard_normal((n, n))
    A[:, c] = 0.0
    return A, c


def repeated_row(n, i1, i2, rng):
    """an integer matrix with two equal rows, from the exact class (times 4: integers) so that no rounding hides the zero pivot: the twin
    rows tie at column i1, the lower one is cancelled exactly, and column i2 is left without a pivot"""
    A = 4.0 * exact_plu(n, rng, repeat=(i1, i2))[0]
    assert np.array_equal(A, np.round(A)) and sum(np.array_equal(A[i], A[k]) for i in range(n) for k in range(i)) >= 1
    return A, i2


def one_bad_entry(n, value, rng):
    A = rng.standard_normal((n, n))
    A[int(rng.integers(0, n)), int(rng.integers(0, n))] = value
    return A, None


FLAG_N = 97
FLAG_CASES = {
    "zero_col_0": lambda rng: zero_column(FLAG_N, 0, rng),
    "zero_col_31": lambda rng: zero_column(FLAG_N, 31, rng),
    "zero_col_32": lambda rng: zero_column(FLAG_N, 32, rng),
    "zero_col_last": lambda rng: zero_column(FLAG_N, FLAG_N - 1, rng),
    "zero_col_last_n27": lambda rng: zero_column(27, 26, rng),
    "repeated_row": lambda rng: repeated_row(FLAG_N, 17, 40, rng),
    "repeated_row_last": lambda rng: repeated_row(FLAG_N, 60, FLAG_N - 1, rng),
    "nan_entry": lambda rng: one_bad_entry(FLAG_N, np.nan, rng),
    "inf_entry": lambda rng: one_bad_entry(FLAG_N, np.inf, rng),
    "neg_inf_entry": lambda rng: one_bad_entry(FLAG_N, -np.inf, rng),
}


def flag_case(name):
    return FLAG_CASES[name](np.random.default_rng([4242, sorted(FLAG_CASES).index(name)]))


# ---------------------------------------------------------------------------------------------------------------- layouts
def to_lapack(F, piv):
    """device layout -> LAPACK layout: the swaps of every panel, applied to the columns left of it"""
    F = np.array(F, copy=True)
    n = F.shape[0]
    for k0 in range(PANEL, n, PANEL):
        for j in range(k0, min(k0 + PANEL, n)):
            p = int(piv[j])
            if p != j:
                F[[j, p], :k0] = F[[p, j], :k0]
    return F


def from_lapack(F, piv):
    """LAPACK layout -> device layout (the inverse of to_lapack)"""
    F = np.array(F, copy=True)
    n = F.shape[0]
    for k0 in range((n - 1) // PANEL * PANEL, 0, -PANEL):
        for j in range(min(k0 + PANEL, n) - 1, k0 - 1, -1):
            p = int(piv[j])
            if p != j:
                F[[j, p], :k0] = F[[p, j], :k0]
    return F


def scipy_as_device(A):
    """scipy's factors of A in the device's layout, and its swap vector (the same convention as the device's piv: 0-based absolute rows)"""
    F, piv = scipy.linalg.lu_factor(A, check_finite=False)
    return from_lapack(F, piv), piv.astype(np.int32)


def permute_rows(A, piv):
    """P A: the swaps of piv applied in column order"""
    PA = np.array(A, copy=True)
    for j, p in enumerate(piv):
        if p != j:
            PA[[j, p]] = PA[[p, j]]
    return PA


# ---------------------------------------------------------------------------------------------------------------- longdouble
def _slices(M, axis, bits=20, count=4):
    R = np.array(M, dtype=np.float64, copy=True)
    out = []
    for _ in range(count):
        mu = np.max(np.abs(R), axis=axis, keepdims=True)
        e = np.ceil(np.log2(np.where(mu > 0, mu, 1.0))).astype(np.int64)
        sigma = np.ldexp(0.75, (e + 54 - bits).astype(np.int32))       # ulp(sigma) = 2^(e + 1 - bits)
        H = (R + sigma) - sigma
        R = R - H
        out.append(H)
    return out


def matmul_ld(A, B):
    """A B accumulated in longdouble (see the module docstring)"""
    n = A.shape[1]
    if n <= 129:
        return A.astype(LD) @ B.astype(LD)
    assert 2 * 20 + np.log2(n) <= 53
    sa, sb = _slices(A, 1), _slices(B, 0)
    S = np.zeros((A.shape[0], B.shape[1]), dtype=LD)
    pairs = sorted(((i, j) for i in range(len(sa)) for j in range(len(sb)) if i + j <= 3), key=lambda q: -(q[0] + q[1]))
    for i, j in pairs:                                                  # small terms first
        S += (sa[i] @ sb[j]).astype(LD)
    return S


def fro(M):
    M = np.asarray(M, dtype=LD)
    return np.sqrt(np.sum(M * M))


def factor_backward_error(A, F_device, piv):
    """|P A - L U|_F / |A|_F in longdouble; P from piv, L and U from the device-layout factors"""
    n = A.shape[0]
    F = to_lapack(F_device, piv)
    L = np.tril(F, -1) + np.eye(n)
    U = np.triu(F)
    # matmul_ld's own error: n roundings of 2^-64 in the longdouble sums plus a dropped remainder below 2^-70, about 2^-11 of the
    # gate's floor n 2^-53
    R = permute_rows(A, piv).astype(LD) - matmul_ld(L, U)
    return float(fro(R) / fro(A))


def solve_backward_error(A, x, b):
    """|b - A x| / (|A|_F |x| + |b|) in longdouble"""
    Al, xl, bl = A.astype(LD), np.asarray(x, dtype=LD), np.asarray(b, dtype=LD)
    num, den = fro(bl - Al @ xl), fro(Al) * fro(xl) + fro(bl)
    return float(num / den) if den > 0 else float(num)


def min_gaussian_swaps(n):
    """Column j of a Gaussian matrix keeps its diagonal as the pivot with probability 1 / (n - j): the columns without a swap number
    H_n = 1 + 1/2 + ... + 1/n on average with a variance below H_n. Three standard deviations below the mean; >= 0.9 n from n = 129."""
    H = float(np.sum(1.0 / np.arange(1, n + 1)))
    return n - H - 3.0 * np.sqrt(H)


def gate(reference_error, n):
    """8 x the reference's own error, or one unit n u of the textbook bound where that is larger (scipy's error is exactly 0 on the
    smallest cases)"""
    return max(GATE_FACTOR * reference_error, n * U53)


# ---------------------------------------------------------------------------------------------------------------- checkers
def check_factors(A, F_device, piv, label):
    """the assertions every class gets on the factors; returns (backward error, scipy's backward error, swap count)"""
    n = A.shape[0]
    piv = np.asarray(piv)
    assert F_device.shape == (n, n) and piv.shape == (n,)
    assert np.isfinite(F_device).all(), f"{label}: non-finite factor entries"
    assert ((piv >= np.arange(n)) & (piv < n)).all(), f"{label}: piv out of range"
    Lmax = float(np.abs(np.tril(F_device, -1)).max()) if n > 1 else 0.0
    assert Lmax <= 1.0, f"{label}: |L| max {Lmax!r} > 1: a pivot was not its column's maximum"
    err = factor_backward_error(A, F_device, piv)
    Fs, ps = scipy_as_device(A)
    ref = factor_backward_error(A, Fs, ps)
    return err, ref, int(np.count_nonzero(piv != np.arange(n)))


def check_solves(A, X, Bv, label):
    """the assertions every class gets on the solutions X [3][n] of the right-hand sides Bv [3][n]; returns [(error, scipy's error)]"""
    assert np.isfinite(X).all(), f"{label}: non-finite solution entries"
    lu = scipy.linalg.lu_factor(A, check_finite=False)
    out = []
    for x, b in zip(X, Bv):
        out.append((solve_backward_error(A, x, b), solve_backward_error(A, scipy.linalg.lu_solve(lu, b, check_finite=False), b)))
    return out


def check_exact(A, F_expected, piv_expected, X_expected, F_device, piv, X, label):
    """the exact class: pivots, L, U and the integer solutions bit for bit"""
    assert np.array_equal(np.asarray(piv), piv_expected), f"{label}: pivot rows differ from the constructed ones"
    assert np.array_equal(to_lapack(F_device, piv), F_expected), f"{label}: L / U differ from the constructed factors"
    assert np.array_equal(X, X_expected), f"{label}: the solutions are not the constructed integers"
