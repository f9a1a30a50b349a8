"""Inputs, layout conversion and expansion of the band-LU kernel tests, shared by the GPU test (tests/test_gpu_band_lu.py: the device's band
factors) and its CPU companion (tests/test_band_lu_companion.py: scipy's factors standing in for the device, through the same functions).
The checkers are those of tests/dense_lu_cases.py: the band factors are expanded to the dense device layout and handed to them.

Storage convention of the device (csrc/dc_adjoint_band.h): LAPACK band storage, element (r, c) at AB[c][kl + ku + r - c] (column-major,
leading dimension ldab = 2 kl + ku + 1 rounded up to 16, kl = ku), the upper kl rows zero on entry (fill). Factors in place and LINPACK-style
throughout ("pure"): the swap of column j is applied to the columns right of j only, and the multipliers of a column stay in the rows they
were computed in, as in LAPACK's dgbtrf (a band has no room for swapped multipliers). piv[j] is the absolute row swapped with row j at
column j, the same vector as LAPACK's. pure_to_device() applies the swaps of every panel to the panel's own columns left of them, which
gives the dense kernels' layout (LINPACK across panels of 32 columns, LAPACK inside one: dense_lu_cases.to_lapack takes it from there).
"""
import numpy as np
import scipy.linalg

import dense_lu_cases as D

PANEL = D.PANEL
NB = 3
# (n, kl), ku = kl: narrowest band; below one panel; one panel + 1 with a band narrower than a panel; band at panel width - 1 / 0 / + 1;
# a trailing window that is no multiple of the 64 tile; band = whole matrix; the hat's band truncated early; the hat's real shape.
# WIDE_SIZES: a band too wide for the panel kernel's LDS (32 (kl + 32) doubles > 159 KB from kl = 605), which takes its global-memory variant
# k_band_panel<1024, false>: the far-edge (a swap in every column), control and exact (ties) classes; not the Gaussian one, whose solves
# there miss the condition on the inputs (scipy's own scaled residual on a nearly dense 700 x 700 Gaussian matrix is 3.0e-16 > 2e-16).
# The Gaussian class: plain seeds swap in 67 % of the columns on average at kl = 2 (a column keeps its diagonal with probability
# 1 / (kl + 1)), not in the 79 ... 98 % a first run of these sizes gave, so matrices() redraws until scipy swaps in >= 75 %: the condition
# holds by construction there (the smallest measured fraction is exactly 75.0 %, at (40, 2)); from kl = 31 up the first draw passes.
SIZES = [(40, 2), (20, 5), (33, 8), (65, 31), (97, 32), (130, 33), (200, 40), (150, 149), (521, 218), (1737, 218)]
WIDE_SIZES = [(700, 650)]
CLASSES = ["gaussian", "far_edge", "control", "exact"]
PIV_SENTINEL = -7
CASES = [(cls, n, kl) for cls in CLASSES[:3] for n, kl in SIZES] + [(cls, n, kl) for cls in ("far_edge", "control") for n, kl in WIDE_SIZES]


def ldab_of(kl):
    return (3 * kl + 1 + 15) // 16 * 16


def npiv_of(n):
    return (n + 15) // 16 * 16


def band_mask(n, kl, ku):
    """True where |row - column| is inside the band: row - column <= kl and column - row <= ku"""
    d = np.arange(n)[:, None] - np.arange(n)[None, :]
    return (d <= kl) & (-d <= ku)


# ---------------------------------------------------------------------------------------------------------------- generators
def gaussian(n, kl, rng):
    return rng.standard_normal((n, n)) * band_mask(n, kl, kl)


def far_edge(n, kl, rng):
    """the pivot of every column c < n - kl is the band's last row c + kl, so every swap spans the whole window and U fills up to offset
    kl + ku"""
    A = 1e-3 * rng.standard_normal((n, n)) * band_mask(n, kl, kl)
    c = np.arange(n)
    A[np.minimum(c + kl, n - 1), c] += 1.0
    return A


def control(n, kl, rng):
    """diagonally dominant: no swaps"""
    return np.eye(n) + 0.01 * rng.standard_normal((n, n)) * band_mask(n, kl, kl)


GENERATORS = dict(gaussian=gaussian, far_edge=far_edge, control=control)


def exact_plu(n, kl, rng):
    """A band matrix (kl = ku) with P A = L U, every intermediate of the elimination exact in fp64, built backwards from its factors:
    A^(n) = U, A^(j) = swap(j, piv[j]) (I + l_j e_j^T) A^(j+1). L has entries in {0, +-1/4, +-1/2}, and +-1 (ties) strictly below the pivot's
    row in about a third of the columns; U integers in -2 .. 2 with +-1, +-2, +-4 on the diagonal. The swaps are disjoint pairs (j, piv[j]),
    piv[j] <= j + kl, so every row moves at most once and its final row index (`home`) is known when its entries are chosen: row U_j may
    reach column home + ku, and a multiplier l_ij is non-zero only where the row it lands in may reach U_j's last column. With ties to the
    lowest row partial pivoting picks exactly the constructed pivots. Returns A, the pure-layout factors (n x n), piv and the tie mask."""
    ku = kl
    piv = np.arange(n)
    src = np.full(n, -1)                          # src[p] = j for a pair (j, p)
    used = np.zeros(n, dtype=bool)
    for j in range(n - 1):
        if used[j] or rng.random() >= 0.8:
            continue
        cand = [p for p in range(j + 1, min(j + kl, n - 1) + 1) if not used[p]]
        if cand:
            p = int(cand[-1] if rng.random() < 0.5 else rng.choice(cand))      # half of the swaps reach the furthest free row
            piv[j] = p; src[p] = j; used[j] = used[p] = True
    F = np.zeros((n, n))
    M = np.zeros((n, n))
    tie = np.zeros(n, dtype=bool)
    for j in range(n - 1, -1, -1):
        home_u = piv[j] if piv[j] != j else (src[j] if src[j] >= 0 else j)
        wide = min(n - 1, home_u + ku)
        E = wide if rng.random() < 0.5 else min(n - 1, min(home_u, j) + ku)
        u = rng.integers(-2, 3, size=E - j + 1).astype(np.float64)
        u[0] = rng.choice([1.0, -1.0, 2.0, -2.0, 4.0, -4.0])
        F[j, j:E + 1] = u
        M[j, j:E + 1] = u
        hi = min(j + kl, n - 1)
        if hi > j:
            rows = np.arange(j + 1, hi + 1)
            home = np.where((src[rows] >= 0) & (src[rows] <= j), src[rows], rows)
            l = rng.choice([0.0, 0.25, -0.25, 0.5, -0.5], size=len(rows))
            below = rows > piv[j]
            if below.any() and rng.random() < 1.0 / 3:
                pick = rng.choice(rows[below], size=min(2, int(below.sum())), replace=False)
                l[pick - (j + 1)] = rng.choice([1.0, -1.0], size=len(pick))
            l[home + ku < E] = 0.0
            tie[j] = bool((np.abs(l) == 1.0).any())
            F[rows, j] = l
            M[j + 1:hi + 1, j:E + 1] += np.outer(l, u)
        if piv[j] != j:
            M[[j, piv[j]]] = M[[piv[j], j]]
    return M, F, piv, tie


def exact_case(n, kl, rng):
    """exact_plu with integer solutions and their exact right-hand sides"""
    A, F, piv, tie = exact_plu(n, kl, rng)
    X = rng.integers(-4, 5, size=(3, n)).astype(np.float64)
    return A, F, piv, tie, X, X @ A.T             # exact: multiples of 1/4 far below 2^53


def seed_of(cls, n, kl):
    return CLASSES.index(cls) * 100003 + 1009 * kl + n


MIN_GAUSSIAN_SWAPS = 0.75


def swap_fraction(A):
    piv = scipy.linalg.lu_factor(A, check_finite=False)[1]
    return np.count_nonzero(piv != np.arange(A.shape[0])) / A.shape[0]


def matrices(cls, n, kl, seed=None):
    """the NB matrices of one call (fixed seeds). The Gaussian class has to swap in >= 75 % of its columns; a column of a band keeps its
    diagonal with probability 1 / (kl + 1), so at kl = 2 only a third of the draws do: the draw is repeated with the next seed until scipy's
    partial pivoting swaps that often (a condition on the input alone; tests/test_band_lu_companion.py asserts it)."""
    seed = seed_of(cls, n, kl) if seed is None else seed
    out = []
    for m in range(NB):
        if cls == "gaussian":
            for t in range(1000):
                A = gaussian(n, kl, np.random.default_rng([seed, m, t]))
                if swap_fraction(A) >= MIN_GAUSSIAN_SWAPS:
                    break
            out.append(A)
            continue
        rng = np.random.default_rng([seed, m])
        out.append(exact_plu(n, kl, rng)[0] if cls == "exact" else GENERATORS[cls](n, kl, rng))
    return out


rhs_for = D.rhs_for

# flag cases: the bad matrix of a call; n = 97 with kl = 32 (three panels and a remainder, a band one panel wide)
FLAG_N, FLAG_KL = 97, 32


def zero_column(c, rng):
    A = gaussian(FLAG_N, FLAG_KL, rng)
    A[:, c] = 0.0
    return A


def one_bad_entry(value, rng):
    A = gaussian(FLAG_N, FLAG_KL, rng)
    c = int(rng.integers(0, FLAG_N))
    r = int(rng.integers(max(0, c - FLAG_KL), min(FLAG_N - 1, c + FLAG_KL) + 1))
    A[r, c] = value
    return A


FLAG_CASES = {
    "zero_col_0": lambda rng: zero_column(0, rng),
    "zero_col_31": lambda rng: zero_column(31, rng),
    "zero_col_32": lambda rng: zero_column(32, rng),
    "zero_col_last": lambda rng: zero_column(FLAG_N - 1, rng),
    "nan_entry": lambda rng: one_bad_entry(np.nan, rng),
    "inf_entry": lambda rng: one_bad_entry(np.inf, rng),
}


def flag_case(name):
    return FLAG_CASES[name](np.random.default_rng([4343, sorted(FLAG_CASES).index(name)]))


# ---------------------------------------------------------------------------------------------------------------- layouts
def to_band(A, kl, fill=np.nan):
    """A (n x n, zero outside the band kl = ku) in the device's band storage AB[column][row of the band], ldab_of(kl) rows per column: the kl
    fill rows zero, every entry that belongs to no matrix element (the corners of the band, the padding rows) = `fill`"""
    n, kv = A.shape[0], 2 * kl
    AB = np.full((n, ldab_of(kl)), fill)
    for c in range(n):
        r0, r1 = max(0, c - kv), min(n - 1, c + kl)
        AB[c, kv + r0 - c:kv + r1 - c + 1] = A[r0:r1 + 1, c]
    return AB


def band_valid(n, kl):
    """mask [n][ldab] of the band-storage entries that belong to a matrix element"""
    return ~np.isnan(to_band(np.zeros((n, n)), kl))


def from_band(AB, n, kl):
    """band storage -> n x n (zero outside kl sub- and kl + ku super-diagonals)"""
    kv = 2 * kl
    F = np.zeros((n, n))
    for c in range(n):
        r0, r1 = max(0, c - kv), min(n - 1, c + kl)
        F[r0:r1 + 1, c] = AB[c, kv + r0 - c:kv + r1 - c + 1]
    return F


def pure_to_device(F, piv):
    """pure LINPACK layout -> the dense kernels' layout: inside every panel, the swap of column j applied to the panel's columns left of j"""
    F = np.array(F, copy=True)
    n = F.shape[0]
    for k0 in range(0, n, PANEL):
        for j in range(k0 + 1, min(k0 + PANEL, n)):
            p = int(piv[j])
            if p != j:
                F[[j, p], k0:j] = F[[p, j], k0:j]
    return F


def lapack_to_pure(F, piv):
    """LAPACK layout (every swap applied to the whole row) -> pure LINPACK layout: the swaps taken back from the columns left of them"""
    F = np.array(F, copy=True)
    for j in range(F.shape[0] - 1, 0, -1):
        p = int(piv[j])
        if p != j:
            F[[j, p], :j] = F[[p, j], :j]
    return F


def scipy_as_band(A, kl):
    """scipy's factors of A as the device would leave them in band storage, and its swap vector"""
    F, piv = scipy.linalg.lu_factor(A, check_finite=False)
    P = lapack_to_pure(F, piv)
    assert not P[~band_mask(A.shape[0], kl, 2 * kl)].any(), "scipy's factors leave the band kl / kl + ku"
    return to_band(P, kl), piv.astype(np.int32)


def expand(AB, piv, n, kl):
    """the device's band factors as the dense device layout dense_lu_cases' checkers take"""
    return pure_to_device(from_band(AB, n, kl), piv)
