"""CPU tests (-m "not gpu") of the numpy restatements in tests/eigen_refs.py -- the sequences cusp/eigen/*.h run -- against
numpy.linalg.eigvals and the closed forms, in float32 and float64, from 20 random start vectors each.

Criterion: relative error < 0.1, the reference's own (testing/spectral_radius.cu).  With the completed column kept on
breakdown the worst error over 300 starts on these matrices was 0.025 (power iteration, k = 40), 0.027 (Arnoldi and
Lanczos, k = 10) and 0.033 (Lanczos and D^-1 A, k = 8): the criterion has a threefold margin over any start, so it
does not depend on the hash the library uses.  Poisson 4 x 4 is used for the row sums only: its Krylov space breaks down
near step 10 and float32 noise then passes the 1e-10 threshold (errors up to 0.14)."""
import functools
import math

import numpy as np
import pytest

import eigen_refs as E

SEEDS = range(20)
TOL = 0.1
DTYPES = [np.float32, np.float64]
# name -> (dense matrix or grid, rho(A), rho(D^-1 A))
CASES = {
    "diag(-5,2)": (None, 5.0, 1.0),
    "poisson2x2": ((2, 2), 6.0, 1.5),
    "poisson37x41": ((37, 41), 7.987577, 7.987577 / 4),
    "poisson64x3": ((64, 3), 7.411878, 7.411878 / 4),
    "poisson130x9": ((130, 9), 7.901538, 7.901538 / 4),
}


def dense_of(name, dtype=np.float64):
    grid = CASES[name][0]
    return np.diag(np.array([-5, 2], dtype)) if grid is None else E.poisson5pt(*grid, dtype=dtype)


@functools.lru_cache(maxsize=None)
def exact(name):
    """(rho(A), rho(D^-1 A)) from numpy.linalg.eigvals of the float64 matrix."""
    A = dense_of(name)
    rho = float(np.max(np.abs(np.linalg.eigvals(A))))
    grid = CASES[name][0]
    rho_d = rho / 4 if grid is not None else float(np.max(np.abs(np.linalg.eigvals(A / np.diag(A)[:, None]))))
    return rho, rho_d


def operators(name, dtype):
    """(A, D^-1 A) as functions of a vector, and the number of rows."""
    grid = CASES[name][0]
    if grid is None:
        A = dense_of(name, dtype)
        return E.dense_operator(A), E.dense_operator((A / np.diag(A)[:, None]).astype(dtype)), 2
    N = grid[0] * grid[1]
    return E.poisson_operator(*grid, dtype), E.poisson_operator(*grid, dtype, scale=np.full(N, 0.25, dtype)), N


def starts(n, dtype):
    for seed in SEEDS:
        rng = np.random.default_rng(seed)
        yield seed, rng.random(n).astype(dtype), rng.random(32).astype(dtype)


def rel(got, want):
    return abs(got - want) / want


@pytest.mark.parametrize("name", list(CASES))
def test_the_table_is_what_eigvals_says(name):
    rho, rho_d = exact(name)
    assert rel(rho, CASES[name][1]) < 1e-6 and rel(rho_d, CASES[name][2]) < 1e-6
    grid = CASES[name][0]
    if grid is not None:
        assert rel(rho, E.poisson_rho(*grid)) < 1e-12


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(CASES))
def test_power_iteration(name, dtype):
    A, _, n = operators(name, dtype)
    for seed, x0, _ in starts(n, dtype):
        assert rel(E.power_iteration(A, x0, 40), exact(name)[0]) < TOL, seed


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("symmetric,k", [(False, 10), (True, 10), (True, 8)])
def test_ritz_spectral_radius(name, dtype, symmetric, k):
    A, _, n = operators(name, dtype)
    for seed, x0, small in starts(n, dtype):
        assert rel(E.ritz_spectral_radius(A, x0, k, symmetric, x0_small=small), exact(name)[0]) < TOL, seed


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(CASES))
def test_rho_Dinv_A(name, dtype):
    _, DA, n = operators(name, dtype)
    for seed, x0, small in starts(n, dtype):
        assert rel(E.ritz_spectral_radius(DA, x0, 8, False, x0_small=small), exact(name)[1]) < TOL, seed


def test_hessenberg_shapes():
    """A 2 x 2 diagonal matrix breaks down at step 1: the kept column makes the block 2 x 2 (the reference's rule: 1 x 1); without
    breakdown the block is k x k, upper Hessenberg with a positive subdiagonal, tridiagonal and symmetric for Lanczos."""
    x0 = np.random.default_rng(0).random(2)
    A = E.dense_operator(dense_of("diag(-5,2)"))
    assert E.arnoldi(A, x0, 10).shape == (2, 2) and E.lanczos(A, x0, 10).shape == (2, 2)
    assert E.arnoldi(A, x0, 10, keep_column=False).shape == (1, 1) and E.lanczos(A, x0, 10, keep_column=False).shape == (1, 1)
    P, _, n = operators("poisson37x41", np.float64)
    x0 = np.random.default_rng(1).random(n)
    H = E.arnoldi(P, x0, 10)
    assert H.shape == (10, 10) and np.all(np.tril(H, -2) == 0) and np.all(np.diag(H, -1) > 0)
    T = E.lanczos(P, x0, 10)
    assert T.shape == (10, 10) and np.all(np.triu(T, 2) == 0) and np.all(np.tril(T, -2) == 0) and np.array_equal(np.diag(T, 1), np.diag(T, -1))
    assert np.allclose(np.diag(T), np.diag(H), rtol=1e-9) and np.allclose(np.diag(T, -1), np.diag(H, -1), rtol=1e-9)


@pytest.mark.parametrize("symmetric", [False, True])
def test_mutant_dropping_the_completed_column_fails_on_diag(symmetric):
    """The reference's rule (the leading j x j block on breakdown at step j) turns diag(-5, 2) into the Rayleigh quotient of the
    start: it must miss the criterion for some of the 20 starts, while the kept column gives 5 for every one of them."""
    A = E.dense_operator(dense_of("diag(-5,2)"))
    kept, dropped = [], []
    for _, x0, small in starts(2, np.float64):
        kept.append(rel(E.ritz_spectral_radius(A, x0, 10, symmetric, True, small), 5.0))
        dropped.append(rel(E.ritz_spectral_radius(A, x0, 10, symmetric, False, small), 5.0))
    assert max(kept) < 1e-6
    assert max(dropped) >= TOL, dropped


# ---- row sums ----
def csr_of(A):
    Ap = np.concatenate([[0], np.cumsum((A != 0).sum(1))]).astype(np.int32)
    return Ap, A[A != 0]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,want", [("diag(-5,2)", 5), ("poisson2x2", 6), ("poisson4x4", 8), ("poisson37x41", 8)])
def test_row_sum_restatements_give_the_disks(name, want, dtype):
    A = E.poisson5pt(4, 4, dtype) if name == "poisson4x4" else dense_of(name, dtype)
    n = A.shape[0]
    truth = np.abs(A.astype(np.float64)).sum(1)
    Ap, Ax = csr_of(A)
    assert np.array_equal(E.csr_abs_row_sums(Ap, Ax), truth) and truth.max() == want
    # ELL: every row padded with zeros to the longest row, column-major with a pitch beyond the rows
    width, pitch = int(np.diff(Ap).max()), n + 3
    ell = np.zeros(width * pitch, dtype)
    for i in range(n):
        ell[np.arange(Ap[i + 1] - Ap[i]) * pitch + i] = Ax[Ap[i]:Ap[i + 1]]
    assert np.array_equal(E.ell_abs_row_sums(n, width, pitch, ell), truth)
    # HYB: the first entry of every row in ELL, the rest in COO
    ell1 = np.zeros(pitch, dtype)
    ell1[:n] = Ax[Ap[:-1]]
    Ai = np.repeat(np.arange(n), np.diff(Ap) - 1)
    rest = np.concatenate([Ax[Ap[i] + 1:Ap[i + 1]] for i in range(n)]) if len(Ai) else np.zeros(0, dtype)
    assert np.array_equal(E.hyb_abs_row_sums(n, 1, pitch, ell1, Ai, rest), truth)
    # DIA: every diagonal that holds an entry; NaN where the column falls outside the matrix -- never read
    offsets = sorted({int(j - i) for i, j in zip(*np.nonzero(A))})
    dia = np.full(len(offsets) * pitch, np.nan, dtype)
    for d, off in enumerate(offsets):
        for i in range(n):
            if 0 <= i + off < n:
                dia[d * pitch + i] = A[i, i + off]
    assert np.array_equal(E.dia_abs_row_sums(n, n, pitch, offsets, dia), truth)


# ---- the hash and the normalise step ----
@pytest.mark.parametrize("dtype", DTYPES)
def test_random_fill_restatement(dtype):
    for seed in (0, 12345):
        x = E.random_fill(1025, seed, dtype)
        assert x.dtype == dtype and np.all(x >= 0) and np.all(x < 1) and len(np.unique(x)) > 1000
        shift, scale = (11, 2.0 ** -53) if dtype == np.float64 else (40, 2.0 ** -24)
        for i in (0, 1, 63, 1024):
            assert x[i] == dtype((E.random_hash(i, seed) >> shift) * scale)
    assert not np.array_equal(E.random_fill(64, 0, dtype), E.random_fill(64, 1, dtype))
    assert abs(float(np.mean(E.random_fill(70001, 3, dtype))) - 0.5) < 0.01
    assert E.random_hash(0, 0) == 0xE220A8397B1DCDAF   # splitmix64's first output for seed 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_scal_recip_restatement(dtype):
    x = E.random_fill(257, 7, dtype)
    nrm_sq = float(np.dot(x.astype(np.float64), x.astype(np.float64)))
    y = E.scal_recip(x, nrm_sq, True)
    assert y.dtype == dtype and abs(math.sqrt(float(np.dot(y.astype(np.float64), y.astype(np.float64)))) - 1) < 1e-5
    beta = dtype(np.sqrt(np.float64(nrm_sq)))
    assert np.array_equal(y, (dtype(1) / beta) * x)
    assert np.array_equal(E.scal_recip(x, np.max(np.abs(x)), False), (dtype(1) / np.max(np.abs(x))) * x)
