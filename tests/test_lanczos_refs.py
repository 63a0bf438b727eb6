"""CPU tests (-m "not gpu") of the numpy restatements of tests/lanczos_refs.py, the references of the Lanczos and gemm tests.

gemm_ref: exact rational arithmetic on small integer-valued operands; math.fsum within k * eps * sum|terms| otherwise; its three mutants
(descending j, fused multiply-add, a chain started from the first product) are each caught by a deck.
tridiagonal_eigen: against scipy.linalg.eigh_tridiagonal(..., lapack_driver='stev') (the default driver did not converge on a Lanczos T taken
to m = N) within n * eps * ||T||_inf on the values and on ||T z - lambda z||, and n * eps on |Z^T Z - I|.
lanczos: the cases of the host and device programs meet their own bars; the reference's reorthogonalisation window of ten is kept as a mutant.

Window mutant, float, the library's start vector (max |E^T E - I| over the returned vectors; window = 0 is the header's rule):
  7 x 5    LA 4, SA 4, BE 5: 1.0 (a Ritz pair returned twice) with window = 10;  <= 0.022 m eps with window = 0
  16 x 12  LA 4, SA 4, BE 5: 0.997 - 1.0 with window = 10;                       <= 0.011 m eps with window = 0
"""
import math
from fractions import Fraction

import numpy as np
import pytest

import lanczos_refs as R

TYPES = (np.float64, np.float32)


# ---- gemm_ref ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TYPES)
def test_gemm_ref_is_exact_on_small_integers(T):
    rng = np.random.default_rng(5)
    for m, k, n in ((1, 1, 1), (3, 0, 2), (5, 7, 3), (9, 70, 9)):
        A, B = rng.integers(-9, 10, (m, k)).astype(T), rng.integers(-9, 10, (k, n)).astype(T)
        C = R.gemm_ref(A, B)
        assert C.dtype == T and C.shape == (m, n)
        for i in range(m):
            for c in range(n):
                assert Fraction(float(C[i, c])) == sum((Fraction(float(A[i, j])) * Fraction(float(B[j, c])) for j in range(k)), Fraction(0))
        if k == 0:
            assert not np.signbit(C).any()


@pytest.mark.parametrize("T", TYPES)
def test_gemm_ref_against_fsum(T):
    rng = np.random.default_rng(6)
    eps = float(np.finfo(T).eps)
    for m, k, n in ((4, 1, 2), (6, 5, 3), (3, 70, 2)):
        A, B = rng.standard_normal((m, k)).astype(T), rng.standard_normal((k, n)).astype(T)
        C = R.gemm_ref(A, B)
        for i in range(m):
            for c in range(n):
                terms = [float(A[i, j]) * float(B[j, c]) for j in range(k)]
                assert abs(float(C[i, c]) - math.fsum(terms)) <= k * eps * math.fsum(abs(t) for t in terms)


@pytest.mark.parametrize("T", TYPES)
def test_gemm_ref_mutants_are_caught(T):
    big = T(2.0) ** (np.finfo(T).nmant + 1)
    # ascending: (big + 1) + 1 = big (each 1 is lost); descending: (1 + 1) + big = big + 2
    A, B = np.array([[big, 1, 1]], T), np.ones((3, 1), T)
    assert R.gemm_ref(A, B)[0, 0] == big and R.gemm_ref(A, B, "descending")[0, 0] == big + T(2)
    # unfused: -fl(x x) + fl(x x) = 0; fused: the rounding error of the second product survives
    x = T(1) + T(np.finfo(T).eps)
    A, B = np.array([[-(x * x), x]], T), np.array([[1], [x]], T)
    assert R.gemm_ref(A, B)[0, 0] == 0 and R.gemm_ref(A, B, "fma")[0, 0] != 0
    # +0 + (-0) = +0; a chain started from the product keeps -0
    A, B = np.array([[-0.0]], T), np.array([[3.0]], T)
    assert not np.signbit(R.gemm_ref(A, B)[0, 0]) and np.signbit(R.gemm_ref(A, B, "first_product")[0, 0])


# ---- tridiagonal_eigen ---------------------------------------------------------------------------------------------------------------------
def tridiagonal_decks():
    run = R.run_case((7, 5, "f64", R.LA, 4, "Full", 1e-10))   # taken to m = N = 35: a tiny trailing beta
    assert run.iterations == 35
    w21 = np.abs(np.arange(-10, 11)).astype(float)
    return {
        "n1": ([3.5], []),
        "n2": ([2.0, -1.0], [0.5]),
        "n2_equal": ([1.0, 1.0], [1e-3]),
        "zero_in_the_middle": ([4.0, 3.0, 2.0, 1.0, 5.0], [1.0, 0.0, 0.5, 0.25]),
        "all_zero": ([3.0, -1.0, 2.0, 2.0], [0.0, 0.0, 0.0]),
        "graded": ([10.0 ** -i for i in range(8)], [10.0 ** -(i + 1) for i in range(7)]),
        "graded_up": ([10.0 ** (i - 7) for i in range(8)], [10.0 ** (i - 7) for i in range(7)]),
        "wilkinson21": (list(w21), [1.0] * 20),
        "lanczos_7x5": (list(run.alphas[:35]), list(run.betas[:34])),
    }


def check_tridiagonal(name, d, e, w, Z):
    """The bars of the issue on one answer (w, Z) for the deck (d, e)."""
    from scipy.linalg import eigh_tridiagonal
    n = len(d)
    T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
    norm = np.max(np.sum(np.abs(T), 1))
    eps = np.finfo(np.float64).eps
    want = eigh_tridiagonal(np.array(d), np.array(e), eigvals_only=True, lapack_driver="stev") if n > 1 else np.array(d)
    figures = (np.max(np.abs(w - want)) / (n * eps * norm), np.max(np.linalg.norm(T @ Z - Z * w, axis=0)) / (n * eps * norm),
               np.max(np.abs(Z.T @ Z - np.eye(n))) / (n * eps))
    print(name, "n", n, "value error, residual, orthogonality over their bars:", figures)
    assert np.all(np.diff(w) >= 0), name
    assert max(figures) <= 1.0, (name, figures)


@pytest.mark.parametrize("name", list(tridiagonal_decks()))
def test_tridiagonal_restatement_against_stev(name):
    d, e = tridiagonal_decks()[name]
    ok, w, Z = R.tridiagonal_eigen(d, e)
    assert ok
    check_tridiagonal(name, d, e, w, Z)
    ok, w2, none = R.tridiagonal_eigen(d, e, vectors=False)
    assert ok and none is None and np.array_equal(w, w2)


def test_tridiagonal_restatement_reports_failure():
    assert R.tridiagonal_eigen([], [])[0]
    assert not R.tridiagonal_eigen([1.0, math.nan, 2.0], [1.0, 1.0])[0]
    assert not R.tridiagonal_eigen(list(range(30)), [1.0] * 29, sweeps_allowed=0)[0]


# ---- the Lanczos loop ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_restated_loop_meets_the_bars_of_the_programs(case):
    r = R.run_case(case)
    assert r.iterations <= 170
    R.check_pairs(case, r.values.astype(np.float64), r.vectors.astype(np.float64), r.iterations, r.converged, what="restatement")
    if case[:2] == (16, 12) and case[5] == "None" and case[2] == "f64":
        assert r.converged and r.iterations == 55


def test_window_of_ten_is_a_mutant():
    """The reference's modifiedGramSchmidt looks at the last ten vectors only: in float the returned vectors then hold a Ritz pair twice
    (max |E^T E - I| > 0.5), while all stored vectors (window = 0) stay under m eps on every case."""
    caught = []
    for case in R.CASES:
        nx, ny, t, part, count, reorth, tol = case
        if reorth != "Full":
            continue
        eps = float(np.finfo(R.TYPES[t]).eps)
        good = R.run_case(case)
        E = good.vectors.astype(np.float64)
        assert np.max(np.abs(E.T @ E - np.eye(E.shape[1]))) <= good.iterations * eps, case
        if t == "f32" and (nx, ny) in ((7, 5), (16, 12)) and count > 1:
            bad = R.run_case(case, window=10)
            E = bad.vectors.astype(np.float64)
            worst = np.max(np.abs(E.T @ E - np.eye(E.shape[1])))
            print(case, "window = 10: max |E^T E - I| =", worst)
            if worst > 0.5:
                caught.append(case)
    assert len(caught) >= 1, "no case shows the loss of orthogonality of the window of ten"
    assert (7, 5, "f32", R.LA, 4, "Full", 1e-6) in caught and (16, 12, "f32", R.SA, 4, "Full", 1e-6) in caught


def test_restart_and_clipping_in_the_restatement():
    eye = R.lanczos(lambda v: v.copy(), 6, np.float64, 2, R.Options(computeEigVecs=True, reorth="Full", tol=1e-10))
    assert eye.restarts >= 1 and np.sum(eye.betas[:5] == 0) == eye.restarts and np.allclose(eye.values, 1.0, atol=1e-14)   # a restart stores beta = 0
    D = np.diag([-5.0, 2.0])
    both = R.lanczos(lambda v: D @ v, 2, np.float64, 9, R.Options(computeEigVecs=True, reorth="Full", eigPart=R.BE))
    assert np.allclose(both.values, [-5.0, 2.0], atol=1e-14)
    assert len(R.lanczos(lambda v: v, 0, np.float64, 3, R.Options()).values) == 0
    assert len(R.lanczos(lambda v: v, 6, np.float64, 0, R.Options()).values) == 0
    # N = 1 with the default options (no reorthogonalisation): the restart vector has norm 0 and the loop ends there -- at the first step, or at
    # the second when the normalised start is an ulp off 1 and the first residual is rounding noise
    one = R.lanczos(lambda v: np.float64(3.5) * v, 1, np.float64, 1, R.Options())
    assert one.iterations <= 2 and one.restarts == 1 and not one.converged and one.values.tolist() == [3.5]
