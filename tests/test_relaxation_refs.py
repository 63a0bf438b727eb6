"""CPU proof of tests/relaxation_refs.py: the numpy restatements of the fused write-backs and of the whole Jacobi /
polynomial calls agree with exact rational arithmetic on small-integer data, reproduce the literal answers of the
reference's own tests (testing/jacobi.cu, testing/polynomial.cu), and every mutant is caught on every case matrix."""
from fractions import Fraction

import numpy as np
import pytest

import relaxation_refs as R
from conftest import dense_to_csr
from special_values import bits_differ, same_bits

DTYPES = (np.float64, np.float32)

# case matrices: at most 8 rows, small integers, a nonzero diagonal that is a power of two (so that the exact Jacobi
# quotient is representable), an empty off-diagonal row, a full row, a 1 x 1 matrix
CASES = {
    "one": [[2]],
    "two": [[2, 1], [1, 4]],
    "tridiagonal5": [[2, -1, 0, 0, 0], [-1, 2, -1, 0, 0], [0, -1, 2, -1, 0], [0, 0, -1, 2, -1], [0, 0, 0, -1, 2]],
    "jacobi5": [[1, 1, 2, 0, 0], [3, 2, 0, 0, 5], [0, 0, 0.5, 0, 0], [0, 6, 7, 4, 0], [0, 8, 0, 0, 8]],
    "full_row8": [[4, 0, 0, 0, 0, 0, 0, 1], [0, 2, 0, 0, 0, 0, 0, 0], [1, 2, 8, 3, -4, 5, -6, 7], [0, 0, 0, 1, 0, 0, 0, 0],
                  [0, 3, 0, 0, 2, 0, 0, 0], [0, 0, 0, 0, 0, 4, -2, 0], [5, 0, 0, 0, 0, 0, 1, 0], [0, 0, 0, -3, 0, 0, 0, 2]],
}
RECT = {"rect3x5": [[1, 0, 2, 0, 0], [0, 0, 0, 0, 0], [0, 3, 0, -1, 4]]}   # the axpby form takes rectangular matrices (and an empty row)


def _csr(name, dtype):
    return dense_to_csr((CASES | RECT)[name], dtype)


def _ints(rng, n, dtype):
    return rng.integers(-4, 5, size=n).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(CASES) + list(RECT))
def test_axpby_form_against_exact_arithmetic(name, dtype):
    Ap, Aj, Ax = _csr(name, dtype)
    rows, cols = len(Ap) - 1, len((CASES | RECT)[name][0])
    rng = np.random.default_rng(len(name))
    for alpha, beta in ((-1, 1), (1, -3), (2, 0.5)):
        x, z = _ints(rng, cols, dtype), _ints(rng, rows, dtype)
        got = R.spmv_axpby(Ap, Aj, Ax, x, alpha, beta, z)
        want = R.exact_axpby(Ap, Aj, Ax, x, alpha, beta, z)
        assert got.dtype == dtype and [Fraction(float(g)) for g in got] == want


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(CASES))
def test_jacobi_form_against_exact_arithmetic(name, dtype):
    Ap, Aj, Ax = _csr(name, dtype)
    n = len(Ap) - 1
    rng = np.random.default_rng(7 + len(name))
    diag = R.extract_diagonal(Ap, Aj, Ax)
    assert [float(d) for d in diag] == [CASES[name][i][i] for i in range(n)]
    for omega in (1, 0.5, -0.25):
        x, b = _ints(rng, n, dtype), _ints(rng, n, dtype)
        got = R.jacobi_sweep(Ap, Aj, Ax, diag, b, x, omega)
        assert [Fraction(float(g)) for g in got] == R.exact_jacobi(Ap, Aj, Ax, diag, b, x, omega)
        assert np.array_equal(R.Jacobi(Ap, Aj, Ax, omega)(b, x), got)


@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_jacobi_answers(dtype):
    Ap, Aj, Ax = _csr("jacobi5", dtype)
    got = R.Jacobi(Ap, Aj, Ax)(np.full(5, 5, dtype), np.full(5, -1, dtype))
    same_bits(got, np.array([8, 6.5, 10, 4.5, 1.625], dtype), "5 x 5 Jacobi")
    Ap, Aj, Ax = dense_to_csr([[2, 1], [1, 3]], dtype)
    b, x = np.full(2, 5, dtype), np.full(2, -1, dtype)
    for relax, args in ((R.Jacobi(Ap, Aj, Ax, 0.5), ()), (R.Jacobi(Ap, Aj, Ax, 1.0), (0.5,))):   # default omega / overridden
        same_bits(relax(b, x, *args), np.array([1, 0.5], dtype), "2 x 2 weighted Jacobi")   # -1 + 0.5 * 8 / 2, -1 + 0.5 * 9 / 3: exact


def test_reference_chebyshev_coefficients():
    got = R.chebyshev_polynomial_coefficients(1.0, 1.0, 2.0)
    want = [-0.32323232, 1.45454545, -2.12121212, 1.0]
    assert got.dtype == np.float64 and len(got) == 4
    assert all(abs(g - w) < 5e-9 for g, w in zip(got, want)), got   # the 8 digits the reference test gives
    assert R.chebyshev_polynomial_coefficients(1.0, dtype=np.float32).dtype == np.float32


@pytest.mark.parametrize("dtype", DTYPES)
def test_polynomial_call_against_exact_arithmetic(dtype):
    """The reference's polynomial cases (tridiagonal 5 x 5, b = 0, x0 = 0..4) with coefficients that are exact in binary, so
    that every step is exact: degree 1 gives x0 + c r, three coefficients give x0 + c0 A^2 r + c1 A r + c2 r."""
    Ap, Aj, Ax = _csr("tridiagonal5", dtype)
    A = np.array(CASES["tridiagonal5"], dtype=object)
    b, x0 = np.zeros(5, dtype), np.arange(5, dtype=dtype)
    fx = np.array([Fraction(int(v)) for v in x0], dtype=object)
    r = -A.dot(fx)
    got = R.Polynomial(Ap, Aj, Ax, [-0.25, 99])(b, x0, [-0.25])
    assert [Fraction(float(g)) for g in got] == list(fx + Fraction(-1, 4) * r)
    coef = [-0.125, 1.0, -2.0]
    got = R.Polynomial(Ap, Aj, Ax, coef)(b, x0, coef)
    want = fx + Fraction(-1, 8) * A.dot(A.dot(r)) + A.dot(r) + Fraction(-2) * r
    assert [Fraction(float(g)) for g in got] == list(want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_polynomial_constructor_shortcut_and_state(dtype):
    Ap, Aj, Ax = _csr("tridiagonal5", dtype)
    T = np.dtype(dtype).type
    relax = R.Polynomial(Ap, Aj, Ax, [0.5, -2, 7])
    same_bits(relax.default_coefficients, np.array([-0.5, 2], dtype), "drops the last coefficient, negates the rest")
    # x == 0: residual = b without a multiply -- with an infinite entry in A the computed residual b - A 0 would be NaN
    Ainf = Ax.copy()
    Ainf[0] = np.inf
    b, x = np.arange(1, 6, dtype=dtype), np.zeros(5, dtype)
    got = R.Polynomial(Ap, Aj, Ainf, [0.5, 7])(b, x)
    same_bits(got, T(1) * (T(-0.5) * b + T(0) * np.zeros(5, dtype)) + x, "the zero-norm shortcut")
    assert np.isnan(R.spmv_axpby(Ap, Aj, Ainf, x, -1.0, 1.0, b)[0])
    # the default-coefficient call equals the explicit call with the same coefficients, and h persists between calls
    rng = np.random.default_rng(5)
    b, x = rng.standard_normal(5).astype(dtype), rng.standard_normal(5).astype(dtype)
    r1, r2 = R.Polynomial(Ap, Aj, Ax, [0.5, -2, 7]), R.Polynomial(Ap, Aj, Ax, [1])
    same_bits(r1(b, x), r2(b, x, [-0.5, 2]), "default against explicit coefficients")
    r1.h[:] = np.inf                        # stale state shows: 0 * inf = NaN, exactly as the class's axpby(residual, h, h, c, 0)
    assert np.isnan(r1(b, x)).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_is_caught_on_every_case_matrix(name, dtype, mutant):
    """Inexact data (seeded normal values, omega / alpha / beta with inexact products): on each case matrix the mutant's result
    differs in its bits from the true one for at least one of 32 decks.  sum_from_y is also caught on small-integer data, where
    nothing rounds."""
    Ap, Aj, _ = _csr(name, dtype)
    n = len(Ap) - 1
    caught_axpby = caught_jacobi = False
    for seed in range(32):
        rng = np.random.default_rng(1000 * len(name) + seed)
        Ax = rng.standard_normal(len(Aj)).astype(dtype)
        x, b, z = (rng.standard_normal(n).astype(dtype) for _ in range(3))
        diag = R.extract_diagonal(Ap, Aj, Ax)
        alpha, beta, omega = 1.0 / 3.0, 0.7, 2.0 / 3.0
        if mutant != "divide_first":
            caught_axpby |= bool(bits_differ(R.spmv_axpby(Ap, Aj, Ax, x, alpha, beta, z, mutant), R.spmv_axpby(Ap, Aj, Ax, x, alpha, beta, z)).any())
        if mutant != "fused_multiply_add":
            caught_jacobi |= bool(bits_differ(R.jacobi_sweep(Ap, Aj, Ax, diag, b, x, omega, mutant), R.jacobi_sweep(Ap, Aj, Ax, diag, b, x, omega)).any())
    if mutant == "sum_from_y":
        _, _, Ai = _csr(name, dtype)
        ones = np.ones(n, dtype)
        assert bits_differ(R.spmv_axpby(Ap, Aj, Ai, ones, 1, 1, ones, mutant), R.spmv_axpby(Ap, Aj, Ai, ones, 1, 1, ones)).any()
        d = R.extract_diagonal(Ap, Aj, Ai)
        assert bits_differ(R.jacobi_sweep(Ap, Aj, Ai, d, ones, ones, 1, mutant), R.jacobi_sweep(Ap, Aj, Ai, d, ones, ones, 1)).any()
    assert caught_axpby or mutant == "divide_first"
    assert caught_jacobi or mutant == "fused_multiply_add"
