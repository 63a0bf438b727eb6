"""CPU tests of the references in blas_extra_refs.py: a wrong reference must not pass a wrong kernel.  Every restatement (a) is
checked against its formula (b) evaluated in exact rational arithmetic, within the bound the GPU tests use."""
import math
from fractions import Fraction

import numpy as np
import pytest

import blas_extra_refs as R

TYPES = [np.float32, np.float64]


def inputs(kernel, T, n, seed):
    rng = np.random.default_rng(seed)
    return {name: rng.standard_normal(n).astype(T) for name in kernel.vecs}


@pytest.mark.parametrize("T", TYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["inexact", "exact"])
@pytest.mark.parametrize("name", sorted(R.KERNELS))
def test_restatement_is_within_the_bound_of_the_exact_formula(name, kind, T):
    kernel = R.KERNELS[name]
    u = Fraction(R.U[T])
    for n in range(1, 9):
        s, v = R.scalars_for(kernel, kind, T), inputs(kernel, T, n, 100 + n)
        got = kernel.restate(T, s, v)
        assert sorted(got) == sorted(kernel.outputs)
        want = kernel.formula(*R.rational(s, v))
        sh, vh = R.higher(T, s, v)
        high = kernel.formula(sh, vh)
        uh = Fraction(float(np.finfo(R.HIGHER[T]).eps)) / 2
        for out in kernel.outputs:
            assert got[out].dtype == T and got[out].shape == (n,)
            value, terms = want[out]
            k = kernel.k[out]
            for i in range(n):
                assert abs(Fraction(float(got[out][i])) - value[i]) <= k * u * terms[i], (name, out, n, i)  # k = kernel.k[out] roundings
                # the higher-precision evaluation the GPU tests compare with: the same k roundings, in its own unit roundoff
                assert abs(Fraction(*high[out][0][i].as_integer_ratio()) - value[i]) <= k * uh * terms[i], (name, out, n, i)
                assert abs(Fraction(*high[out][1][i].as_integer_ratio()) - terms[i]) <= k * uh * terms[i]


@pytest.mark.parametrize("name", sorted(R.KERNELS))
def test_a_wrong_formula_is_outside_the_bound(name):
    """The bound is tight enough to tell formulas apart: one operand's sign flipped moves a result out of it."""
    kernel, T = R.KERNELS[name], np.float64
    s, v = R.scalars_for(kernel, "inexact", T), inputs(kernel, T, 8, 7)
    got = kernel.restate(T, s, v)
    flipped = dict(v)
    flipped[kernel.vecs[0]] = -v[kernel.vecs[0]]
    want = kernel.formula(*R.rational(s, flipped))
    worst = max(abs(Fraction(float(got[out][i])) - want[out][0][i]) / (kernel.k[out] * Fraction(R.U[T]) * want[out][1][i])
                for out in kernel.outputs for i in range(8))
    assert worst > 1


def test_exact_scalars_have_exact_quotients_and_inexact_ones_do_not():
    for kernel in R.KERNELS.values():
        if kernel.by_value:
            continue
        for T in TYPES:
            for num, den in (("rz", "yp"), ("rz_old", "yp"), ("rz_new", "rz_old"), ("rz_new", "rz"), ("rho", "d1"), ("d2", "d3"), ("rz", "yy"), ("num", "den")):
                if num in kernel.scalars and den in kernel.scalars:
                    e, x = R.SCALARS["exact"], R.SCALARS["inexact"]
                    assert Fraction(float(T(e[num] / e[den]))) == Fraction(e[num]) / Fraction(e[den])
                    assert Fraction(float(T(x[num] / x[den]))) != Fraction(x[num]) / Fraction(x[den])
    assert float(np.float32(R.SCALARS["inexact"]["h"])) != R.SCALARS["inexact"]["h"]


def test_sums_name_the_products_of_the_returned_vectors():
    for T in TYPES:
        for name in ("pcg_update", "bicg_s", "bicg_xr", "cr_xr", "cr_py", "axpy_dot"):
            kernel = R.KERNELS[name]
            s, v = R.scalars_for(kernel, "inexact", T), inputs(kernel, T, 8, 3)
            got = kernel.restate(T, s, v)
            for a, b in kernel.sums(T, got, v).values():
                assert a.dtype == T and b.dtype == T
                total, absolute = R.exact_sum(a, b)
                exact = sum(Fraction(float(x)) * Fraction(float(y)) for x, y in zip(a, b))
                assert abs(Fraction(total) - exact) <= Fraction(2.0 ** -52) * Fraction(absolute)
                if T is np.float32:  # products of two floats are exact in double, fsum rounds once
                    assert total == float(exact) or abs(Fraction(total) - exact) <= Fraction(2.0 ** -53) * abs(exact)
    x = np.array([1.5, -2.0, 0.25], np.float32)
    assert R.exact_sum(x, x) == (6.3125, 6.3125) and R.exact_sum(x, -x) == (-6.3125, 6.3125)


def test_amax_reference_takes_the_first_position_and_skips_nans():
    nan, inf = float("nan"), float("inf")
    cases = [
        ([], (0.0, 0)), ([nan, nan], (0.0, 0)), ([0.0], (0.0, 0)), ([-0.0, -0.0], (0.0, 0)),
        ([1.0, -3.0, 3.0, 2.0], (3.0, 1)),        # the negative value comes first: it wins the tie
        ([1.0, 3.0, -3.0], (3.0, 1)),
        ([nan, 2.0, nan, -2.0], (2.0, 1)),        # NaNs skipped, first of the tie
        ([nan, 1.0, -inf, inf], (inf, 2)),
        ([-5.0, 1.0], (5.0, 0)),
    ]
    for x, want in cases:
        for ref in (R.amax_ref, R.amax_ref_fast):
            got = ref(np.array(x, np.float64))
            assert got == want and math.copysign(1.0, got[0]) == 1.0, (x, got)
    rng = np.random.default_rng(5)
    x = rng.integers(-4, 5, 500).astype(np.float32)  # many ties
    x[rng.integers(0, 500, 40)] = np.nan
    assert R.amax_ref(x) == R.amax_ref_fast(x)


def diagonal_cases(T):
    """(rows, Ap, Aj, Ax): the hand-made matrix of the GPU test and random ones, rows > columns and rows < columns."""
    out = [R.hand_made_matrix(T)]
    rng = np.random.default_rng(9)
    for rows, cols in ((7, 3), (3, 7), (40, 40)):
        lens = rng.integers(0, 6, rows)
        Ap = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        Aj = rng.integers(0, cols, int(Ap[-1])).astype(np.int32)  # unsorted, with repeats
        out.append((rows, Ap, Aj, rng.standard_normal(int(Ap[-1])).astype(T)))
    return out


@pytest.mark.parametrize("T", TYPES, ids=["f32", "f64"])
def test_csr_diagonal_references(T):
    rows, Ap, Aj, Ax = R.hand_made_matrix(T)
    d = R.csr_diagonal_ref(T, rows, Ap, Aj, Ax, 0)
    assert d.dtype == T and d.tolist() == [T(0.1), T(0.3), 0.0, T(T(1e8) + T(0.7)), 0.0, 0.0]
    r = R.csr_diagonal_ref(T, rows, Ap, Aj, Ax, 1)
    assert r[2] == np.inf and r[4] == np.inf and r[0] == T(1) / T(0.1)
    # fewer rows than columns: the first 3 rows of the same arrays
    assert R.csr_diagonal_ref(T, 3, Ap[:4], Aj, Ax, 0).tolist() == d[:3].tolist()
    for rows, Ap, Aj, Ax in diagonal_cases(T):
        for rec in (0, 1):
            assert np.array_equal(R.csr_diagonal_ref(T, rows, Ap, Aj, Ax, rec), R.csr_diagonal_ref_fast(T, rows, Ap, Aj, Ax, rec))
