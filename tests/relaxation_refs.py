"""The two fused write-backs of spmv_csr_epilogue.hip and the whole cusp::relaxation::jacobi / polynomial calls, restated in
numpy with one rounding per operation in the matrix's own type T -- plus three deliberately wrong variants.

Plain module: no fixtures, no GPU.  tests/test_relaxation_refs.py proves these restatements against exact rational
arithmetic and against the literal answers of the reference's own tests, and that every mutant is caught;
tests/test_relaxation_gpu.py compares the kernels with them bit for bit.

    row sum       s_i = (((T(0) + Ax[j0] * x[Aj[j0]]) + Ax[j0 + 1] * x[Aj[j0 + 1]]) + ...)      storage order
    axpby form    out[i] = alpha * s_i + beta * z[i]
    Jacobi form   x_out[i] = x[i] + omega * (b[i] - s_i) / diag[i]        omega * (b - s) first, then the division
"""
from fractions import Fraction

import numpy as np

MUTANTS = ("divide_first", "fused_multiply_add", "sum_from_y")


def row_sums(Ap, Aj, Ax, x, start=None):
    """s_i for every row, in T.  start: None (the sums start at T(0)) or a vector the sums start from (the sum_from_y mutant)."""
    T = Ax.dtype.type
    rows = len(Ap) - 1
    s = np.empty(rows, Ax.dtype)
    with np.errstate(all="ignore"):
        prod = Ax * x[Aj]                       # one rounding per product
        for i in range(rows):
            acc = T(0) if start is None else start[i]
            for p in prod[int(Ap[i]):int(Ap[i + 1])]:
                acc = acc + p                   # numpy scalars of type T: one rounding per add
            s[i] = acc
    return s


def _round_to(dtype, q):
    """A rational rounded once to dtype (float() rounds a Fraction correctly to double; for float32 the second rounding can
    differ from a single one in rare ties -- this serves the fused mutant only, which has to differ, not to be exact)."""
    return np.dtype(dtype).type(float(q))


def epilogue_axpby(s, alpha, beta, z, mutant=None):
    """out = alpha * s + beta * z in T.  mutant fused_multiply_add: beta * z rounded, then alpha * s + that with ONE rounding
    (what a contracted multiply-add gives); finite inputs only."""
    T = s.dtype.type
    alpha, beta = T(alpha), T(beta)
    with np.errstate(all="ignore"):
        if mutant == "fused_multiply_add":
            t1 = beta * z
            return np.array([_round_to(s.dtype, Fraction(float(alpha)) * Fraction(float(si)) + Fraction(float(ti))) for si, ti in zip(s, t1)],
                            s.dtype)
        return alpha * s + beta * z


def epilogue_jacobi(s, x, b, diag, omega, mutant=None):
    """x_out = x + omega * (b - s) / diag in T.  mutant divide_first: x + omega * ((b - s) / diag)."""
    omega = s.dtype.type(omega)
    with np.errstate(all="ignore"):
        if mutant == "divide_first":
            return x + omega * ((b - s) / diag)
        return x + (omega * (b - s)) / diag


def spmv_axpby(Ap, Aj, Ax, x, alpha, beta, z, mutant=None):
    s = row_sums(Ap, Aj, Ax, x, start=z if mutant == "sum_from_y" else None)
    return epilogue_axpby(s, alpha, beta, z, mutant)


def jacobi_sweep(Ap, Aj, Ax, diag, b, x, omega, mutant=None):
    s = row_sums(Ap, Aj, Ax, x, start=x if mutant == "sum_from_y" else None)
    return epilogue_jacobi(s, x, b, diag, omega, mutant)


def extract_diagonal(Ap, Aj, Ax):
    """d[i] = the sum of row i's entries in column i, 0 where none is stored."""
    rows = len(Ap) - 1
    d = np.zeros(rows, Ax.dtype)
    for i in range(rows):
        for jj in range(int(Ap[i]), int(Ap[i + 1])):
            if Aj[jj] == i:
                d[i] = d[i] + Ax[jj]
    return d


class Jacobi:
    """cusp::relaxation::jacobi<T>: jacobi(A, omega = 1); relax(b, x) and relax(b, x, omega) return the new x."""

    def __init__(self, Ap, Aj, Ax, omega=1.0):
        self.A = (Ap, Aj, Ax)
        self.default_omega = Ax.dtype.type(omega)
        self.diagonal = extract_diagonal(Ap, Aj, Ax)

    def __call__(self, b, x, omega=None, mutant=None):
        return jacobi_sweep(*self.A, self.diagonal, b, x, self.default_omega if omega is None else omega, mutant)


def chebyshev_polynomial_coefficients(rho, lower_bound=1.0 / 30.0, upper_bound=1.1, dtype=np.float64):
    """The cubic whose roots are the three Chebyshev points of [lower_bound * rho, upper_bound * rho], normalised to constant
    term 1; coefficients from the highest power down (four of them)."""
    T = np.dtype(dtype).type
    lo, hi = T(lower_bound) * T(rho), T(upper_bound) * T(rho)
    roots = [lo + (hi - lo) * (T(np.cos(np.pi * (2 * k + 1) / 6)) + T(1)) / T(2) for k in range(3)]
    poly = np.poly(np.array(roots, dtype)).astype(dtype)
    return poly / poly[-1]


class Polynomial:
    """cusp::relaxation::polynomial<T>: polynomial(A, coefficients) keeps all but the last coefficient, negated;
    relax(b, x) uses those, relax(b, x, coefficients) uses the given ones as they are.  h persists between calls, as in
    the class (the first step reads it: 0 * h)."""

    def __init__(self, Ap, Aj, Ax, coefficients):
        T = Ax.dtype.type
        self.A = (Ap, Aj, Ax)
        self.default_coefficients = np.array([-T(c) for c in list(coefficients)[:-1]], Ax.dtype)
        self.h = np.zeros(len(Ap) - 1, Ax.dtype)

    def __call__(self, b, x, coefficients=None):
        Ap, Aj, Ax = self.A
        T = Ax.dtype.type
        coef = self.default_coefficients if coefficients is None else np.asarray(coefficients, Ax.dtype)
        with np.errstate(all="ignore"):
            if not np.any(x * x):                 # nrm2(x) == 0: a sum of squares is zero only if every square is
                residual = b.copy()
            else:
                residual = spmv_axpby(Ap, Aj, Ax, x, -1.0, 1.0, b)         # 1 * b + (-1) * (A x)
            self.h = coef[0] * residual + T(0) * self.h
            for c in coef[1:]:
                self.h = spmv_axpby(Ap, Aj, Ax, self.h, 1.0, c, residual)  # 1 * (A h) + c * residual
            return T(1) * self.h + x


# ------------------------------------------------------------------------------------------------
# exact arithmetic (the check of the restatements above; small-integer data, so nothing rounds)
# ------------------------------------------------------------------------------------------------
def exact_row_sums(Ap, Aj, Ax, x):
    return [sum((Fraction(float(Ax[jj])) * Fraction(float(x[Aj[jj]])) for jj in range(int(Ap[i]), int(Ap[i + 1]))), Fraction(0))
            for i in range(len(Ap) - 1)]


def exact_axpby(Ap, Aj, Ax, x, alpha, beta, z):
    return [Fraction(alpha) * s + Fraction(beta) * Fraction(float(zi)) for s, zi in zip(exact_row_sums(Ap, Aj, Ax, x), z)]


def exact_jacobi(Ap, Aj, Ax, diag, b, x, omega):
    return [Fraction(float(xi)) + Fraction(omega) * (Fraction(float(bi)) - s) / Fraction(float(di))
            for s, xi, bi, di in zip(exact_row_sums(Ap, Aj, Ax, x), x, b, diag)]
