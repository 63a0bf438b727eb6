"""References for cusp::eigen::lobpcg (test infrastructure shared by test_lobpcg_refs.py, test_lobpcg_host.py and test_lobpcg_gpu.py).

1. The three kernels of csrc/lobpcg.hip in the form of blas_extra_refs.py: `restate(T, s, v)` is numpy in T, operation by operation (the
   library is built with -ffp-contract=off: compared BIT FOR BIT); `formula(s, v)` is the mathematics over any arithmetic and returns, per
   output, (value, sum of |terms|); a result in T lies within k * u * sum|terms| of it, k = KERNELS[name].k[output] the roundings on the
   longest path to the output (a scalar rounded to T, a multiply, an add, a root count one each) plus one for the second-order terms of a
   chain that long.  `sums(T, got, v)` names the two factor arrays of every reduction, taken from the vectors the kernel RETURNED.
   Scalars: `lambda` and `pp` are device doubles; cx, cr, cp, lambda_new are passed by value and must be values of T.
   `mutant` names one deliberate mistake (MUTANTS); test_lobpcg_refs.py shows that each is caught.
2. `sygv_small`: cusp/detail/sygv_small.h restated step by step in float64.
3. `lobpcg`: the whole loop as the header layer runs it on host_memory.  Dots are SEQUENTIAL left-to-right sums in T from T(0), as the host
   cusp::blas::dot forms them (multishift_refs.dot: a cumulative sum cannot be reordered); nrm2 is the root of that sum; the multiply is the
   host CSR loop.  Every normalisation multiplies by T(1) / T(norm)."""
import math
from fractions import Fraction

import numpy as np

import multishift_refs as MS
from blas_extra_refs import HIGHER, U, Kernel, exact_sum, higher, rational  # noqa: F401  (re-exported for the tests)
from eigen_refs import random_fill
from multishift_refs import dense, dot, nrm2, poisson5pt, spmv  # noqa: F401

MUTANTS = ("fma", "unscaled_p_in_sums", "old_p_in_x", "first_ignored")


def _fma(a, x, y, T):
    """a x + y with ONE rounding to T (the product kept in the precision above T)."""
    H = HIGHER[T]
    return (H(a) * x.astype(H) + y.astype(H)).astype(T)


def _sqrt(v):
    if isinstance(v, Fraction):  # exact: the tests hand over squares of rationals
        n, d = math.isqrt(v.numerator), math.isqrt(v.denominator)
        assert n * n == v.numerator and d * d == v.denominator
        return Fraction(n, d)
    return np.sqrt(v)


# ---- residual: r <- T(-lambda) x + ax --------------------------------------------------------------------------------------------------
def _r_residual(T, s, v, mutant=None):
    neg = -T(np.float64(s["lambda"]))
    if mutant == "fma":
        return {"r": _fma(neg, v["x"], v["ax"], T)}
    return {"r": neg * v["x"] + v["ax"]}


def _f_residual(s, v):
    t = s["lambda"] * v["x"]
    return {"r": (v["ax"] - t, abs(v["ax"]) + abs(t))}


def _s_residual(T, got, v):
    return {"rr": (got["r"], got["r"])}


# ---- gram: p, ap <- s p, s ap with s = T(1) / T(sqrt(pp)); eight sums (three without p) -------------------------------------------------
GRAM_SUMS = ("xaw", "waw", "xw", "xap", "wap", "pap", "xp", "wp")


def _r_gram(T, s, v, mutant=None):
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = T(1) / T(np.sqrt(np.float64(s["pp"])))
        return {"p": scale * v["p"], "ap": scale * v["ap"]}


def _f_gram(s, v):
    scale = 1 / _sqrt(s["pp"])
    p, ap = scale * v["p"], scale * v["ap"]
    return {"p": (p, abs(p)), "ap": (ap, abs(ap))}


def _s_gram(T, got, v, mutant=None):
    p, ap = (v["p"], v["ap"]) if mutant == "unscaled_p_in_sums" else (got["p"], got["ap"])
    x, w, aw = v["x"], v["w"], v["aw"]
    return {"xaw": (x, aw), "waw": (w, aw), "xw": (x, w), "xap": (x, ap), "wap": (w, ap), "pap": (p, ap), "xp": (x, p), "wp": (w, p)}


def _r_gram_first(T, s, v, mutant=None):
    return {}


def _f_gram_first(s, v):
    return {}


def _s_gram_first(T, got, v, mutant=None):
    x, w, aw = v["x"], v["w"], v["aw"]
    return {"xaw": (x, aw), "waw": (w, aw), "xw": (x, w)}


# ---- update ------------------------------------------------------------------------------------------------------------------------------
def _update_restate(first, with_r):
    def restate(T, s, v, mutant=None):
        cx, cr, cp, neg = T(s["cx"]), T(s["cr"]), T(s["cp"]), -T(s["lambda_new"])
        assert float(cx) == s["cx"] and float(cr) == s["cr"] and float(cp) == s["cp"] and float(neg) == -s["lambda_new"], "by-value scalars are values of T"
        one = T(1)
        as_first = first and mutant != "first_ignored"
        if mutant == "fma":
            p = _fma(cr, v["w"], v["p"] if as_first else cp * v["p"], T)
            ap = _fma(cr, v["aw"], v["ap"] if as_first else cp * v["ap"], T)
        elif as_first:
            p, ap = cr * v["w"] + v["p"], cr * v["aw"] + v["ap"]
        else:
            p, ap = cr * v["w"] + cp * v["p"], cr * v["aw"] + cp * v["ap"]
        px, apx = (v["p"], v["ap"]) if mutant == "old_p_in_x" else (p, ap)
        x, ax = cx * v["x"] + one * px, cx * v["ax"] + one * apx
        out = {"p": p, "ap": ap, "x": x, "ax": ax}
        if with_r:
            out["r"] = _fma(neg, x, ax, T) if mutant == "fma" else neg * x + ax
        return out
    return restate


def _update_formula(first, with_r):
    def formula(s, v):
        cp = 1 if first else s["cp"]
        t = {k: (s["cr"] * v[a], cp * v[b]) for k, a, b in (("p", "w", "p"), ("ap", "aw", "ap"))}
        out = {k: (t[k][0] + t[k][1], abs(t[k][0]) + abs(t[k][1])) for k in t}
        for k, src in (("x", "p"), ("ax", "ap")):
            tx = s["cx"] * v[k]
            out[k] = (tx + out[src][0], abs(tx) + out[src][1])
        if with_r:
            out["r"] = (out["ax"][0] - s["lambda_new"] * out["x"][0], out["ax"][1] + abs(s["lambda_new"]) * out["x"][1])
        return out
    return formula


def _s_update(with_r):
    def sums(T, got, v):
        out = {"pp": (got["p"], got["p"])}
        if with_r:
            out["rr"] = (got["r"], got["r"])
        return out
    return sums


_UV = ("w", "aw", "p", "ap", "x", "ax", "r")
_US = ("cx", "cr", "cp", "lambda_new")
# k: p, ap: multiply, multiply, add = 3 (+1); x, ax: p's 3, cx x, T(1) p, add = 6 (+1); r: x's 6, lambda x, add = 8 (+1)
_UK = {"p": 4, "ap": 4, "x": 7, "ax": 7, "r": 9}
KERNELS = {k.name: k for k in (
    Kernel("residual", ("lambda",), ("x", "ax", "r"), ("r",), {"r": 4}, _r_residual, _f_residual, _s_residual),      # lambda -> T, multiply, add (+1)
    Kernel("gram", ("pp",), ("x", "w", "aw", "p", "ap"), ("p", "ap"), {"p": 5, "ap": 5}, _r_gram, _f_gram, _s_gram),  # root, -> T, reciprocal, multiply (+1)
    Kernel("gram_first", (), ("x", "w", "aw"), (), {}, _r_gram_first, _f_gram_first, _s_gram_first),
    Kernel("update", _US, _UV, ("p", "ap", "x", "ax", "r"), _UK, _update_restate(False, True), _update_formula(False, True), _s_update(True), by_value=True),
    Kernel("update_first", _US, _UV, ("p", "ap", "x", "ax", "r"), _UK, _update_restate(True, True), _update_formula(True, True), _s_update(True), by_value=True),
    Kernel("update_no_r", _US, _UV[:6], ("p", "ap", "x", "ax"), _UK, _update_restate(False, False), _update_formula(False, False), _s_update(False), by_value=True),
)}

# pp: squares of rationals, so that the exact formula has a rational root: 6.25 -> s = 0.4 (rounded), 4 -> s = 0.5 (exact)
SCALARS = {
    "inexact": {"lambda": 1.75 / 0.6, "pp": 6.25, "cx": 0.9 / 1.7, "cr": -1.1 / 0.3, "cp": 0.7 / 1.3, "lambda_new": 2.9 / 1.1},
    "exact": {"lambda": -1.5, "pp": 4.0, "cx": 0.5, "cr": -2.0, "cp": 0.25, "lambda_new": 3.0},
}


def scalars_for(kernel, kind, T):
    """The scalars of one kernel; the by-value ones are made values of T: the caller hands them over exactly."""
    return {n: (float(T(SCALARS[kind][n])) if kernel.by_value else SCALARS[kind][n]) for n in kernel.scalars}


# ---- cusp/detail/sygv_small.h ----------------------------------------------------------------------------------------------------------------
def sygv_small(n, A, B):
    """(ok, w, Z): Cholesky of B, C = L^-1 A L^-T, cyclic Jacobi, ascending order, Z = L^-T V -- the header's steps in the header's order."""
    f = np.float64
    A, B = np.asarray(A, f).reshape(n, n), np.asarray(B, f).reshape(n, n)
    L, C, V, Y = (np.zeros((3, 3), f) for _ in range(4))
    with np.errstate(all="ignore"):
        for j in range(n):
            d = B[j, j]
            for k in range(j):
                d = d - L[j, k] * L[j, k]
            if not (d > 0.0) or not np.isfinite(d):
                return False, None, None
            L[j, j] = np.sqrt(d)
            for i in range(j + 1, n):
                s = B[i, j]
                for k in range(j):
                    s = s - L[i, k] * L[j, k]
                L[i, j] = s / L[j, j]
        for c in range(n):
            for i in range(n):
                s = A[i, c] if i >= c else A[c, i]
                for k in range(i):
                    s = s - L[i, k] * Y[k, c]
                Y[i, c] = s / L[i, i]
        for r in range(n):
            for i in range(n):
                s = Y[r, i]
                for k in range(i):
                    s = s - L[i, k] * C[r, k]
                C[r, i] = s / L[i, i]
        for i in range(n):
            for j in range(i):
                C[i, j] = C[j, i] = f(0.5) * (C[i, j] + C[j, i])
        for i in range(n):
            V[i, i] = 1.0
        for _ in range(60):
            rotated = False
            for p in range(n - 1):
                for q in range(p + 1, n):
                    apq = C[p, q]
                    if not (abs(apq) > f(1e-18) * (abs(C[p, p]) + abs(C[q, q]))):
                        continue
                    rotated = True
                    tau = (C[q, q] - C[p, p]) / (f(2.0) * apq)
                    t = f(1.0) / (tau + np.sqrt(f(1.0) + tau * tau)) if tau >= 0.0 else f(-1.0) / (-tau + np.sqrt(f(1.0) + tau * tau))
                    c = f(1.0) / np.sqrt(f(1.0) + t * t)
                    s = t * c
                    for k in range(n):
                        ckp, ckq = C[k, p], C[k, q]
                        C[k, p], C[k, q] = c * ckp - s * ckq, s * ckp + c * ckq
                        vkp, vkq = V[k, p], V[k, q]
                        V[k, p], V[k, q] = c * vkp - s * vkq, s * vkp + c * vkq
                    for k in range(n):
                        cpk, cqk = C[p, k], C[q, k]
                        C[p, k], C[q, k] = c * cpk - s * cqk, s * cpk + c * cqk
                    C[p, q] = C[q, p] = 0.0
            if not rotated:
                break
        order = list(range(n))
        for i in range(1, n):
            j = i
            while j > 0 and C[order[j], order[j]] < C[order[j - 1], order[j - 1]]:
                order[j], order[j - 1] = order[j - 1], order[j]
                j -= 1
        w, Z = np.zeros(n, f), np.zeros((n, n), f)
        for j in range(n):
            src = order[j]
            w[j] = C[src, src]
            for i in range(n - 1, -1, -1):
                s = V[i, src]
                for k in range(i + 1, n):
                    s = s - L[k, i] * Z[k, j]
                Z[i, j] = s / L[i, i]
    return True, w, Z


def gram_pair(lam, g, n):
    f = float
    if n == 3:
        return ([[f(lam), f(g[0]), f(g[3])], [f(g[0]), f(g[1]), f(g[4])], [f(g[3]), f(g[4]), f(g[5])]],
                [[1.0, f(g[2]), f(g[6])], [f(g[2]), 1.0, f(g[7])], [f(g[6]), f(g[7]), 1.0]])
    return [[f(lam), f(g[0])], [f(g[0]), f(g[1])]], [[1.0, f(g[2])], [f(g[2]), 1.0]]


def ritz_step(T, lam, g, with_p, largest, solver=sygv_small):
    """detail::lobpcg_detail::ritz_step: (ok, used_p, lambda, cx, cr, cp); the 2 x 2 pair when the 3 x 3 gramB is not positive definite."""
    for n in ((3, 2) if with_p else (2,)):
        ok, w, Z = solver(n, *gram_pair(lam, g, n))
        if not ok:
            continue
        col = n - 1 if largest else 0
        return True, n == 3, T(w[col]), T(Z[0, col]), T(Z[1, col]), T(Z[2, col]) if n == 3 else T(0)
    return False, False, T(0), T(0), T(0), T(0)


# ---- the whole loop (host_memory) ---------------------------------------------------------------------------------------------------------------
class Result:
    def __init__(self):
        self.residuals, self.iteration_count, self.converged, self.retries = [], 0, False, 0


def lobpcg(A, x0, tolerance, iteration_limit, largest, dinv=None, solver=sygv_small):
    """cusp::eigen::lobpcg on host_memory with monitor(ones, iteration_limit, tolerance): returns (lambda, X, Result).  dinv: the reciprocal
    diagonal of cusp::precond::diagonal (None: the identity)."""
    T = x0.dtype.type
    N = A[0]
    one = T(1)
    tol = T(tolerance)
    b_norm = nrm2(np.ones(N, T))
    X = (one / T(nrm2(x0))) * x0
    AX = spmv(A, X)
    lam = dot(X, AX)
    P, AP = np.zeros(N, T), np.zeros(N, T)
    res = Result()
    r_norm = np.finfo(T).max
    while res.iteration_count < min(N, iteration_limit):
        first = res.iteration_count == 0
        R = (-lam) * X + one * AX
        r_norm = nrm2(R)
        res.residuals.append(r_norm)
        if r_norm < tol:
            break
        W = R.copy() if dinv is None else dinv * R
        W = (one / T(nrm2(W))) * W
        AW = spmv(A, W)
        if not first:
            s = one / T(nrm2(P))
            P, AP = s * P, s * AP
        g = [dot(X, AW), dot(W, AW), dot(X, W)] + ([T(0)] * 5 if first else [dot(X, AP), dot(W, AP), dot(P, AP), dot(X, P), dot(W, P)])
        ok, used_p, lam_new, cx, cr, cp = ritz_step(T, lam, g, not first, largest, solver)
        if not ok:
            break
        res.retries += int(not first and not used_p)
        lam = lam_new
        if first:
            P, AP = cr * W + P, cr * AW + AP
        else:
            P, AP = cr * W + cp * P, cr * AW + cp * AP
        X, AX = cx * X + one * P, cx * AX + one * AP
        res.iteration_count += 1
    res.converged = bool(r_norm <= T(T(0) + tol * b_norm))
    return lam, X, res


def poisson_plus_diagonal(nx, ny, dtype):
    """A_1 = poisson5pt + diag(1 + i mod 7): a diagonal that is not constant, so that Jacobi preconditioning does something."""
    N, Ap, Aj, Ax = poisson5pt(nx, ny, dtype)
    Ax = Ax.copy()
    for i in range(N):
        for jj in range(Ap[i], Ap[i + 1]):
            if Aj[jj] == i:
                Ax[jj] = Ax[jj] + dtype(1 + i % 7)
    return N, Ap, Aj, Ax


def diagonal_inverse(A):
    N, Ap, Aj, Ax = A
    T = Ax.dtype.type
    d = np.zeros(N, T)
    for i in range(N):
        for jj in range(Ap[i], Ap[i + 1]):
            if Aj[jj] == i:
                d[i] = d[i] + Ax[jj]
    return (T(1) / d).astype(T)


def start_vector(N, T, seed=7):
    """cusp::random_array<T>(N, seed)."""
    return random_fill(N, seed, T)


# the solver cases of the host and device programs: (name, matrix, nx, ny, type, tolerance, preconditioner, largest)
CASES = (
    ("smallest", "poisson", 10, 10, "f64", 1e-8, "identity"), ("smallest", "poisson", 7, 5, "f64", 1e-8, "identity"),
    ("smallest", "poisson", 33, 31, "f64", 1e-8, "identity"), ("smallest", "poisson", 10, 10, "f32", 1e-3, "identity"),
    ("smallest", "poisson", 7, 5, "f32", 1e-3, "identity"), ("smallest", "poisson", 33, 31, "f32", 1e-3, "identity"),
    ("smallest", "a1", 10, 10, "f64", 1e-8, "diagonal"), ("smallest", "a1", 10, 10, "f64", 1e-8, "identity"),
    ("smallest", "a1", 10, 10, "f32", 1e-3, "diagonal"), ("largest", "poisson", 10, 10, "f64", 1e-8, "identity"),
    ("largest", "poisson", 33, 31, "f64", 1e-8, "identity"),
)
LIMIT = 500


def case_matrix(kind, nx, ny, T):
    return poisson5pt(nx, ny, T) if kind == "poisson" else poisson_plus_diagonal(nx, ny, T)


def exact_eigenvalue(kind, nx, ny, largest):
    w = np.linalg.eigvalsh(dense(case_matrix(kind, nx, ny, np.float64)))
    return float(w[-1] if largest else w[0])


def run_case(case, solver=sygv_small):
    which, kind, nx, ny, tname, tol, precond = case
    T = {"f32": np.float32, "f64": np.float64}[tname]
    A = case_matrix(kind, nx, ny, T)
    dinv = diagonal_inverse(A) if precond == "diagonal" else None
    return lobpcg(A, start_vector(A[0], T), tol, LIMIT, which == "largest", dinv, solver)
