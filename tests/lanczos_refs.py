"""numpy restatements for cusp::eigen::lanczos, cusp::blas::gemm / cmi_dense_gemm_* and cusp/detail/tridiagonal_eigen.h, checked on the CPU by
tests/test_lanczos_refs.py and used as the reference of the host and device tests.

gemm_ref            C(i, c) = the chain s = +0; s = s + A(i, j) B(j, c), j ascending, one rounded multiply and one rounded add per term, in T.
tridiagonal_eigen   the implicit QL sweeps of the header, step for step, in double.
lanczos             the loop of cusp/eigen/lanczos.h's plain path in T (dot products and norms through numpy, so the last bits of a sum may
                    differ from the host loops': the tests compare iteration counts within a margin and values within bars, not bits).
                    `window`: 0 reorthogonalises against every stored vector (the header); 10 is the reference's window of ten, kept as a mutant.
"""
import math
from fractions import Fraction

import numpy as np

from eigen_refs import random_fill
from multishift_refs import dense, poisson5pt

SA, LA, BE = "SA", "LA", "BE"


# ---- gemm ---------------------------------------------------------------------------------------------------------------------------------
def gemm_ref(A, B, mutant=None):
    """A (m x k), B (k x n) 2-D arrays of one float type -> C (m x n).  Mutants: 'descending' (j from k - 1 down), 'fma' (each term fused:
    the product is not rounded), 'first_product' (the chain starts from the first product instead of +0)."""
    T = A.dtype.type
    m, k = A.shape
    n = B.shape[1]
    C = np.zeros((m, n), T)
    order = range(k - 1, -1, -1) if mutant == "descending" else range(k)
    with np.errstate(all="ignore"):
        for c in range(n):
            s = np.zeros(m, T)
            first = True
            for j in order:
                if mutant == "fma":   # the product is not rounded: exact rational arithmetic, rounded once (tiny decks only)
                    s = np.array([T(float(Fraction(float(s[i])) + Fraction(float(A[i, j])) * Fraction(float(B[j, c])))) for i in range(m)], T)
                elif mutant == "first_product" and first:
                    s = (A[:, j] * B[j, c]).astype(T)
                else:
                    s = (s + (A[:, j] * B[j, c]).astype(T)).astype(T)
                first = False
            C[:, c] = s
    return C


# ---- the tridiagonal solver -----------------------------------------------------------------------------------------------------------------
def tridiagonal_eigen(diagonal, off_diagonal, vectors=True, sweeps_allowed=60):
    """(ok, w ascending, Z or None): cusp::detail::tridiagonal_eigen, step for step."""
    d = [float(x) for x in diagonal]
    n = len(d)
    e = [float(x) for x in off_diagonal[:max(n - 1, 0)]] + [0.0]
    Z = np.eye(n) if vectors else None
    for l in range(n):
        sweeps = 0
        while True:
            m = l
            while m + 1 < n:
                dd = abs(d[m]) + abs(d[m + 1])
                if abs(e[m]) + dd == dd:
                    break
                m += 1
            if m == l:
                break
            if sweeps == sweeps_allowed:
                return False, None, None
            sweeps += 1
            g = (d[l + 1] - d[l]) / (2.0 * e[l])
            r = math.hypot(g, 1.0)
            g = d[m] - d[l] + e[l] / (g + math.copysign(r, g))
            s = c = 1.0
            p = 0.0
            underflow = False
            for i in range(m - 1, l - 1, -1):
                f = s * e[i]
                b = c * e[i]
                r = math.hypot(f, g)
                e[i + 1] = r
                if r == 0.0:
                    d[i + 1] -= p
                    e[m] = 0.0
                    underflow = True
                    break
                s = f / r
                c = g / r
                g = d[i + 1] - p
                r = (d[i] - g) * s + 2.0 * c * b
                p = s * r
                d[i + 1] = g + p
                g = c * r - b
                if vectors:
                    zi, zj = Z[:, i].copy(), Z[:, i + 1].copy()
                    Z[:, i + 1] = s * zi + c * zj
                    Z[:, i] = c * zi - s * zj
            if underflow:
                continue
            d[l] -= p
            e[l] = g
            e[m] = 0.0
    w = np.array(d)
    if not np.all(np.isfinite(w)):
        return False, None, None
    order = np.argsort(w, kind="stable")
    return True, w[order], (Z[:, order] if vectors else None)


# ---- the Lanczos loop -----------------------------------------------------------------------------------------------------------------------
class Options:
    """cusp::eigen::lanczos_options<T>: the reference's fields and defaults."""

    def __init__(self, **kw):
        self.computeEigVecs = False
        self.minIter = self.maxIter = 0
        self.extraIter = self.stride = 10
        self.reorth = "None"
        self.eigPart = LA
        self.memoryExpansionFactor = 1.2
        self.tol = 1e-4
        self.doubleReorthGamma = 1.0 / math.sqrt(2.0)
        self.defaultMinIterFactor, self.defaultMaxIterFactor = 5, 50
        self.eigLowCut, self.eigHighCut = math.inf, -math.inf
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


class Result:
    pass


def lanczos(apply, N, T, wanted, options, window=0, start=None):
    """cusp::eigen::lanczos(A, eigVals(wanted), eigVecs, options) in T; apply(v) = A v.  Returns a Result with values, vectors (N x found or
    None), iterations, converged, alphas, betas, restarts."""
    o = options
    full = o.reorth == "Full"
    wanted = min(wanted, N)
    ends = (wanted + 1) // 2 if o.eigPart == BE else wanted
    min_iter, max_iter = o.minIter, o.maxIter
    if min_iter == 0:
        min_iter = o.defaultMinIterFactor * ends
        if max_iter:
            min_iter = min(max_iter, min_iter)
    if max_iter == 0:
        max_iter = 500 + o.defaultMaxIterFactor * ends
    if full:
        min_iter, max_iter = min(min_iter, N), min(max_iter, N)
    max_iter = max(max_iter, min_iter)
    stride = o.stride or 10
    tol = T(o.tol if o.tol >= 0 else math.sqrt(np.finfo(T).eps))
    out = Result()
    out.values, out.vectors, out.iterations, out.converged, out.restarts = np.zeros(0, T), None, 0, False, 0
    out.alphas = out.betas = ()
    if N == 0 or wanted == 0 or max_iter == 0:
        return out
    low = wanted if o.eigPart == SA else (wanted // 2 if o.eigPart == BE else 0)
    high = wanted - low
    keep = full or o.computeEigVecs
    eps = np.finfo(T).eps
    gamma = T(o.doubleReorthGamma)
    v0 = np.zeros(N, T)
    v1 = random_fill(N, 0, T) if start is None else start.astype(T)
    v1 = (v1 * (T(1) / T(np.sqrt(np.dot(v1, v1))))).astype(T)
    V, alphas, betas = [], [], []
    bb_prev, beta_sum = T(0), T(0)
    low_found = high_found = low_conv = high_conv = 0
    check_from = min_iter
    it = 0

    def against(q, v):
        return (v - (np.dot(q, v) * q).astype(T)).astype(T)

    def gram_schmidt(v, columns):
        for i in range(max(columns - window, 0) if window else 0, columns):
            v = against(V[i], v)
        return v

    def norm(v):
        return T(np.sqrt(np.dot(v, v)))

    def ritz(n):
        ok, w, _ = tridiagonal_eigen(alphas[:n], betas[:max(n - 1, 0)], vectors=False)
        assert ok
        return w

    with np.errstate(all="ignore"):
        while True:
            if keep:
                V.append(v1)
            v2 = apply(v1).astype(T)
            if it > 0:
                v2 = (v2 - (bb_prev * v0).astype(T)).astype(T)
            aa = T(np.dot(v1, v2))
            v2 = (v2 - (aa * v1).astype(T)).astype(T)
            bb = norm(v2)
            alphas.append(float(aa))
            if it + 1 == max_iter:
                betas.append(float(bb))
                it += 1
                break
            if (full or it + 1 < N) and it + 1 >= check_from and (it + 1 - check_from) % stride == 0 and low <= it and high <= it:
                r0, r1 = ritz(it), ritz(it + 1)
                i, left = 0, low
                s = s0 = a0 = T(0)
                while left and r1[i] <= o.eigLowCut:
                    a0, s0, s = T(a0 + T(abs(r0[i]))), T(s0 + T(r0[i])), T(s + T(r1[i]))
                    left -= 1
                    i += 1
                low_found = low - left
                low_err = T(0) if (a0 == 0 and s == 0) else abs((s - s0) / a0)
                i, left = it, high
                s = s0 = a0 = T(0)
                while left and r1[i] >= o.eigHighCut:
                    a0, s0, s = T(a0 + T(abs(r0[i - 1]))), T(s0 + T(r0[i - 1])), T(s + T(r1[i]))
                    left -= 1
                    i -= 1
                high_found = high - left
                high_err = T(0) if (a0 == 0 and s == 0) else abs((s - s0) / a0)
                if low_err <= tol and high_err <= tol:
                    if o.extraIter == 0:
                        low_conv, high_conv = low_found, high_found
                    if low_conv < low_found or high_conv < high_found:
                        low_conv, high_conv = low_found, high_found
                        check_from = min(it + o.extraIter + 1, max_iter)
                    else:
                        out.converged = True
                        betas.append(float(bb))
                        it += 1
                        break
            betas.append(float(bb))
            beta_sum = T(beta_sum + bb)
            if full:
                v2 = gram_schmidt(v2, it + 1)
                bb_old, bb = bb, norm(v2)
                if gamma >= 1 or bb < gamma * bb_old:
                    v2 = gram_schmidt(v2, it + 1)
                    bb = norm(v2)
                betas[it] = float(bb)
            if bb < beta_sum * eps or bb == 0:
                out.restarts += 1
                v2 = random_fill(N, out.restarts, T)
                if keep:
                    v2 = gram_schmidt(v2, it + 1)
                else:
                    if it > 0:
                        v2 = against(v0, v2)
                    v2 = against(v1, v2)
                bb = norm(v2)
                betas[it] = 0.0
                if bb == 0:   # nothing is left outside the span of the vectors kept: the loop ends with this step
                    it += 1
                    break
            v2 = (v2 * (T(1) / T(bb))).astype(T)
            v0, v1, bb_prev = v1, v2, bb
            it += 1
    m = it
    ok, w, S = tridiagonal_eigen(alphas[:m], betas[:m - 1], vectors=o.computeEigVecs)
    assert ok
    if not out.converged:
        low_found = 0
        while low_found < low and low_found < m and w[low_found] <= o.eigLowCut:
            low_found += 1
        high_found = 0
        while high_found < high and low_found + high_found < m and w[m - 1 - high_found] >= o.eigHighCut:
            high_found += 1
    chosen = list(range(low_found)) + list(range(m - high_found, m))
    out.values = w[chosen].astype(T)
    out.iterations, out.alphas, out.betas = m, np.array(alphas), np.array(betas)
    if o.computeEigVecs and chosen:
        out.vectors = gemm_ref(np.stack(V[:m], 1), S[:, chosen].astype(T))
    return out


# ---- the cases of the host and device programs -------------------------------------------------------------------------------------------------
TYPES = {"f64": np.float64, "f32": np.float32}
PARTS = ((LA, 1), (LA, 4), (SA, 4), (BE, 5))
#        grid,     type,  tol
TABLE = (((7, 5), "f64", 1e-10), ((7, 5), "f32", 1e-6), ((16, 12), "f64", 1e-10), ((16, 12), "f32", 1e-6), ((33, 31), "f64", 1e-10))
# (nx, ny, type, part, count, reorth, tol): every grid and type of TABLE with every (part, count), Full with eigenvectors; then 16 x 12 without
# reorthogonalisation, (LA, 1), at the table's tolerances (55 steps in double)
CASES = tuple((nx, ny, t, part, count, "Full", tol) for (nx, ny), t, tol in TABLE for part, count in PARTS) + \
    ((16, 12, "f64", LA, 1, "None", 1e-10), (16, 12, "f32", LA, 1, "None", 1e-6))

_dense = {}
_runs = {}


def matrix(nx, ny):
    if (nx, ny) not in _dense:
        _dense[nx, ny] = dense(poisson5pt(nx, ny, np.float64))
    return _dense[nx, ny]


def case_options(case):
    nx, ny, t, part, count, reorth, tol = case
    return Options(computeEigVecs=True, reorth=reorth, eigPart=part, tol=tol)


def run_case(case, window=0):
    """The restated loop on one case, computed once per (case, window)."""
    if (case, window) not in _runs:
        nx, ny, t, part, count, reorth, tol = case
        T = TYPES[t]
        A = matrix(nx, ny).astype(T)
        _runs[case, window] = lanczos(lambda v: A @ v, nx * ny, T, count, case_options(case), window=window)
    return _runs[case, window]


def wanted_extremes(nx, ny, part, count):
    """The wanted ends of the DISTINCT spectrum (non-square grids: every extreme eigenvalue is simple), low end ascending then high end."""
    w = np.linalg.eigvalsh(matrix(nx, ny))
    low = count if part == SA else (count // 2 if part == BE else 0)
    high = count - low
    return np.r_[w[:low], w[len(w) - high:]]


def check_pairs(case, values, vectors, iterations, converged, what=""):
    """Bars (i)-(v) of the solver cases on returned pairs (values: found, vectors: N x found, both as float64 of the returned T values)."""
    nx, ny, t, part, count, reorth, tol = case
    T = TYPES[t]
    A = matrix(nx, ny)
    exact = np.linalg.eigvalsh(A)
    lam_max = exact[-1]
    assert lam_max < 8
    want = wanted_extremes(nx, ny, part, count)
    ref = run_case(case)
    eps = float(np.finfo(T).eps)
    assert len(values) == len(want) and vectors.shape == (nx * ny, len(want)), (what, len(values), vectors.shape)             # (v)
    low = count if part == SA else (count // 2 if part == BE else 0)
    assert np.all(np.diff(values[:low]) > 0) and np.all(np.diff(values[low:]) > 0), (what, values)                           # (v)
    figures = {}
    for j, lam in enumerate(values):                                                                                            # (i)
        e = vectors[:, j]
        res = np.linalg.norm(A @ e - lam * e) / np.linalg.norm(e)
        gap = np.min(np.abs(exact - lam))
        figures.setdefault("excess_eps", []).append(max(gap - res, 0.0) / (eps * lam_max))
        assert gap <= res + 64 * eps * lam_max, (what, j, lam, gap, res)
    ref_error = float(np.max(np.abs(ref.values.astype(np.float64) - want)))
    tol_case = tolerance(case)
    figures["value_error"] = float(np.max(np.abs(values - want)))
    if tol_case is not None:                                                                                                    # (ii)
        assert figures["value_error"] <= tol_case, (what, values, want, tol_case, ref_error)
    if reorth == "Full":                                                                                                        # (iii)
        figures["orthogonality_over_m_eps"] = float(np.max(np.abs(vectors.T @ vectors - np.eye(len(values))))) / (iterations * eps)
        assert figures["orthogonality_over_m_eps"] <= 1.0, (what, figures)
    assert converged == ref.converged, (what, converged, ref.converged)                                                       # (iv)
    max_iter = min(500 + 50 * ((count + 1) // 2 if part == BE else count), nx * ny if reorth == "Full" else 10 ** 9)
    assert iterations <= 1.5 * ref.iterations and iterations <= max_iter, (what, iterations, ref.iterations)
    print(what, case, "iterations", iterations, "restatement", ref.iterations, figures)
    return figures


# (ii): ten times the restatement's own error with the library's start vector, and no looser than the issue's figures (1e-9 double, 1e-5 float)
RESTATEMENT_ERRORS = {}


def tolerance(case):
    """None where nothing is asserted on the values beside (i): 7 x 5 (the run is taken to m = N: the values are then exact to rounding, and
    held by (i)) has the bars of 16 x 12."""
    nx, ny, t, part, count, reorth, tol = case
    cap = 1e-9 if t == "f64" else 1e-5
    ref = run_case(case)
    if not ref.converged and reorth == "None":
        return None
    err = float(np.max(np.abs(ref.values.astype(np.float64) - wanted_extremes(nx, ny, part, count))))
    floor = 64 * float(np.finfo(TYPES[t]).eps) * 8   # the rounding term of (i): a bar below it would ask more than the arithmetic can give
    return min(cap, max(10 * err, floor))
