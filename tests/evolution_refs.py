"""References for evolution strength of connection and cusp::gallery::diffusion, written from the contract of
include/cusp_mi355x.h and cusp/precond/aggregation/strength.h -- numpy in the value type T, one rounding per operation:

  transpose_positions   t(e) = the position of (col(e), row(e)); conforming = every row strictly ascending by column, every column inside
                        the matrix, every entry with a partner.
  masked_product        out[e] = sum of Vx[p] * Wx[q] over the columns that rows row(e) and col(e) have in common (p in row(e), q in
                        row col(e)), in ascending column order from +0, the product and the sum rounded separately in T.
  evolution_strength    the nineteen steps of strength.h.  Where the reference's C++ expression mixes a double literal with T the step is
                        evaluated in double and rounded once:  v = T((row == col) - (1.0 / double(T(rho))) * double(v))   (rho itself is
                        first rounded to T: the functor's member is a T),  a = T(|1.0 - double(a)|),  the 1e-4 constants are T(1e-4),
                        sqrt(eps_T) is the T square root,  s = T(0.5 * double(T(a + a_t))),  the filter compares s >= T(T(epsilon) * small)
                        (the product of two T in double is exact, so this is "in double, rounded once" for the epsilon that T holds).
  diffusion             the reference's nine stencil values in T from cos / sin of the double angle, entries equal to zero not stored.

Plain module: no fixtures, no GPU.  MUTANTS names one deliberately wrong variant per stated order or precision;
tests/test_evolution_refs.py proves that a deck catches each of them.
"""
from fractions import Fraction

import numpy as np

import amg_refs as AR

DTYPES = (np.float64, np.float32)
MUTANTS = ("fma_chain", "descending_merge", "tpos_identity", "half_dropped", "filter_greater", "min_with_zeros", "diagonal_not_reset", "b_zeros_kept",
           "rho_product_in_value_type")


def csr_rows(Ap):
    return AR.csr_rows(Ap).astype(np.int64)


def transpose_positions(n, Ap, Aj):
    """(tpos, conforming).  tpos is defined only when conforming."""
    Ap, Aj = np.asarray(Ap, np.int64), np.asarray(Aj, np.int64)
    tpos = np.zeros(len(Aj), np.int32)
    if len(Ap) != n + 1 or Ap[0] != 0 or Ap[n] != len(Aj) or np.any(np.diff(Ap) < 0):
        return tpos, False
    where = {}
    for i in range(n):
        prev = -1
        for e in range(Ap[i], Ap[i + 1]):
            j = int(Aj[e])
            if j <= prev or j >= n:
                return tpos, False
            prev = j
            where[(i, j)] = e
    for (i, j), e in where.items():
        if (j, i) not in where:
            return tpos, False
        tpos[e] = where[(j, i)]
    return tpos, True


def _matches(n, Ap, Aj, e, row):
    """The pairs (p, q) of step 5 for entry e, in ascending column order: one merge of rows row(e) and col(e)."""
    col = int(Aj[e])
    if col < 0 or col >= n:
        return []
    p, pe, q, qe = int(Ap[row]), int(Ap[row + 1]), int(Ap[col]), int(Ap[col + 1])
    out = []
    while p < pe and q < qe:
        if Aj[p] == Aj[q]:
            out.append((p, q))
            p += 1
            q += 1
        elif Aj[p] < Aj[q]:
            p += 1
        else:
            q += 1
    return out


def _round(fr, T):
    """The fraction rounded to T (through double for float32: the mutant that uses it needs no more)."""
    return T(float(fr))


def masked_product(n, Ap, Aj, Vx, Wx, mutant=None):
    T = Vx.dtype.type
    rows = csr_rows(Ap)
    out = np.zeros(len(Aj), Vx.dtype)
    with np.errstate(all="ignore"):
        for e in range(len(Aj)):
            pairs = _matches(n, Ap, Aj, e, int(rows[e]))
            if mutant == "descending_merge":
                pairs = pairs[::-1]
            s = T(0)
            for p, q in pairs:
                if mutant == "fma_chain":
                    s = _round(Fraction(float(Vx[p])) * Fraction(float(Wx[q])) + Fraction(float(s)), T)
                else:
                    s = T(s + T(Vx[p] * Wx[q]))
            out[e] = s
    return out


def exact_masked_product(n, Ap, Aj, Vx, Wx):
    """Per entry: (the exact sum, the exact sum of the terms' magnitudes, the number of terms) as Fractions (finite operands only)."""
    rows = csr_rows(Ap)
    out = []
    for e in range(len(Aj)):
        terms = [Fraction(float(Vx[p])) * Fraction(float(Wx[q])) for p, q in _matches(n, Ap, Aj, e, int(rows[e]))]
        out.append((sum(terms, Fraction(0)), sum((abs(t) for t in terms), Fraction(0)), len(terms)))
    return out


def unit_roundoff(dtype):
    return Fraction(1, 2 ** (53 if np.dtype(dtype) == np.float64 else 24))


def scaled_values(n, Ap, Aj, Ax, rho, mutant=None):
    """Steps 1, 2 and 4: v = (row == col) - (1.0 / rho) * (Ax / D[row])."""
    dtype = Ax.dtype
    T = dtype.type
    rows = csr_rows(Ap)
    with np.errstate(all="ignore"):
        D = AR.diagonal(n, Ap, Aj, Ax)
        v = (Ax / D[rows]).astype(dtype)
        eye = rows == Aj
        rho_t = T(rho)
        if mutant == "rho_product_in_value_type":
            return (eye.astype(dtype) - (T(T(1) / rho_t) * v).astype(dtype)).astype(dtype)
        inv = np.float64(1.0) / np.float64(rho_t)
        return (eye.astype(np.float64) - inv * v.astype(np.float64)).astype(dtype)


def row_minimum(n, Ap, s, mutant=None):
    """Step 16's chain per row: the reference's non_zero_minimum from the row's first entry on, left to right."""
    small = np.full(n, np.finfo(s.dtype).max, s.dtype)
    for i in range(n):
        lo, hi = int(Ap[i]), int(Ap[i + 1])
        if hi <= lo:
            continue
        acc = s[lo]
        for e in range(lo + 1, hi):
            rhs = s[e]
            if mutant == "min_with_zeros":
                acc = acc if acc < rhs else rhs
            elif acc == 0:
                acc = rhs
            elif rhs == 0:
                pass
            else:
                acc = acc if acc < rhs else rhs
        small[i] = acc
    return small


def evolution_strength(n, Ap, Aj, Ax, B, rho, epsilon=4.0, mutant=None, data=None):
    """The whole measure for a given non-zero rho on a conforming matrix.  Returns a dict: tpos, v, data, s (the final s[e] of
    every entry of A) and S = (Sp, Sj, Sx).  `data`: step 5's result supplied by the caller (the rest follows from it)."""
    dtype = Ax.dtype
    T = dtype.type
    Ap, Aj = np.asarray(Ap, np.int32), np.asarray(Aj, np.int32)
    tpos, ok = transpose_positions(n, Ap, Aj)
    assert ok, "evolution_strength: the pattern does not conform"
    if mutant == "tpos_identity":
        tpos = np.arange(len(Aj), dtype=np.int32)
    rows = csr_rows(Ap)
    v = scaled_values(n, Ap, Aj, Ax, rho, mutant)
    if data is None:
        data = masked_product(n, Ap, Aj, v, v[tpos], mutant)
    data = np.asarray(data, dtype)
    with np.errstate(all="ignore"):
        DAt = AR.diagonal(n, Ap, Aj, data)
        Bs = np.asarray(B, dtype).copy()
        if mutant != "b_zeros_kept":
            Bs[Bs == 0] = T(1)
        a = ((T(1) * DAt[rows]).astype(dtype) * Bs[Aj]).astype(dtype)
        neg = (data * a).astype(dtype) < 0
        a = (a / data).astype(dtype)
        weak = a < T(1e-4)
        a = np.abs(np.float64(1.0) - a.astype(np.float64)).astype(dtype)
        a[neg | weak] = T(0)
        a[(a < np.sqrt(T(np.finfo(dtype).eps))) & (a != 0)] = T(1e-4)
        both = (a + a[tpos]).astype(dtype)
        s = both if mutant == "half_dropped" else (np.float64(0.5) * both.astype(np.float64)).astype(dtype)
        if epsilon != np.inf:
            small = row_minimum(n, Ap, s, mutant)
            limit = (T(epsilon) * small[rows]).astype(dtype)
            drop = (s > limit) if mutant == "filter_greater" else (s >= limit)
            s = np.where(drop, T(0), s).astype(dtype)
        if mutant != "diagonal_not_reset":
            s[rows == Aj] = T(1)
        s = (s + s[tpos]).astype(dtype)
        keep = s != 0
    Sp = np.zeros(n + 1, np.int64)
    np.add.at(Sp, rows[keep] + 1, 1)
    return {"tpos": tpos, "v": v, "data": data, "s": s, "S": (np.cumsum(Sp).astype(np.int32), Aj[keep].astype(np.int32), s[keep])}


# ---- cusp::gallery::diffusion ------------------------------------------------------------------------------------------------
def diffusion_coefficients(eps, theta, method, dtype):
    """(a, b, c, d, e) in T, as the reference's expressions round them: C, S, CC, SS, CS in T; every expression with a double
    literal in double and rounded once on assignment; FE's `x /= 6.0` is a second double division and rounding."""
    T = np.dtype(dtype).type
    eps, theta = float(eps), float(theta)
    C, S = T(np.cos(theta)), T(np.sin(theta))
    CC, SS, CS = float(T(C * C)), float(T(S * S)), float(T(C * S))
    if method == "FE":
        a = T((-1.0 * eps - 1.0) * CC + (-1.0 * eps - 1.0) * SS + (3.0 * eps - 3.0) * CS)
        b = T((2.0 * eps - 4.0) * CC + (-4.0 * eps + 2.0) * SS)
        c = T((-1.0 * eps - 1.0) * CC + (-1.0 * eps - 1.0) * SS + (-3.0 * eps + 3.0) * CS)
        d = T((-4.0 * eps + 2.0) * CC + (2.0 * eps - 4.0) * SS)
        e = T((8.0 * eps + 8.0) * CC + (8.0 * eps + 8.0) * SS)
        return tuple(T(float(x) / 6.0) for x in (a, b, c, d, e))
    assert method == "FD"
    a = T(0.5 * (eps - 1.0) * CS)
    return a, T(-(eps * SS + CC)), T(-a), T(-(eps * CC + SS)), T(2.0 * (eps + 1.0))


def diffusion(m, n, eps=1e-5, theta=np.pi / 4, method="FE", dtype=np.float64):
    """(N, Ap, Aj, Ax): the nine-point stencil on an m x n grid (m the fast direction), zero stencil values not stored."""
    a, b, c, d, e = diffusion_coefficients(eps, theta, method, dtype)
    stencil = [(-1, -1, a), (0, -1, b), (1, -1, c), (-1, 0, d), (0, 0, e), (1, 0, d), (-1, 1, c), (0, 1, b), (1, 1, a)]
    N = m * n
    Ap, Aj, Ax = [0], [], []
    for r in range(N):
        ix, iy = r % m, r // m
        for dx, dy, val in stencil:
            if 0 <= ix + dx < m and 0 <= iy + dy < n and val != 0:
                Aj.append(r + dx + dy * m)
                Ax.append(val)
        Ap.append(len(Aj))
    return N, np.array(Ap, np.int32), np.array(Aj, np.int32), np.array(Ax, dtype)


# ---- the decks shared by the CPU and the GPU tests ---------------------------------------------------------------------------
def from_dense(M, dtype):
    M = np.asarray(M)
    n = M.shape[0]
    Ap, Aj, Ax = [0], [], []
    for i in range(n):
        for j in np.flatnonzero(M[i]):
            Aj.append(j)
            Ax.append(M[i, j])
        Ap.append(len(Aj))
    return n, np.array(Ap, np.int32), np.array(Aj, np.int32), np.array(Ax, dtype)


def arrow(n, dtype):
    """Row 0 and column 0 full, the diagonal, nothing else: row 0 has n entries, every other row 2."""
    M = np.zeros((n, n))
    k = np.arange(1, n)
    M[0, 1:] = -1.0 / (k + 1)
    M[1:, 0] = -1.0 / (k + 2)
    M[np.arange(n), np.arange(n)] = 2.0 + 0.25 * (np.arange(n) % 5)
    return from_dense(M, dtype)


def tridiagonal_with_gaps(n, dtype, missing=(0, 64, 129)):
    M = np.zeros((n, n))
    i = np.arange(n)
    M[i, i] = 2.0 + 0.125 * (i % 7)
    M[i[:-1], i[:-1] + 1] = -1.0 + 0.0625 * (i[:-1] % 3)
    M[i[1:], i[1:] - 1] = -0.75 - 0.0625 * (i[1:] % 5)
    for r in missing:
        M[r, r] = 0.0
    return from_dense(M, dtype)


def random_symmetric_pattern(n, dtype, seed=7):
    rng = np.random.default_rng(seed)
    mask = rng.random((n, n)) < 0.12
    mask = mask | mask.T | np.eye(n, dtype=bool)
    M = np.where(mask, rng.standard_normal((n, n)), 0.0)                     # unsymmetric values
    M[np.arange(n), np.arange(n)] = 3.0 + rng.random(n)
    B = rng.standard_normal(n)
    B[::5] = 0.0
    B[3] = -0.0
    B[1::7] = -np.abs(B[1::7])
    return from_dense(np.where(mask & (M == 0), 0.5, M), dtype), B.astype(dtype)


def decks(dtype):
    """name -> (n, Ap, Aj, Ax, B, rho, epsilon).  rho is supplied (near each matrix's rho(D^-1 A), any non-zero value serves)."""
    out = {}
    for method in ("FD", "FE"):
        for angle, tag in ((0.0, "0"), (np.pi / 4, "pi/4")):
            N, Ap, Aj, Ax = diffusion(7, 5, 1e-3, angle, method, dtype)
            out[f"diffusion 7x5 {method} angle {tag}"] = (N, Ap, Aj, Ax, np.ones(N, dtype), 1.9, 4.0)
    out["1x1"] = (*from_dense([[3.0]], dtype), np.ones(1, dtype), 1.0, 4.0)
    out["diagonal 65"] = (*from_dense(np.diag(1.0 + np.arange(65) % 4), dtype), np.ones(65, dtype), 1.0, 4.0)
    out["tridiagonal 130 with gaps"] = (*tridiagonal_with_gaps(130, dtype), np.ones(130, dtype), 1.7, 4.0)
    out["arrow 70"] = (*arrow(70, dtype), np.ones(70, dtype), 1.6, 4.0)
    out["arrow 200"] = (*arrow(200, dtype), np.ones(200, dtype), 1.6, 4.0)
    A, B = random_symmetric_pattern(40, dtype)
    out["random 40"] = (*A, B, 1.8, 4.0)
    out["random 40, epsilon inf"] = (*A, B, 1.8, np.inf)
    out["random 40, epsilon 1"] = (*A, B, 1.8, 1.0)
    N, Ap, Aj, Ax = diffusion(7, 5, 1e-3, np.pi / 4, "FE", dtype)
    out["diffusion 7x5 FE angle pi/4, epsilon 1"] = (N, Ap, Aj, Ax, np.ones(N, dtype), 1.9, 1.0)
    out["empty"] = (0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, dtype), np.zeros(0, dtype), 1.5, 4.0)
    return out


def nonconforming():
    """name -> (n, Ap, Aj): patterns that the measure refuses."""
    i32 = lambda *v: np.array(v, np.int32)  # noqa: E731
    return {
        "asymmetric pattern": (3, i32(0, 2, 3, 4), i32(0, 1, 1, 2)),
        "unsorted row": (3, i32(0, 3, 5, 7), i32(0, 2, 1, 0, 1, 0, 2)),
        "repeated column": (2, i32(0, 3, 5), i32(0, 1, 1, 0, 1)),
        "column outside": (2, i32(0, 2, 4), i32(0, 2, 0, 1)),
        "negative column": (2, i32(0, 2, 4), i32(-1, 0, 0, 1)),
    }
