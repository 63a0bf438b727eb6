"""References for the set-up kernels of smoothed-aggregation multigrid, written from the contract of
include/cusp_mi355x.h -- numpy scalars in the value type, one rounding per operation, plain loops:

  strength       keep A_ij when |A_ij| >= theta * sqrt(|A_ii| |A_jj|): product and square root in the value type, the product
                 with theta and the comparison in double; A_ii = 0 where no diagonal is stored, the storage-order sum (from 0)
                 where it is stored more than once; storage order kept.
  scale_rows     out[e] = (Ax[e] / d[row(e)]) * lam, the division first.
  fit            R[a] = sqrt(B[i0]^2 + B[i1]^2 + ...) over the rows of aggregate a in ascending order, starting from the first
                 square; T_i = B[i] / R[aggregates[i]]; a row with aggregates[i] == -1 is empty; an unused id has R = 0.
  elementwise    C(i,j) = the left-to-right sum of A's entries at (i,j) in storage order, then B's (each negated first for
                 subtraction), starting from the first of them; a result equal to zero is dropped, NaN kept.
  presmooth      x[i] = (omega * b[i]) / d[i], the product first.
  standard_aggregate, smooth_prolongator (scale_rows, the SpGEMM of spgemm_refs with zeros dropped, subtract), galerkin
  (two such products), lu_factor / lu_solve (dense, partial pivoting, the first largest pivot).

Plain module: no fixtures, no GPU.  MUTANTS names one deliberately wrong variant per stated order; tests/test_amg_refs.py
proves that a deck catches each of them.
"""
from fractions import Fraction

import numpy as np

import spgemm_refs as SR

DTYPES = (np.float64, np.float32)
MUTANTS = ("sum_from_zero", "rows_descending", "b_before_a", "minus_instead_of_negate", "scale_product_first", "presmooth_quotient_first", "zeros_kept",
           "threshold_in_value_type")


def csr_rows(Ap):
    return np.repeat(np.arange(len(Ap) - 1), np.diff(Ap))


# ---- (a) ------------------------------------------------------------------------------------------------------------------
def diagonal(n, Ap, Aj, Ax):
    """cusp::extract_diagonal: 0 where none is stored, the storage-order sum from 0 where there are several."""
    T = Ax.dtype.type
    d = np.zeros(n, Ax.dtype)
    rows = csr_rows(Ap)
    with np.errstate(all="ignore"):
        for e in np.flatnonzero(np.asarray(Aj) == rows):     # storage order
            d[rows[e]] = T(d[rows[e]] + Ax[e])
    return d


def strong(aij, aii, ajj, theta, mutant=None):
    """Arrays (or scalars) of the value type -> bool: |aij| >= theta * sqrt(|aii| |ajj|)."""
    dtype = np.asarray(aij).dtype
    with np.errstate(all="ignore"):
        root = np.sqrt((np.abs(aii) * np.abs(ajj)).astype(dtype))          # product and square root rounded in the value type
        if mutant == "threshold_in_value_type":
            return np.abs(aij) >= (dtype.type(theta) * root).astype(dtype)
        return np.abs(aij).astype(np.float64) >= np.float64(theta) * root.astype(np.float64)


def strength(n, Ap, Aj, Ax, theta, mutant=None, return_mask=False):
    """(Sp, Sj, Sx): the filtered matrix, storage order kept (return_mask: the kept entries of A as a bool array instead)."""
    d = diagonal(n, Ap, Aj, Ax)
    rows = csr_rows(Ap)
    inside = (Aj >= 0) & (Aj < n)
    ajj = np.where(inside, d[np.where(inside, Aj, 0)], Ax.dtype.type(0)).astype(Ax.dtype) if n else np.zeros(0, Ax.dtype)
    keep = np.asarray(strong(Ax, d[rows], ajj, theta, mutant), bool) if len(Aj) else np.zeros(0, bool)
    if return_mask:
        return keep
    Sp = np.zeros(n + 1, np.int64)
    np.add.at(Sp, rows[keep] + 1, 1)
    return np.cumsum(Sp).astype(np.int32), Aj[keep].astype(np.int32), Ax[keep]


# ---- (b), (e) -------------------------------------------------------------------------------------------------------------
def scale_rows(Ap, Ax, d, lam, mutant=None):
    T = Ax.dtype.type
    dr = d[csr_rows(Ap)]
    with np.errstate(all="ignore"):
        if mutant == "scale_product_first":
            return ((Ax * T(lam)).astype(Ax.dtype) / dr).astype(Ax.dtype)
        return ((Ax / dr).astype(Ax.dtype) * T(lam)).astype(Ax.dtype)


def presmooth(d, b, omega, mutant=None):
    T = b.dtype.type
    with np.errstate(all="ignore"):
        if mutant == "presmooth_quotient_first":
            return (T(omega) * (b / d).astype(b.dtype)).astype(b.dtype)
        return ((T(omega) * b).astype(b.dtype) / d).astype(b.dtype)


# ---- (c) ------------------------------------------------------------------------------------------------------------------
def fit(aggregates, B, num_aggregates, mutant=None):
    """(Tp, Tj, Tx, R)."""
    T = B.dtype.type
    n = len(aggregates)
    assert all(-1 <= a < num_aggregates for a in aggregates)
    R = np.zeros(num_aggregates, B.dtype)
    with np.errstate(all="ignore"):
        for a in range(num_aggregates):
            rows = np.flatnonzero(aggregates == a)             # ascending
            if len(rows) == 0:
                continue
            if mutant == "rows_descending":
                rows = rows[::-1]
            if mutant == "sum_from_zero":
                s, rest = T(0), rows
            else:
                s, rest = T(B[rows[0]] * B[rows[0]]), rows[1:]
            for i in rest:
                s = T(s + T(B[i] * B[i]))
            R[a] = np.sqrt(s)
        inside = aggregates >= 0
        Tp = np.r_[0, np.cumsum(inside)].astype(np.int32)
        Tj = aggregates[inside].astype(np.int32)
        Tx = (B[inside] / R[Tj]).astype(B.dtype)
    return Tp, Tj, Tx, R


# ---- (d) ------------------------------------------------------------------------------------------------------------------
def is_sorted(n_cols, Ap, Aj):
    Ap = np.asarray(Ap, np.int64)
    if Ap[0] != 0 or Ap[-1] != len(Aj) or np.any(np.diff(Ap) < 0):
        return False
    if len(Aj) and (Aj.min() < 0 or Aj.max() >= n_cols):
        return False
    rows = csr_rows(Ap)
    return bool(np.all((rows[1:] != rows[:-1]) | (Aj[1:] >= Aj[:-1])))


def chain_value(a_vals, b_vals, op, T, mutant=None):
    """The value of one (i, j) BEFORE the zero test: A's entries left to right, then B's, from the first of them.  Subtraction
    negates each value of B and adds it; the mutant subtracts instead (from +0 where B's value comes first), which differs in
    the sign of a zero only: -(+0.0) is -0.0, 0 - (+0.0) is +0.0.  Both are dropped by the zero test, so the difference is
    visible here and in no stored entry."""
    terms = [(v, 0) for v in a_vals] + [(v, 1) for v in b_vals]
    if mutant == "b_before_a":
        terms = [(v, 1) for v in b_vals] + [(v, 0) for v in a_vals]
    s = None
    with np.errstate(all="ignore"):
        for v, which in terms:
            if which == 1 and op == "subtract":
                if mutant == "minus_instead_of_negate":
                    s = T(T(0) - v) if s is None else T(s - v)
                    continue
                v = T(-v)
            s = v if s is None else T(s + v)
    return s


def elementwise(m, n, Ap, Aj, Ax, Bp, Bj, Bx, op, mutant=None):
    """(Cp, Cj, Cx) for op "add" / "subtract"; the operands' rows are sorted by column (a column may repeat)."""
    assert is_sorted(n, Ap, Aj) and is_sorted(n, Bp, Bj)
    T = Ax.dtype.type
    Cp, Cj, Cx = [0], [], []
    for i in range(m):
        chains = {}
        for q in range(Ap[i], Ap[i + 1]):
            chains.setdefault(int(Aj[q]), ([], []))[0].append(Ax[q])
        for q in range(Bp[i], Bp[i + 1]):
            chains.setdefault(int(Bj[q]), ([], []))[1].append(Bx[q])
        for c in sorted(chains):
            s = chain_value(*chains[c], op, T, mutant)
            if s == 0 and mutant != "zeros_kept":
                continue
            Cj.append(c)
            Cx.append(s)
        Cp.append(len(Cj))
    return np.array(Cp, np.int32), np.array(Cj, np.int32), np.array(Cx, Ax.dtype)


def exact_elementwise(m, Ap, Aj, Ax, Bp, Bj, Bx, op):
    """{(i, j): Fraction} of A +/- B, zero results dropped."""
    out = {}
    for i in range(m):
        for q in range(Ap[i], Ap[i + 1]):
            out[(i, int(Aj[q]))] = out.get((i, int(Aj[q])), Fraction(0)) + Fraction(float(Ax[q]))
        for q in range(Bp[i], Bp[i + 1]):
            v = Fraction(float(Bx[q]))
            out[(i, int(Bj[q]))] = out.get((i, int(Bj[q])), Fraction(0)) + (-v if op == "subtract" else v)
    return {k: v for k, v in out.items() if v != 0}


# ---- aggregation, prolongator, Galerkin product -----------------------------------------------------------------------------
def standard_aggregate(n, Ap, Aj):
    """The reference's three-pass sequential aggregation on the structure of C: (aggregates int32 with -1 = isolated, roots)."""
    agg = np.zeros(n, np.int64)
    roots = {}
    nxt = 1
    for i in range(n):
        if agg[i]:
            continue
        has_n = has_a = False
        for jj in range(Ap[i], Ap[i + 1]):
            j = Aj[jj]
            if j != i:
                has_n = True
                if agg[j]:
                    has_a = True
                    break
        if not has_n:
            agg[i] = -n
        elif not has_a:
            agg[i] = nxt
            roots[nxt - 1] = i
            for jj in range(Ap[i], Ap[i + 1]):
                agg[Aj[jj]] = nxt
            nxt += 1
    for i in range(n):
        if agg[i]:
            continue
        for jj in range(Ap[i], Ap[i + 1]):
            t = agg[Aj[jj]]
            if t > 0:
                agg[i] = -t
                break
    nxt -= 1
    for i in range(n):
        t = agg[i]
        if t != 0:
            agg[i] = t - 1 if t > 0 else (-1 if t == -n else -t - 1)
            continue
        agg[i] = nxt
        roots[nxt] = i
        for jj in range(Ap[i], Ap[i + 1]):
            if agg[Aj[jj]] == 0:
                agg[Aj[jj]] = nxt
        nxt += 1
    return agg.astype(np.int32), np.array([roots[a] for a in range(nxt)], np.int32)


def multiply(A, B):
    """The host SpGEMM of spgemm_refs (zero sums dropped) on (rows, cols, Ap, Aj, Ax) tuples."""
    assert A[1] == B[0]
    return (A[0], B[1], *SR.spgemm(A[0], A[1], B[1], *A[2:], *B[2:], drop_zeros=True))


def smooth_prolongator(S, Tm, rho, omega=4.0 / 3.0):
    """P = T - (omega / rho) D^-1 S T in the sequential path's order: scale_rows, multiply, subtract."""
    n, _, Sp, Sj, Sx = S
    T = Sx.dtype.type
    d = diagonal(n, Sp, Sj, Sx)
    lam = T(omega / rho)
    DinvS = (n, n, Sp, Sj, scale_rows(Sp, Sx, d, lam))
    temp = multiply(DinvS, Tm)
    return (Tm[0], Tm[1], *elementwise(Tm[0], Tm[1], *Tm[2:], *temp[2:], "subtract"))


def galerkin(R, A, P):
    return multiply(R, multiply(A, P))


# ---- dense LU ---------------------------------------------------------------------------------------------------------------
def lu_factor(M):
    """In place on a copy: (LU, pivot) by rows with partial pivoting (the first row of largest magnitude); raises on a zero pivot."""
    A = np.array(M)
    T = A.dtype.type
    n = A.shape[0]
    piv = np.arange(n)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if A[p, k] == 0:
            raise ZeroDivisionError("singular matrix")
        if p != k:
            A[[k, p]] = A[[p, k]]
            piv[[k, p]] = piv[[p, k]]
        for i in range(k + 1, n):
            A[i, k] = T(A[i, k] / A[k, k])
            for j in range(k + 1, n):
                A[i, j] = T(A[i, j] - T(A[i, k] * A[k, j]))
    return A, piv


def lu_solve(LU, piv, b):
    T = LU.dtype.type
    n = len(b)
    x = b[piv].astype(LU.dtype)
    for i in range(n):
        for j in range(i):
            x[i] = T(x[i] - T(LU[i, j] * x[j]))
    for i in range(n - 1, -1, -1):
        for j in range(i + 1, n):
            x[i] = T(x[i] - T(LU[i, j] * x[j]))
        x[i] = T(x[i] / LU[i, i])
    return x


# ---- decks ------------------------------------------------------------------------------------------------------------------
def next_after(v, up):
    T = type(v)
    return np.nextafter(v, T(np.inf) if up else T(-np.inf))


def threshold_deck(dtype):
    """A 2 x 2 matrix per case with diagonal (a, c) and A_01 placed AT theta * sqrt(a c) as double arithmetic gives it, one
    ulp below and one ulp above: (n, Ap, Aj, Ax, theta, keeps A_01?)."""
    T = np.dtype(dtype).type
    out = []
    for a, c, theta in ((4.0, 9.0, 0.25), (3.0, 5.0, 0.25), (1.0, 1.0, 1.0), (2.0, 7.0, 1.0), (1.0, 3.0, 0.1)):
        root = np.sqrt(T(T(a) * T(c)))
        limit = np.float64(theta) * np.float64(root)
        v = T(limit)
        if np.float64(v) < limit:
            v = next_after(v, True)                            # the smallest value of the type that passes
        for val, keep in ((v, True), (next_after(v, False), False), (next_after(v, True), True)):
            Ap, Aj, Ax = SR.csr([[(0, a), (1, -val)], [(0, 0.0), (1, c)]], dtype)
            out.append((2, Ap, Aj, Ax, theta, keep))
    return out


def value_type_threshold_case():
    """f32: theta = 0.1 is not a float, so float(theta) * sqrt(1 * c) rounded to float is not the double product theta * sqrt.
    The first c whose float threshold lies BELOW the double one: A_01 = the float threshold passes in float and fails in double."""
    T = np.float32
    for c in range(2, 100):
        root = np.sqrt(T(c))
        v = T(T(0.1) * root)
        if np.float64(v) < 0.1 * np.float64(root):
            Ap, Aj, Ax = SR.csr([[(0, 1.0), (1, v)], [(1, float(c))]], T)
            return 2, Ap, Aj, Ax, 0.1, False
    raise AssertionError("no such c")


def binade_deck(dtype, count=60, reps=200):
    """One aggregate, B = 2^29 and then 2^-30 .. 2^28 (`count` binades, each value `reps` times), all positive: no cancellation.
    In row order the large square comes first and swallows every square below half its ulp, one at a time; in an order that
    lets the small squares accumulate first they carry into it, by tens of ulps: the rounded sum tells the order."""
    T = np.dtype(dtype).type
    k = np.r_[count // 2 - 1, np.repeat(np.arange(count - 1) - count // 2, reps)]
    return np.zeros(len(k), np.int32), (T(2.0) ** k.astype(dtype)).astype(dtype)


def random_sorted_csr(rng, m, n, density, dtype, duplicates=True):
    lens = rng.binomial(max(n, 1), density, size=m) if n else np.zeros(m, np.int64)
    Ap = np.r_[0, np.cumsum(lens)].astype(np.int32)
    if duplicates:
        rows = [np.sort(rng.integers(0, n, size=l)) for l in lens]
    else:
        rows = [np.sort(rng.permutation(n)[:l]) for l in lens]
    Aj = np.concatenate(rows + [np.zeros(0, np.int64)]).astype(np.int32)
    Ax = rng.integers(-4, 5, size=len(Aj)).astype(dtype) * dtype(0.25)   # small multiples of 1/4: cancellations happen, sums are exact
    return Ap, Aj, Ax
