"""References for the CSR x CSR multiply (SpGEMM), written from the contract of DESIGN 3.9 -- numpy, in the value type:

  structure  one entry of C per distinct (i, c) with at least one structural product A(i,j) B(j,c); every row's columns
             strictly ascending; exact-zero sums are KEPT (the device) -- `drop_zeros` removes them (the host path).
  values     s = T(0); for jj over row i of A in storage order, for kk over row Aj[jj] of B in storage order with
             Bj[kk] == c: s = s + (Ax[jj] * Bx[kk]); multiply and add rounded separately.

Plain module: no fixtures, no GPU.  `spgemm` is the fast restatement (all products expanded in expansion order, a STABLE
sort by (row, column), then the chains advanced one position at a time over all segments at once: every add is one numpy
add in the value type, in chain order).  `spgemm_loop` is the slow literal restatement with dictionaries, and carries the
five deliberately wrong variants (MUTANTS) that tests/test_spgemm_refs.py proves the decks below catch:

  mutant            caught by deck
  reversed          order        (big, 1, big, 1, -big over duplicate columns and several rows of B: any re-association changes bits)
  start_at_first    minus_zero   (a lone product of -0.0 must come out +0.0)
  fma               fma          (a product whose rounding error survives only when fused)
  drop_zeros        cancel       (an exact cancellation is a kept 0.0 entry; `fma` catches it as well)
  unsorted          order        (first-touch column order of row 0 is 1, 0)
"""
from fractions import Fraction

import numpy as np

DTYPES = (np.float64, np.float32)
MUTANTS = ("reversed", "start_at_first", "fma", "drop_zeros", "unsorted")
CAUGHT_BY = {"reversed": "order", "start_at_first": "minus_zero", "fma": "fma", "drop_zeros": "cancel", "unsorted": "order"}


def csr(rows, dtype):
    """CSR arrays from a list of rows, each a list of (column, value) in storage order."""
    Ap = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int32)
    Aj = np.array([c for r in rows for c, _ in r], np.int32)
    Ax = np.array([v for r in rows for _, v in r], dtype)
    return Ap, Aj, Ax


def expand(m, Ap, Aj, Bp, Bj):
    """Every product in expansion order: (row of A, entry of A, entry of B), int64 arrays."""
    Ap, Bp = np.asarray(Ap, np.int64), np.asarray(Bp, np.int64)
    a_ent = np.arange(Ap[0], Ap[m], dtype=np.int64)
    a_row = np.repeat(np.arange(m, dtype=np.int64), np.diff(Ap[:m + 1]))
    j = np.asarray(Aj, np.int64)[a_ent]
    blen = Bp[j + 1] - Bp[j]
    e = np.repeat(a_ent, blen)
    first = np.cumsum(blen) - blen
    kk = np.repeat(Bp[j], blen) + (np.arange(int(blen.sum()), dtype=np.int64) - np.repeat(first, blen))
    return np.repeat(a_row, blen), e, kk


def spgemm(m, k, n, Ap, Aj, Ax, Bp, Bj, Bx, drop_zeros=False):
    """C = A B by the contract.  Returns (Cp int32, Cj int32, Cx in the type of Ax)."""
    dtype = Ax.dtype
    assert Bx.dtype == dtype
    row, e, kk = expand(m, Ap, Aj, Bp, Bj)
    col = np.asarray(Bj, np.int64)[kk]
    with np.errstate(all="ignore"):
        prod = (Ax[e] * Bx[kk]).astype(dtype)            # one rounding: the multiply
    order = np.lexsort((col, row))                        # stable: equal (row, column) stay in expansion order
    row, col, prod = row[order], col[order], prod[order]
    P = len(prod)
    head = np.ones(P, bool)
    head[1:] = (row[1:] != row[:-1]) | (col[1:] != col[:-1])
    start = np.flatnonzero(head)
    length = np.diff(np.r_[start, P])
    s = np.zeros(len(start), dtype)                       # every chain starts at +0
    with np.errstate(all="ignore"):
        for t in range(int(length.max()) if len(length) else 0):
            live = np.flatnonzero(length > t)
            s[live] = s[live] + prod[start[live] + t]     # one rounding: the add
    crow, ccol = row[start], col[start]
    if drop_zeros:
        keep = ~(s == 0)                                  # NaN is kept: it does not compare equal to zero
        crow, ccol, s = crow[keep], ccol[keep], s[keep]
    Cp = np.zeros(m + 1, np.int64)
    np.add.at(Cp, crow + 1, 1)
    return np.cumsum(Cp).astype(np.int32), ccol.astype(np.int32), s


def _fma(a, b, s):
    """round(a * b + s) with ONE rounding (finite arguments)."""
    T = type(s)
    if T is np.float32:
        return np.float32(np.longdouble(a) * np.longdouble(b) + np.longdouble(s))  # the product of two f32 is exact in longdouble
    return np.float64(float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(s))))


def spgemm_loop(m, k, n, Ap, Aj, Ax, Bp, Bj, Bx, mutant=None, drop_zeros=False):
    """The literal restatement, one Python loop per level; `mutant` is one of MUTANTS or None."""
    assert mutant is None or mutant in MUTANTS
    T = Ax.dtype.type
    Cp, Cj, Cx = [0], [], []
    with np.errstate(all="ignore"):
        for i in range(m):
            chains = {}                                   # column -> [(a, b), ...] in expansion order; dicts keep first-touch order
            for jj in range(Ap[i], Ap[i + 1]):
                j = Aj[jj]
                for kk in range(Bp[j], Bp[j + 1]):
                    chains.setdefault(int(Bj[kk]), []).append((Ax[jj], Bx[kk]))
            cols = list(chains) if mutant == "unsorted" else sorted(chains)
            for c in cols:
                terms = chains[c][::-1] if mutant == "reversed" else chains[c]
                if mutant == "start_at_first":
                    s = T(terms[0][0] * terms[0][1])
                    terms = terms[1:]
                else:
                    s = T(0)
                for a, b in terms:
                    s = _fma(a, b, s) if mutant == "fma" else T(s + T(a * b))
                if (drop_zeros or mutant == "drop_zeros") and s == 0:
                    continue
                Cj.append(c)
                Cx.append(s)
            Cp.append(len(Cj))
    return np.array(Cp, np.int32), np.array(Cj, np.int32), np.array(Cx, Ax.dtype)


def exact(m, k, n, Ap, Aj, Ax, Bp, Bj, Bx):
    """{(i, c): Fraction} -- the exact product, for inputs whose partial sums are representable."""
    out = {}
    for i in range(m):
        for jj in range(Ap[i], Ap[i + 1]):
            j = Aj[jj]
            for kk in range(Bp[j], Bp[j + 1]):
                key = (i, int(Bj[kk]))
                out[key] = out.get(key, Fraction(0)) + Fraction(float(Ax[jj])) * Fraction(float(Bx[kk]))
    return out


def transpose(rows, cols, Ap, Aj, Ax):
    """CSR of the transpose (stable: a column's entries in row order)."""
    Ai = np.repeat(np.arange(rows), np.diff(Ap))
    order = np.argsort(Aj, kind="stable")
    Tp = np.zeros(cols + 1, np.int64)
    np.add.at(Tp, np.asarray(Aj, np.int64) + 1, 1)
    return np.cumsum(Tp).astype(np.int32), Ai[order].astype(np.int32), Ax[order]


def poisson5pt(nx, ny, dtype):
    """The 5-point Laplacian on an nx x ny grid (4 on the diagonal, -1 off it), sorted rows: (N, Ap, Aj, Ax)."""
    r = np.arange(nx * ny)
    ix, iy = r % nx, r // nx
    cand = np.stack([r - nx, r - 1, r, r + 1, r + nx], 1)
    keep = np.stack([iy > 0, ix > 0, np.ones_like(r, bool), ix < nx - 1, iy < ny - 1], 1)
    vals = np.broadcast_to(np.array([-1, -1, 4, -1, -1], dtype), cand.shape)
    Ap = np.r_[0, np.cumsum(keep.sum(1))].astype(np.int32)
    return nx * ny, Ap, cand[keep].astype(np.int32), vals[keep].astype(dtype)


def aggregation_2x2(nx, ny, dtype):
    """The piecewise-constant prolongator of 2 x 2 aggregates on an nx x ny grid (nx, ny even): (nx ny) x (nx ny / 4), one 1 per row."""
    r = np.arange(nx * ny)
    agg = (r // nx // 2) * (nx // 2) + (r % nx) // 2
    return np.arange(nx * ny + 1, dtype=np.int32), agg.astype(np.int32), np.ones(nx * ny, dtype)


# ------------------------------------------------------------------------------------------------
# decks: name -> (m, k, n, Ap, Aj, Ax, Bp, Bj, Bx)
# ------------------------------------------------------------------------------------------------
def decks(dtype):
    dtype = np.dtype(dtype)
    T = dtype.type
    big = T(2.0) ** (53 if dtype == np.float64 else 24)   # big + 1 rounds back to big (ties to even); 2 + big is representable
    eps = T(2.0) ** (-30 if dtype == np.float64 else -13)  # (1 + eps)^2 = 1 + 2 eps + eps^2, and eps^2 is below half an ulp
    out = {}
    # C(0,0) = big + 1 + 1 + big + 1 - big in that order (= big); reversed it is big + 2.  Row 0 of A is unsorted and holds column 2
    # twice; row 2 of B is unsorted and holds column 0 twice; the first column row 0 touches is 1.
    A = csr([[(2, 1.0), (0, 1.0), (2, 1.0), (1, 1.0)], [(1, 2.0)]], dtype)
    B = csr([[(0, 1.0), (1, 1.0)], [(0, -big), (1, 2.0)], [(1, 3.0), (0, big), (0, 1.0)]], dtype)
    out["order"] = (2, 3, 2, *A, *B)
    # a lone product of -0.0; a sum of two -0.0 products (still +0.0: the chain starts at +0)
    A = csr([[(0, -0.0)], [(0, -0.0), (1, -0.0)]], dtype)
    B = csr([[(0, 1.0)], [(0, 2.0)]], dtype)
    out["minus_zero"] = (2, 2, 1, *A, *B)
    # -(1 + 2 eps) first, then (1 + eps)(1 + eps): unfused 0.0 exactly, fused eps^2
    A = csr([[(0, 1.0), (1, 1.0 + eps)]], dtype)
    B = csr([[(0, -(1.0 + 2 * eps))], [(0, 1.0 + eps)]], dtype)
    out["fma"] = (1, 2, 1, *A, *B)
    # exact cancellation next to an ordinary entry, and an explicit zero of A times a value
    A = csr([[(0, 1.0), (1, 1.0)], [(0, 0.0)]], dtype)
    B = csr([[(0, 1.0), (1, 5.0)], [(0, -1.0)]], dtype)
    out["cancel"] = (2, 2, 2, *A, *B)
    # Inf * 0 is a NaN entry; Inf - Inf too; NaN propagates; an Inf alone stays
    A = csr([[(0, np.inf)], [(0, np.inf), (1, -np.inf)], [(1, np.nan), (2, 1.0)], [(2, np.inf)]], dtype)
    B = csr([[(0, 0.0)], [(0, 1.0)], [(0, 2.0), (1, -1.0)]], dtype)
    out["inf_nan"] = (4, 3, 2, *A, *B)
    return out


def random_pair(rng, m, k, n, da, db, dtype, duplicates=True):
    """Random CSR A (m x k) and B (k x n) with densities da, db; rows unsorted, duplicates allowed, some explicit zeros."""
    def one(rows, cols, d):
        lens = rng.binomial(cols, d, size=rows) if cols else np.zeros(rows, np.int64)
        Ap = np.r_[0, np.cumsum(lens)].astype(np.int32)
        nnz = int(Ap[-1])
        if duplicates:
            Aj = rng.integers(0, max(cols, 1), size=nnz).astype(np.int32)
        else:
            Aj = np.concatenate([rng.permutation(cols)[:l] for l in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
        Ax = rng.standard_normal(nnz).astype(dtype)
        Ax[rng.random(nnz) < 0.05] = 0
        return Ap, Aj, Ax
    return (m, k, n, *one(m, k, da), *one(k, n, db))
