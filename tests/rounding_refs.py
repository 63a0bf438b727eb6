"""Exact row sums, the rounding-error bound and the matrices of tests/test_rounding_gpu.py, plus numpy restatements of
honest and of subtly wrong summation orders (tests/test_rounding_refs.py checks all of it on the CPU).

The bar.  A kernel that multiplies and adds in the working precision T (unit roundoff u: 2^-53 for f64, 2^-24 for f32)
computes, for a row of n terms (the products a_ij x_j, plus y0 when accumulating) added in ANY order, with or without FMA,

    |y - exact| <= gamma_n * B,    gamma_n = n u / (1 - n u),    B = sum_j |a_ij x_j| (+ |y0|)

(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: each term passes through at most n roundings -- one
for its product, at most n - 1 for the additions above it).  The reference here is the exact sum rounded ONCE to float64,
which costs one more u: the tests hold |y - round(exact)| <= gamma_{n+1} B.  Nothing gets a looser bar than the suite's older
one (1e-6 B for f64, 1e-5 B for f32): f32 rows beyond about 160 terms keep 1e-5.
"""
import math
from types import SimpleNamespace

import numpy as np

U = {np.dtype(np.float64): 2.0 ** -53, np.dtype(np.float32): 2.0 ** -24}
TOL_TODAY = {np.dtype(np.float64): 1e-6, np.dtype(np.float32): 1e-5}

LADDER_LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513,
                  1023, 1025, 4097)
ELL_LENGTHS = tuple(l for l in LADDER_LENGTHS if l <= 129)
COLS = 5000
GIANT_LENGTH = 100000
PROFILES = ("normal", "wide")


def gamma(n, dtype):
    """gamma_n(u_T) = n u / (1 - n u), elementwise."""
    nu = np.asarray(n, np.float64) * U[np.dtype(dtype)]
    return nu / (1.0 - nu)


def bar(n, dtype):
    """The factor of B a row of n terms is held to: min(today's tolerance, gamma_{n+1})."""
    return np.minimum(TOL_TODAY[np.dtype(dtype)], gamma(np.asarray(n) + 1, dtype))


# ------------------------------------------------------------------------------------------------------------------------
# exact row sums
# ------------------------------------------------------------------------------------------------------------------------
def two_product(a, b):
    """Veltkamp / Dekker: p = fl(a b) and e with p + e == a b exactly (float64 arrays, no overflow / underflow in range here)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    p = a * b
    split = 134217729.0  # 2^27 + 1
    ca, cb = split * a, split * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def exact_rows(Ap, Aj, Ax, x, y0=None):
    """Per row: (the exact sum of the products a_ij x_j (+ y0), rounded once to float64;  B = sum |a_ij x_j| (+ |y0|),
    over-estimated by at most 2^-50 relative and never under-estimated;  n = number of terms, y0 counting as one).
    f32 inputs: the products are exact in float64; f64 inputs: each product is split into two float64 pieces without error.
    Either way math.fsum adds a row's pieces exactly and rounds once."""
    Ap = np.asarray(Ap, np.int64)
    rows = len(Ap) - 1
    a, b = np.asarray(Ax), np.asarray(x)[np.asarray(Aj, np.int64)]
    if a.dtype == np.float32:
        p = a.astype(np.float64) * b.astype(np.float64)
        e = None
    else:
        p, e = two_product(a, b)
    absp = np.abs(p)
    abse = None if e is None else np.where(p < 0, -e, e)  # |p + e| = |p| + sign(p) e  (|e| <= ulp(p) / 2)
    exact, B = np.zeros(rows), np.zeros(rows)
    n = np.diff(Ap) + (0 if y0 is None else 1)
    for i in range(rows):
        lo, hi = int(Ap[i]), int(Ap[i + 1])
        parts, mags = p[lo:hi].tolist(), absp[lo:hi].tolist()
        if e is not None:
            parts += e[lo:hi].tolist()
            mags += abse[lo:hi].tolist()
        if y0 is not None:
            parts.append(float(y0[i]))
            mags.append(abs(float(y0[i])))
        exact[i] = math.fsum(parts)
        B[i] = math.fsum(mags)
    return exact, B * (1.0 + 2.0 ** -50), n.astype(np.int64)


def within_rounding_bound(got, exact, B, n, dtype):
    """The rows of `got` outside the bar, as (row, got, exact, n, err / B, bar):
      n == 0: +0.0 to the bit;   n == 1 (one product, or y0 alone): that value rounded to T;
      otherwise |got - exact| <= min(TOL_TODAY, gamma_{n+1}(u_T)) * B."""
    dtype = np.dtype(dtype)
    got = np.asarray(got)
    assert got.dtype == dtype and got.shape == exact.shape == B.shape == n.shape
    g = got.astype(np.float64)
    lim = bar(n, dtype)
    err = np.abs(g - exact)
    with np.errstate(invalid="ignore"):
        ok = err <= lim * B  # (NaN / inf in got: False)
    zero_bits = np.zeros(1, dtype).view(np.uint64 if dtype == np.float64 else np.uint32)[0]
    bits = got.view(np.uint64 if dtype == np.float64 else np.uint32)
    ok = np.where(n == 0, bits == zero_bits, ok)
    ok = np.where(n == 1, g == exact.astype(dtype).astype(np.float64), ok)
    bad = np.nonzero(~ok)[0]
    return [(int(i), float(g[i]), float(exact[i]), int(n[i]), float(err[i] / B[i]) if B[i] > 0 else float("inf"), float(lim[i])) for i in bad]


def worst_ratio(got, exact, B, n, dtype, min_terms=2):
    """max over rows with n >= min_terms of err / (gamma_{n+1} B): information for the tables, never a threshold."""
    m = (n >= min_terms) & (B > 0)
    if not m.any():
        return 0.0
    err = np.abs(np.asarray(got)[m].astype(np.float64) - exact[m])
    return float(np.max(err / (gamma(n[m] + 1, dtype) * B[m])))


def describe(bad, limit=3):
    """Failure text: row, n, err / B and the bar of the first offenders."""
    return "; ".join(f"row {i}: n={nn} got={g!r} exact={e!r} err/B={r:.3e} bar={l:.3e}" for i, g, e, nn, r, l in bad[:limit]) + \
        (f" (+{len(bad) - limit} more)" if len(bad) > limit else "")


# ------------------------------------------------------------------------------------------------------------------------
# matrices
# ------------------------------------------------------------------------------------------------------------------------
def _values(rng, size, profile):
    if profile == "normal":
        return rng.standard_normal(size)
    assert profile == "wide"
    return np.exp2(rng.uniform(-20.0, 20.0, size)) * rng.choice((-1.0, 1.0), size)


def _row_lengths(lengths, seed):
    """Each ladder length three times in a seeded shuffle, with a block of 64 rows of 16, 300 empty rows and a block of 64 rows of 3
    in between; the last row is not empty."""
    rng = np.random.default_rng(seed)
    lad = np.array(sorted(lengths) * 3)
    rng.shuffle(lad)
    third = len(lad) // 3
    return np.concatenate([lad[:third], np.full(64, 16), lad[third:2 * third], np.zeros(300, np.int64), lad[2 * third:], np.full(64, 3), [7]])


def _build(lens, profile, dtype, seed, giant_at=None):
    rng = np.random.default_rng(seed)
    cols = [np.sort(rng.choice(COLS, size=int(l), replace=False)) for l in lens]
    if giant_at is not None:  # (drawn last, so the other rows are the ladder's own)
        cols.insert(giant_at, np.sort(rng.integers(0, COLS, GIANT_LENGTH)))
        lens = np.insert(lens, giant_at, GIANT_LENGTH)
    Ap = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    Aj = np.concatenate(cols).astype(np.int32)
    vrng = np.random.default_rng(seed + 1000)
    Ax = _values(vrng, len(Aj), profile).astype(dtype)
    x = _values(vrng, COLS, profile).astype(dtype)
    y0 = vrng.standard_normal(len(lens)).astype(dtype)
    return SimpleNamespace(rows=len(lens), cols=COLS, Ap=Ap, Aj=Aj, Ax=Ax, x=x, y0=y0, lengths=np.diff(Ap).astype(np.int64),
                           profile=profile, dtype=np.dtype(dtype))


_cache = {}


def matrix(name, profile="normal", dtype=np.float64):
    """"ladder": 519 rows of the ladder lengths, 5000 columns (sorted in a row, no duplicates); "giant": ladder with one row of
    100 000 entries (columns repeat) put in as row 100; "ell_ladder": the lengths up to 129.  Cached: treat as read-only."""
    key = (name, profile, np.dtype(dtype))
    if key not in _cache:
        if name == "ladder":
            M = _build(_row_lengths(LADDER_LENGTHS, 7), profile, dtype, 11)
        elif name == "giant":
            M = _build(_row_lengths(LADDER_LENGTHS, 7), profile, dtype, 11, giant_at=100)
        elif name == "ell_ladder":
            M = _build(_row_lengths(ELL_LENGTHS, 8), profile, dtype, 12)
        else:
            raise KeyError(name)
        M.name = name
        for a in (M.Ap, M.Aj, M.Ax, M.x, M.y0):
            a.setflags(write=False)
        _cache[key] = M
    return _cache[key]


def exact_of(M, accumulate):
    """exact_rows of a cached matrix, computed once per (matrix, accumulate)."""
    key = ("exact", M.name, M.profile, M.dtype, bool(accumulate))
    if key not in _cache:
        _cache[key] = exact_rows(M.Ap, M.Aj, M.Ax, M.x, M.y0 if accumulate else None)
    return _cache[key]


# ------------------------------------------------------------------------------------------------------------------------
# summation orders in numpy: honest ones, and mutants with one defect each
# ------------------------------------------------------------------------------------------------------------------------
def _tree(v):
    """Fold a power-of-two number of lanes as a shuffle tree does: lane k += lane k + half."""
    while len(v) > 1:
        h = len(v) // 2
        v = v[:h] + v[h:]
    return v[0]


def _lane_partials(terms, lanes, carry):
    """Lane l adds terms l, l + lanes, ... in order, its partial sum carried in `carry`."""
    k = -(-len(terms) // lanes)
    t = np.zeros(k * lanes, terms.dtype)
    t[:len(terms)] = terms
    return np.cumsum(t.reshape(k, lanes).astype(carry), axis=0, dtype=carry)[-1]  # (np.cumsum adds sequentially in `carry`)


def strided_sum(terms, lanes, y0=None, carry=None, final_fold=None):
    """`lanes` strided lanes, then a tree, then y0 on top -- in the terms' own type unless a defect is asked for:
    carry = the type the lane partials are kept in;  final_fold = the type the last cross-lane add passes through."""
    T = terms.dtype
    if len(terms) == 0:
        total = T.type(0)
    else:
        v = _lane_partials(terms, lanes, carry or T).astype(T)
        if final_fold is not None and lanes > 1:
            while len(v) > 2:
                h = len(v) // 2
                v = v[:h] + v[h:]
            total = T.type(v[0].astype(final_fold) + v[1].astype(final_fold))
        else:
            total = _tree(v)
    return total if y0 is None else T.type(y0 + total)


def reverse_sum(terms, y0=None):
    T = terms.dtype
    total = np.cumsum(terms[::-1], dtype=T)[-1] if len(terms) else T.type(0)
    return total if y0 is None else T.type(total + y0)


def pairwise_sum(terms, y0=None):
    T = terms.dtype
    if y0 is not None:
        terms = np.concatenate([[y0], terms]).astype(T)
    if len(terms) == 0:
        return T.type(0)
    size = 1 << (len(terms) - 1).bit_length()
    v = np.zeros(size, T)
    v[:len(terms)] = terms
    while len(v) > 1:
        v = v[0::2] + v[1::2]
    return v[0]


def row_terms(M, i):
    """The rounded products of row i, in storage order, in the matrix's type."""
    lo, hi = int(M.Ap[i]), int(M.Ap[i + 1])
    return M.Ax[lo:hi] * M.x[M.Aj[lo:hi]]


HONEST = {f"strided{l}": (lambda t, y0, l=l: strided_sum(t, l, y0)) for l in (2, 4, 8, 16, 32, 64)}
HONEST["reverse"] = reverse_sum
HONEST["pairwise"] = pairwise_sum

MUTANT_LANES = 8
MUTANTS = {
    "float32 carry": lambda t, y0: strided_sum(t, MUTANT_LANES, y0, carry=np.float32),
    "float32 final fold": lambda t, y0: strided_sum(t, MUTANT_LANES, y0, final_fold=np.float32),
    "last term dropped": lambda t, y0: strided_sum(t[:-1], MUTANT_LANES, y0),
    "first term twice": lambda t, y0: strided_sum(np.concatenate([t[:1], t]), MUTANT_LANES, y0),
}


def bfloat16_round(v):
    """float32 -> bfloat16 (round to nearest even) -> float32."""
    b = np.asarray(v, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def bfloat16_carry_sum(terms, lanes, y0=None):
    """f32 mutant: every lane's running sum is stored as bfloat16 after each add."""
    T = terms.dtype
    k = -(-len(terms) // lanes)
    t = np.zeros(k * lanes, T)
    t[:len(terms)] = terms
    acc = np.zeros(lanes, np.float32)
    for step in t.reshape(k, lanes):
        acc = bfloat16_round(acc + step.astype(np.float32))
    total = _tree(acc.astype(T))
    return total if y0 is None else T.type(y0 + total)


def apply_order(M, order, accumulate, rows=None):
    """One summation order over the rows of a matrix (all of them by default): the y a kernel using it would write."""
    rows = range(M.rows) if rows is None else rows
    return np.array([order(row_terms(M, i), M.y0[i] if accumulate else None) for i in rows], M.dtype)
