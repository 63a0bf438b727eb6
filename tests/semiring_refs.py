"""The semiring multiply restated: cusp::multiply(A, x, y, initialize, combine, reduce) for the named functors, as plain Python loops
over numpy scalars of the matrix's type (one rounding per operation), in each format's own order -- what cusp::detail::host_multiply
does and what cmi_spmv_*_semiring_* must reproduce bit for bit.  Seven deliberately wrong variants (MUTANTS), the format conversions
the tests need, and the decks.

Plain module: no fixtures, no GPU.  tests/test_semiring_refs.py proves on the CPU that the loops are exact arithmetic / plain
selection where that is defined and that every mutant is caught by the deck meant for it.

    s = y0[i] (y0 given) or init;   for each entry of row i in the format's own order:   s = reduce(s, combine(A_ij, x_j));   y[i] = s
"""
import numpy as np

import special_values as sv

COMBINES = ("plus", "multiplies", "minimum", "maximum", "project1st", "project2nd")
REDUCES = ("plus", "multiplies", "minimum", "maximum")
PAIRS = tuple((c, r) for c in COMBINES for r in REDUCES)
OP_CODE = {n: k for k, n in enumerate(COMBINES)}     # the values of cmi_op
MUTANTS = ("fmin_fmax", "tie_keeps_first", "reversed_chain", "start_at_first_term", "ell_padding_takes_part", "dia_skips_stored_zeros",
           "hyb_coo_reinitialises")


# ------------------------------------------------------------------------------------------------
# the operations, on numpy scalars
# ------------------------------------------------------------------------------------------------
def _operations(mutant=None):
    if mutant == "fmin_fmax":
        lo, hi = (lambda a, b: np.fmin(a, b)), (lambda a, b: np.fmax(a, b))
    elif mutant == "tie_keeps_first":
        lo, hi = (lambda a, b: a if a <= b else b), (lambda a, b: b if a <= b else a)
    else:
        lo, hi = (lambda a, b: a if a < b else b), (lambda a, b: b if a < b else a)
    return {"plus": lambda a, b: a + b, "multiplies": lambda a, b: a * b, "minimum": lo, "maximum": hi, "project1st": lambda a, b: a,
            "project2nd": lambda a, b: b}


def _chain(start, terms, combine, reduce, mutant):
    """`terms`: the row's (matrix value, vector value) pairs in the format's own order."""
    ops = _operations(mutant)
    comb, red = ops[combine], ops[reduce]
    if mutant == "reversed_chain":
        terms = terms[::-1]
    t = [comb(a, b) for a, b in terms]
    if mutant == "start_at_first_term" and t:
        s, t = t[0], t[1:]
    else:
        s = start
    for p in t:
        s = red(s, p)
    return s


def _type(*arrays):
    return next(a for a in arrays if a is not None).dtype.type


def _run(rows_terms, T, combine, reduce, y0, init, mutant):
    y = np.empty(len(rows_terms), np.dtype(T))
    with np.errstate(all="ignore"):
        for i, terms in enumerate(rows_terms):
            y[i] = _chain(T(y0[i]) if y0 is not None else T(init), terms, combine, reduce, mutant)
    return y


def _pair(T, Ax, x, e, j):
    """(matrix value, vector value) of one entry; a stream that is not there (None: the operations do not read it) stands as zero."""
    return (Ax[e] if Ax is not None else T(0), x[j] if x is not None else T(0))


# ------------------------------------------------------------------------------------------------
# the five loops
# ------------------------------------------------------------------------------------------------
def terms_csr(Ap, Aj, Ax, x):
    T = _type(Ax, x)
    return [[_pair(T, Ax, x, e, Aj[e] if Aj is not None else 0) for e in range(int(Ap[i]), int(Ap[i + 1]))] for i in range(len(Ap) - 1)]


def terms_coo(rows, Ai, Aj, Ax, x):
    """Entry order: y[Ai[n]] = reduce(y[Ai[n]], ...) for n ascending is, per row, the row's entries in storage order."""
    T = _type(Ax, x)
    out = [[] for _ in range(rows)]
    for n in range(len(Ai)):
        out[int(Ai[n])].append(_pair(T, Ax, x, n, Aj[n] if Aj is not None else 0))
    return out


def terms_ell(rows, width, pitch, eAj, eAx, x, mutant=None):
    """Slots ascending at n * pitch + i; a slot with column -1 is skipped.  mutant ell_padding_takes_part: it takes part with its stored value
    and x[0]."""
    T = _type(eAx, x)
    out = []
    for i in range(rows):
        terms = []
        for n in range(width):
            j = int(eAj[n * pitch + i])
            if j != -1:
                terms.append(_pair(T, eAx, x, n * pitch + i, j))
            elif mutant == "ell_padding_takes_part":
                terms.append(_pair(T, eAx, x, n * pitch + i, 0))
        out.append(terms)
    return out


def terms_dia(rows, cols, pitch, offsets, vals, x, mutant=None):
    """Diagonals in storage order; every slot whose column i + offset lies in [0, cols) takes part, stored zeros included.  mutant
    dia_skips_stored_zeros: a slot whose value compares equal to zero is left out."""
    T = _type(vals, x)
    out = []
    for i in range(rows):
        terms = []
        for d, k in enumerate(offsets):
            j = i + int(k)
            if 0 <= j < cols:
                if mutant == "dia_skips_stored_zeros" and vals is not None and vals[d * pitch + i] == 0:
                    continue
                terms.append(_pair(T, vals, x, d * pitch + i, j))
        out.append(terms)
    return out


def semiring_csr(Ap, Aj, Ax, x, combine, reduce, y0=None, init=0.0, mutant=None):
    return _run(terms_csr(Ap, Aj, Ax, x), _type(Ax, x), combine, reduce, y0, init, mutant)


def semiring_coo(rows, Ai, Aj, Ax, x, combine, reduce, y0=None, init=0.0, mutant=None):
    return _run(terms_coo(rows, Ai, Aj, Ax, x), _type(Ax, x), combine, reduce, y0, init, mutant)


def semiring_ell(rows, width, pitch, eAj, eAx, x, combine, reduce, y0=None, init=0.0, mutant=None):
    return _run(terms_ell(rows, width, pitch, eAj, eAx, x, mutant), _type(eAx, x), combine, reduce, y0, init, mutant)


def semiring_dia(rows, cols, pitch, offsets, vals, x, combine, reduce, y0=None, init=0.0, mutant=None):
    return _run(terms_dia(rows, cols, pitch, offsets, vals, x, mutant), _type(vals, x), combine, reduce, y0, init, mutant)


def semiring_hyb(rows, width, pitch, eAj, eAx, cAi, cAj, cAx, x, combine, reduce, y0=None, init=0.0, mutant=None):
    """The ELL part with the caller's start, then the COO part with identity as its initialise.  mutant hyb_coo_reinitialises: the COO part
    applies the caller's initialise again."""
    y = semiring_ell(rows, width, pitch, eAj, eAx, x, combine, reduce, y0, init, mutant)
    if mutant == "hyb_coo_reinitialises":
        return semiring_coo(rows, cAi, cAj, cAx, x, combine, reduce, y0, init, mutant)
    return semiring_coo(rows, cAi, cAj, cAx, x, combine, reduce, y, 0.0, mutant)


# ------------------------------------------------------------------------------------------------
# conversions (test infrastructure; the chains per row stay those of the CSR storage order)
# ------------------------------------------------------------------------------------------------
def ell_pitch(rows):
    return (rows + 15) // 16 * 16


def csr_to_coo(Ap):
    return np.repeat(np.arange(len(Ap) - 1, dtype=np.int32), np.diff(Ap))


def csr_to_ell(Ap, Aj, Ax, width=None):
    """(width, pitch, eAj, eAx): column-major, padding column -1 and value 0.  width below the longest row drops the rest (HYB's ELL part)."""
    rows, lens = len(Ap) - 1, np.diff(Ap)
    width = int(lens.max()) if width is None and rows else int(width or 0)
    pitch = ell_pitch(rows)
    eAj, eAx = np.full(width * pitch, -1, np.int32), np.zeros(width * pitch, Ax.dtype)
    for i in range(rows):
        n = min(int(lens[i]), width)
        s = int(Ap[i])
        eAj[np.arange(n) * pitch + i] = Aj[s:s + n]
        eAx[np.arange(n) * pitch + i] = Ax[s:s + n]
    return width, pitch, eAj, eAx


def csr_to_hyb(Ap, Aj, Ax, width):
    """(width, pitch, eAj, eAx, cAi, cAj, cAx): the first `width` entries of every row in the ELL part, the rest in the COO part."""
    _, pitch, eAj, eAx = csr_to_ell(Ap, Aj, Ax, width)
    within = np.arange(len(Aj)) - np.repeat(Ap[:-1].astype(np.int64), np.diff(Ap))
    rest = within >= width
    return width, pitch, eAj, eAx, csr_to_coo(Ap)[rest], Aj[rest], Ax[rest]


def csr_to_dia(rows, cols, Ap, Aj, Ax, offsets, pitch):
    """Values on the given diagonals (every entry must lie on one of them, once); slots without an entry hold zero."""
    vals = np.zeros(len(offsets) * pitch, Ax.dtype)
    where = {int(k): d for d, k in enumerate(offsets)}
    Ai = csr_to_coo(Ap)
    for e in range(len(Aj)):
        vals[where[int(Aj[e]) - int(Ai[e])] * pitch + int(Ai[e])] = Ax[e]
    return vals


# ------------------------------------------------------------------------------------------------
# matrices and decks: name -> (Ax, x, y0) for a special_values.Matrix
# ------------------------------------------------------------------------------------------------
ELL_MAX_WIDTH = 64
_matrices = {}


def matrices(dtype):
    """special_values' matrices plus `irregular_short`: `irregular` without its rows of more than ELL_MAX_WIDTH entries (one has 5000), the
    matrix whose ELL form the tests use."""
    key = np.dtype(dtype).name
    if key not in _matrices:
        m = dict(sv.matrices(dtype))
        m["irregular_short"] = sv.without_long_rows(m["irregular"], ELL_MAX_WIDTH + 1)
        _matrices[key] = m
    return _matrices[key]


def hyb_width(M):
    """Where the tests split a matrix into ELL and COO parts, so that both parts have entries: the mean row length rounded up, or -- where
    that reaches the longest row (`banded`: rows of 6 to 8, mean 7.8) -- two below the longest row."""
    longest = int(M.row_lengths().max()) if M.rows else 0
    width = max(1, int(np.ceil(M.nnz / max(M.rows, 1))))
    return width if width < longest else max(1, longest - 2)


def hyb_parts(M, width=None):
    """(entries in the ELL part, entries in the COO part) of the split at `width` (default hyb_width)."""
    width = hyb_width(M) if width is None else width
    lens = M.row_lengths()
    return int(np.minimum(lens, width).sum()), int(np.maximum(lens - width, 0).sum())


DECKS = ("nan_positions", "zero_ties", "stored_zeros", "ordinary")
INITS = (np.inf, -np.inf, np.nan, 2.5, 0.0)        # constants the tests start chains from (+-inf: the identities of minimum / maximum)


def nan_rows(M):
    """row -> which of its entries has a NaN in x: 0 first, 1 middle, 2 last (rows of at least three entries, every 40th triple)."""
    lens = M.row_lengths()
    return {r: (r % 40) // 2 for r in range(M.rows) if r % 40 in (1, 3, 5) and lens[r] >= 3}


def decks(M, dtype):
    dtype = np.dtype(dtype)
    seed = sum(map(ord, M.name)) * 11 + dtype.itemsize
    out = {}

    rng = np.random.default_rng(seed)
    Ax, x, y0 = (rng.standard_normal(n).astype(dtype) for n in (M.nnz, M.cols, M.rows))
    out["ordinary"] = (Ax, x, y0)

    # NaNs in x at the first, the middle and the last entry of some rows
    rng = np.random.default_rng(seed + 1)
    Ax, x, y0 = (rng.standard_normal(n).astype(dtype) for n in (M.nnz, M.cols, M.rows))
    for r, pos in nan_rows(M).items():
        s, e = int(M.Ap[r]), int(M.Ap[r + 1])
        x[M.Aj[(s, (s + e - 1) // 2, e - 1)[pos]]] = np.nan
    out["nan_positions"] = (Ax, x, y0)

    # +0.0 / -0.0 ties in both orders: neighbouring columns of x hold zeros of opposite sign, the values change sign along a row
    rng = np.random.default_rng(seed + 2)
    mag = (0.5 + rng.random(M.nnz)).astype(dtype)
    within = np.arange(M.nnz) - np.repeat(M.Ap[:-1].astype(np.int64), M.row_lengths())
    flip = np.repeat(np.arange(M.rows) % 2, M.row_lengths())
    Ax = (mag * np.where((within + flip) % 2 == 0, 1.0, -1.0)).astype(dtype)
    x = np.where(np.arange(M.cols) % 2 == 0, 0.0, -0.0).astype(dtype)
    out["zero_ties"] = (Ax, x, np.array([-0.0, 0.0, -1.5, 1.5], dtype)[np.arange(M.rows) % 4])

    # stored zeros: every third entry holds an exact zero (of either sign); in DIA form they sit on in-range diagonals
    rng = np.random.default_rng(seed + 3)
    Ax, x, y0 = (rng.standard_normal(n).astype(dtype) for n in (M.nnz, M.cols, M.rows))
    Ax[::3] = 0.0
    Ax[3::6] = -0.0
    out["stored_zeros"] = (Ax, x, y0)
    return out


def small_integers(M, dtype, seed=5):
    """A deck on which plus and multiplies never round: values and x in {-2, -1, 1, 2} (rows of at most 40 entries: |product chain| < 2^41)."""
    rng = np.random.default_rng(seed)
    pick = np.array([-2, -1, 1, 2], np.dtype(dtype))
    return rng.choice(pick, M.nnz), rng.choice(pick, M.cols), rng.choice(pick, M.rows)


def same_bits(got, want, what=""):
    sv.same_bits(got, want, what)
