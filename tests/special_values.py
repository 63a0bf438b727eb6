"""IEEE special values for the multiply tests: a bit-level comparison, the reference's host loops restated as plain Python
loops (with four deliberately wrong variants), five small matrices and five input decks per matrix.

Plain module: no fixtures, no GPU.  tests/test_special_values_refs.py proves on the CPU that every deck meets the floor
counts stated below and that every mutant loop is caught by the deck meant for it; tests/test_special_values_gpu.py runs
the decks through every kernel.

The NaN set J of the two near-miss decks is {0, cols-1, cols-2} on every matrix.  On `runs` it also holds the columns
right and left of the dedicated near-miss pieces; on the other four matrices it also holds every 41st column (j % 41 ==
20), because three columns alone cannot give 50 NaN rows and 50 finite neighbours on a stencil.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DTYPES = (np.float64, np.float32)
DECKS = ("nan_near_miss", "inf_near_miss", "signed_zeros", "subnormals", "overflow_order")
FINITE_DECKS = ("signed_zeros", "subnormals")
MUTANTS = ("start_at_first_product", "zero_times_padding", "pairwise", "flush_subnormals")


# ------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------
def _uint(a):
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def bits_differ(got, want):
    """Boolean array: where `got` and `want` differ as same_bits counts it (NaN against NaN is equal whatever the sign
    and payload; everything else by bit pattern)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype
    gn, wn = np.isnan(got), np.isnan(want)
    return (gn != wn) | (~gn & ~wn & (_uint(np.ascontiguousarray(got)) != _uint(np.ascontiguousarray(want))))


def same_bits(got, want, what=""):
    """Assert that two float arrays hold the same values bit for bit: equal shape and dtype, NaNs at the same positions
    (sign and payload of a NaN are not compared: x86 and gfx950 produce different default NaNs), equal unsigned-integer
    views everywhere else -- so -0.0 differs from +0.0 and a subnormal from 0."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype, f"{what}: dtype {got.dtype} against {want.dtype}"
    assert got.shape == want.shape, f"{what}: shape {got.shape} against {want.shape}"
    assert got.dtype.kind == "f", f"{what}: not a float array ({got.dtype})"
    bad = bits_differ(got, want)
    if bad.any():
        g, w = _uint(np.ascontiguousarray(got)), _uint(np.ascontiguousarray(want))
        digits = 2 * got.dtype.itemsize
        where = np.argwhere(bad)[:6]
        lines = [f"  {tuple(int(i) for i in p)}: got {got[tuple(p)]!r} 0x{int(g[tuple(p)]):0{digits}x}, "
                 f"want {want[tuple(p)]!r} 0x{int(w[tuple(p)]):0{digits}x}" for p in where]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ in their bits\n" + "\n".join(lines))


# ------------------------------------------------------------------------------------------------
# the reference's host loops, one rounding per operation, in the matrix's own type
# ------------------------------------------------------------------------------------------------
def _flush(v, tiny):
    return v * type(v)(0) if abs(v) < tiny else v   # a zero with v's sign (v is never NaN or inf where this is used)


def _pieces(cols_of_row, cap=4):
    """Cut a row's columns into pieces of consecutive columns, at most `cap` long: (first index, length) pairs."""
    out, k, n = [], 0, len(cols_of_row)
    while k < n:
        m = 1
        while m < cap and k + m < n and cols_of_row[k + m] == cols_of_row[k] + m:
            m += 1
        out.append((k, m))
        k += m
    return out


def _chain(start, prods, mutant, tiny):
    """Add `prods` to `start` (None: the sum starts at zero) the way the reference does, or the way `mutant` does."""
    T = prods.dtype.type
    if mutant == "pairwise":
        s = [T(0) if start is None else start, T(0)]
        for k, p in enumerate(prods):
            s[k & 1] = s[k & 1] + p
        return s[0] + s[1]
    if mutant == "start_at_first_product" and start is None and len(prods):
        acc, prods = prods[0], prods[1:]
    else:
        acc = T(0) if start is None else start
    if mutant == "flush_subnormals":
        for p in prods:
            acc = _flush(acc + _flush(p, tiny), tiny)
        return acc
    for p in prods:
        acc = acc + p
    return acc


def loop_spmv_csr(Ap, Aj, Ax, x, y0=None, accumulate=False, mutant=None):
    """acc = 0 (or y0[i]); acc = acc + Ax[jj] * x[Aj[jj]] in storage order.  mutant zero_times_padding: behind every piece
    of fewer than 4 consecutive columns the next column of x is multiplied by a zero value and added."""
    T = Ax.dtype.type
    rows, cols, tiny = len(Ap) - 1, len(x), np.finfo(Ax.dtype).tiny
    y = np.empty(rows, Ax.dtype)
    with np.errstate(all="ignore"):
        prod = Ax * x[Aj]
        for i in range(rows):
            s, e = int(Ap[i]), int(Ap[i + 1])
            p = prod[s:e]
            if mutant == "zero_times_padding":
                c, q = Aj[s:e], []
                for k, m in _pieces(c):
                    q.extend(p[k:k + m])
                    if m < 4:
                        q.append(T(0) * x[min(int(c[k]) + m, cols - 1)])
                p = np.array(q, Ax.dtype)
            y[i] = _chain(y0[i] if accumulate else None, p, mutant, tiny)
    return y


def loop_spmv_ell(rows, width, pitch, eAj, eAx, x, y0=None, accumulate=False, mutant=None):
    """Per row the slots n = 0 .. width-1 at n * pitch + i; a slot with column -1 is skipped.  mutant zero_times_padding:
    it gathers x[0] and multiplies it by the slot's value (zero) instead."""
    tiny = np.finfo(eAx.dtype).tiny
    y = np.empty(rows, eAx.dtype)
    J = eAj.reshape(width, pitch)[:, :rows] if width else np.zeros((0, rows), np.int32)
    V = eAx.reshape(width, pitch)[:, :rows] if width else np.zeros((0, rows), eAx.dtype)
    with np.errstate(all="ignore"):
        P = V * x[np.maximum(J, 0)]
        for i in range(rows):
            p = P[:, i] if mutant == "zero_times_padding" else P[J[:, i] != -1, i]
            y[i] = _chain(y0[i] if accumulate else None, p, mutant, tiny)
    return y


def loop_spmv_dia(rows, cols, pitch, offsets, vals, x, y0=None, accumulate=False):
    """Per row the diagonals in order; every slot whose column row + offset lies in [0, cols) is multiplied, explicit zeros
    included."""
    T = vals.dtype.type
    y = np.empty(rows, vals.dtype)
    V = vals.reshape(len(offsets), pitch)
    with np.errstate(all="ignore"):
        for i in range(rows):
            acc = y0[i] if accumulate else T(0)
            for d, k in enumerate(offsets):
                j = i + int(k)
                if 0 <= j < cols:
                    acc = acc + V[d, i] * x[j]
            y[i] = acc
    return y


def loop_spmv_coo(rows, Ai, Aj, Ax, x, y0=None, accumulate=False):
    """y = 0 (or y0); y[Ai[n]] = y[Ai[n]] + Ax[n] * x[Aj[n]] in entry order."""
    y = np.array(y0, Ax.dtype) if accumulate else np.zeros(rows, Ax.dtype)
    with np.errstate(all="ignore"):
        prod = Ax * x[Aj]
        for n in range(len(Ax)):
            y[Ai[n]] = y[Ai[n]] + prod[n]
    return y


def loop_spmv_hyb(rows, width, pitch, eAj, eAx, cAi, cAj, cAx, x, y0=None, accumulate=False, mutant=None):
    """The ELL part with the caller's start, then the COO part added on top."""
    y = loop_spmv_ell(rows, width, pitch, eAj, eAx, x, y0, accumulate, mutant)
    return loop_spmv_coo(rows, cAi, cAj, cAx, x, y, True)


# ------------------------------------------------------------------------------------------------
# matrices (structure only; the decks give the values)
# ------------------------------------------------------------------------------------------------
class Matrix:
    def __init__(self, name, rows, cols, Ap, Aj, **extra):
        self.name, self.rows, self.cols = name, int(rows), int(cols)
        self.Ap, self.Aj = np.ascontiguousarray(Ap, np.int32), np.ascontiguousarray(Aj, np.int32)
        self.nnz = len(self.Aj)
        self.Ai = np.repeat(np.arange(self.rows, dtype=np.int32), np.diff(self.Ap))
        self.near_miss_rows = extra.pop("near_miss_rows", np.zeros(0, np.int64))
        self.near_miss_cols = extra.pop("near_miss_cols", np.zeros(0, np.int64))
        self.__dict__.update(extra)

    def row_lengths(self):
        return np.diff(self.Ap)


def _from_rows(name, rows, cols, row_cols, **extra):
    lens = np.array([len(r) for r in row_cols], np.int64)
    Ap = np.r_[0, np.cumsum(lens)]
    Aj = np.concatenate([np.asarray(r, np.int64) for r in row_cols]) if lens.sum() else np.zeros(0, np.int64)
    assert Aj.min() >= 0 and Aj.max() < cols
    return Matrix(name, rows, cols, Ap, Aj, **extra)


def _poisson(m, n):
    r = np.arange(m * n)
    ix, iy = r % m, r // m
    cand = np.stack([r - m, r - 1, r, r + 1, r + m], 1)
    keep = np.stack([iy > 0, ix > 0, np.ones_like(r, bool), ix < m - 1, iy < n - 1], 1)
    return _from_rows("poisson100", m * n, m * n, [c[k] for c, k in zip(cand, keep)])


def _banded():
    g = np.load(os.path.join(GOLDEN, "banded_700x900_dia.npz"))
    rows, cols, off = int(g["rows"]), int(g["cols"]), g["offsets"].astype(np.int64)
    row_cols = [[i + k for k in off if 0 <= i + k < cols] for i in range(rows)]
    return _from_rows("banded", rows, cols, row_cols, dia_offsets=g["offsets"].astype(np.int32), dia_pitch=int(g["pitch"]))


RUNS_ROWS, RUNS_COLS = 2000, 2003
_NM_BASE, _NM_STRIDE, _NM_COUNT = 1000, 8, 100       # dedicated column blocks [1000 + 8 k, +8) of the near-miss rows
_A_LO, _A_HI, _C_LO, _C_HI = 3, 990, 1810, 1990       # where ordinary runs live; [1995, 2003) belongs to the edge rows


def _random_runs(rng, lo, hi, count):
    """`count` entries in [lo, hi) as ascending runs of 1..4 consecutive columns with at least one column between runs."""
    out, c = [], lo + int(rng.integers(0, 40))
    while count > 0 and c + 4 < hi:
        m = min(int(rng.integers(1, 5)), count)
        out.extend(range(c, c + m))
        count -= m
        c += m + 1 + int(rng.integers(1, 30))
    return out


def _runs():
    """2000 x 2003, rows of 24..60 entries in column runs of 1..4, every 97th row empty.  Row r with r % 20 == 3 is near-miss
    row k = r // 20: besides its ordinary runs it holds ONE single column B + 1 and ONE run B + 4 .. B + 6 in its own block
    B = 1000 + 8 k, which no other row touches -- so B, B + 2, B + 3 and B + 7 are columns that only an over-fetch reads.
    Rows with r % 100 == 57: a piece ending at cols - 1 - (k % 4), of length 1 + (k // 4) % 4 (k = r // 100).  Rows with
    r % 20 == 11 start at column 1, those with r % 20 == 12 at column 0."""
    rng = np.random.default_rng(20250)
    row_cols, nm_rows, nm_cols = [], [], []
    for r in range(RUNS_ROWS):
        if r % 97 == 0:
            row_cols.append([])
            continue
        n = int(rng.integers(24, 61))
        head, mid, tail = [], [], []
        if r % 20 == 3 and r // 20 < _NM_COUNT:
            B = _NM_BASE + _NM_STRIDE * (r // 20)
            mid = [B + 1, B + 4, B + 5, B + 6]
            nm_rows.append(r)
            nm_cols += [B, B + 2, B + 3, B + 7]
        elif r % 100 == 57:
            k = r // 100
            end, m = RUNS_COLS - 1 - (k % 4), 1 + (k // 4) % 4
            tail = list(range(end - m + 1, end + 1))
        elif r % 20 == 11:
            head = [1]
        elif r % 20 == 12:
            head = [0, 1]
        n -= len(head) + len(mid) + len(tail)
        na = n // 2
        row_cols.append(head + _random_runs(rng, _A_LO, _A_HI, na) + mid + _random_runs(rng, _C_LO, _C_HI, n - na) + tail)
    return _from_rows("runs", RUNS_ROWS, RUNS_COLS, row_cols, near_miss_rows=np.array(nm_rows), near_miss_cols=np.array(nm_cols))


def _band():
    """4096 x 4096, 16..40 entries per row anywhere within +-1500 of the diagonal (ascending, distinct)."""
    rng = np.random.default_rng(4096)
    n, row_cols = 4096, []
    for r in range(n):
        lo, hi = max(0, r - 1500), min(n, r + 1501)
        row_cols.append(np.sort(rng.choice(np.arange(lo, hi), size=int(rng.integers(16, 41)), replace=False)))
    return _from_rows("band", n, n, row_cols)


def _irregular(dtype):
    g = np.load(os.path.join(GOLDEN, "irregular_1500x1237.npz"))
    p = "f64" if np.dtype(dtype) == np.float64 else "f32"
    return Matrix("irregular", int(g["rows"]), int(g["cols"]), g[p + "_Ap"], g[p + "_Aj"])


_matrix_cache = {}


def matrices(dtype):
    """name -> Matrix.  Only `irregular` depends on the type (the fixture holds one structure per type)."""
    key = np.dtype(dtype).name
    if key not in _matrix_cache:
        if "shared" not in _matrix_cache:
            _matrix_cache["shared"] = {"poisson100": _poisson(100, 100), "banded": _banded(), "runs": _runs(), "band": _band()}
        _matrix_cache[key] = dict(_matrix_cache["shared"], irregular=_irregular(dtype))
    return _matrix_cache[key]


def without_long_rows(M, limit):
    """M with every row of `limit` or more entries emptied (the wave-tile kernels refuse such rows)."""
    lens = M.row_lengths()
    keep = np.repeat(lens < limit, lens)
    return Matrix(M.name + "_short", M.rows, M.cols, np.r_[0, np.cumsum(np.where(lens < limit, lens, 0))], M.Aj[keep])


# ------------------------------------------------------------------------------------------------
# decks
# ------------------------------------------------------------------------------------------------
def nan_columns(M):
    """The set J of the near-miss decks (see the module docstring)."""
    J = {0, M.cols - 1, M.cols - 2}
    if M.name.startswith("runs"):
        J.update(int(c) for c in M.near_miss_cols)
    else:
        J.update(range(20, M.cols, 41))
    return np.array(sorted(J), np.int64)


def _ordinary(M, dtype, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(M.nnz).astype(dtype), rng.standard_normal(M.cols).astype(dtype),
            rng.standard_normal(M.rows).astype(dtype))


def _within(M):
    return np.arange(M.nnz) - np.repeat(M.Ap[:-1].astype(np.int64), M.row_lengths())


def decks(M, dtype):
    """name -> (Ax, x, y0) for matrix M, seeded."""
    dtype = np.dtype(dtype)
    T, fi = dtype.type, np.finfo(dtype)
    seed = sum(map(ord, M.name)) * 7 + dtype.itemsize
    J = nan_columns(M)
    out = {}

    Ax, x, y0 = _ordinary(M, dtype, seed + 1)
    x[J] = np.nan
    out["nan_near_miss"] = (Ax, x, y0)

    Ax, x, y0 = _ordinary(M, dtype, seed + 2)
    x[J] = np.where(np.arange(len(J)) % 2 == 0, np.inf, -np.inf)
    hit = np.flatnonzero(np.isin(M.Aj, J))
    Ax[hit[::3]] = 0.0                                   # 0 * inf = NaN in the reference itself
    out["inf_near_miss"] = (Ax, x, y0)

    rng = np.random.default_rng(seed + 3)
    mag = (0.5 + rng.random(M.nnz)).astype(dtype)
    group = np.repeat((np.arange(M.rows) // 3) % 3, M.row_lengths())   # 0: products all -0.0, 1: all +0.0, 2: mixed
    sign = np.where(group == 0, 1.0, np.where(group == 1, -1.0, np.where(_within(M) % 2 == 0, 1.0, -1.0)))
    out["signed_zeros"] = ((mag * sign).astype(dtype), np.full(M.cols, -0.0, dtype),
                           np.array([-0.0, 0.0, -1.5], dtype)[np.arange(M.rows) % 3])

    rng = np.random.default_rng(seed + 4)
    f = T(2.0) ** (-70 if dtype == np.float32 else -520)
    odd = lambda n: (2 * rng.integers(0, 4, size=n) + 1).astype(dtype)  # noqa: E731
    out["subnormals"] = (odd(M.nnz) * f, odd(M.cols) * f, odd(M.rows) * f * f)

    Ax, _, y0 = _ordinary(M, dtype, seed + 5)
    rng = np.random.default_rng(seed + 6)
    x = rng.choice(np.array([1, -1, 2, -2, 4, -4], dtype), size=M.cols)
    B = T(0.75) * fi.max
    w = _within(M)
    first4 = (w < 4) & np.repeat(M.row_lengths() >= 4, M.row_lengths())
    Ax[first4] = (np.where(w[first4] < 2, B, -B) / x[M.Aj[first4]]).astype(dtype)
    out["overflow_order"] = (Ax, x, y0)
    return out
