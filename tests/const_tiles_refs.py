"""Test infrastructure for csr_wavev's CONSTANT tiles: a numpy restatement of the marking and of its keep rule, shared by
tests/test_const_tiles_refs.py (CPU) and tests/test_const_tiles_gpu.py.

The marks (csrc/spmv_csr.hip, wavev_const_scan_kernel) sit on the shift-invariant tiles' table of tests/shift_tiles_refs.py: a tile that table
marks -- nr >= 1 rows of L entries each, L the matrix's longest row, 1..8 -- is CONSTANT iff every row's L values equal the first row's L values
BY BIT PATTERN (the words are compared as integers: +0 and -0 differ, NaNs of equal payload are equal, NaNs of different payload differ).  The
marks are kept iff constant tiles >= 1 and 4 * constant tiles >= the tiles that have entries.  A constant tile's multiply reads L values where
the tile holds nr L: `skipped` counts the entries of the constant tiles, whose stream is never requested."""
import numpy as np

import shift_tiles_refs as sh
import uniform_tiles_refs as ut


def bits(Ax):
    """The values' words as unsigned integers of the same width."""
    Ax = np.ascontiguousarray(Ax)
    return Ax.view({8: np.uint64, 4: np.uint32}[Ax.dtype.itemsize])


def marks(Ap, Aj, Ax, V, marked=None):
    """(constant bool[tiles], tiles that have entries, entries of the constant tiles).  Row by row: within a marked tile every row equals the
    first iff every row but the first equals its predecessor, so one comparison of neighbouring rows and a running count decide all tiles.
    `marked` (the shift table's marks, when the caller has them) saves the pass over the columns."""
    Ap = np.asarray(Ap, np.int64)
    row_start, nz, L, _ = ut.partition(Ap, V)
    tiles = len(nz) - 1
    cnt = np.diff(nz)
    with_entries = int((cnt > 0).sum())
    if marked is None:
        marked = sh.table(Ap, Aj, V)[0]
    const = np.zeros(tiles, bool)
    if not marked.any():
        return const, with_entries, 0
    b = bits(Ax)
    rows = len(Ap) - 1
    full = np.diff(Ap) == L  # rows of L entries: every row of a marked tile is one
    differs = np.ones(rows, bool)  # row r is not (a full row equal to the full row r - 1)
    r = np.flatnonzero(full[1:] & full[:-1]) + 1
    same = np.ones(len(r), bool)
    for k in range(L):
        same &= b[Ap[r] + k] == b[Ap[r - 1] + k]
    differs[r] = ~same
    run = np.concatenate(([0], np.cumsum(differs)))  # run[i] = rows < i that differ from their predecessor
    at = np.flatnonzero(marked)
    a, e = row_start[at], row_start[at + 1]
    const[at] = run[e] - run[a + 1] == 0  # rows a + 1 .. e - 1 all equal their predecessor
    return const, with_entries, int(cnt[const].sum())


def brute_force(Ap, Aj, Ax, V):
    """Constant tiles by comparing every row of every marked tile with the tile's first row, word by word."""
    Ap = np.asarray(Ap, np.int64)
    row_start, _, L, _ = ut.partition(Ap, V)
    marked = sh.brute_force(Ap, Aj, V)
    b = bits(Ax)
    out = []
    for t in range(len(row_start) - 1):
        a, e = int(row_start[t]), int(row_start[t + 1])
        ok = bool(marked[t])
        if ok:
            first = [int(w) for w in b[Ap[a]:Ap[a] + L]]
            ok = all(int(b[Ap[r] + k]) == first[k] for r in range(a, e) for k in range(L))
        out.append(ok)
    return np.array(out, bool)


def keep_rule(constant, with_entries):
    """The plan keeps the marks: at least one constant tile, and at least a quarter of the tiles that have entries."""
    return constant >= 1 and 4 * constant >= with_entries


def kept(Ap, Aj, Ax, V):
    """(the plan keeps the marks, constant tiles): the shift table is kept and the rule above holds."""
    table_kept, _ = sh.kept(Ap, Aj, V)
    const, with_entries, _ = marks(Ap, Aj, Ax, V)
    n = int(const.sum())
    return bool(table_kept and keep_rule(n, with_entries)), n


def mark_bytes(Ap, V):
    """One bit per wave tile, in 32-bit words."""
    tiles = len(ut.partition(Ap, V)[1]) - 1
    return 4 * ((tiles + 31) // 32)


# ---- matrices ---------------------------------------------------------------------------------------------------------------------
def toeplitz(rows, L, dtype, seed=0):
    """(Ap, Aj, columns, first row's values): `rows` rows of L entries at the fixed offsets of shift_tiles_refs, every tile shift-invariant.
    The values are for the caller to lay out."""
    lens, Aj, cols = sh._toeplitz(L, rows=rows)(1)
    Ap = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    first = np.random.default_rng(2700 + 10 * L + seed).standard_normal(L).astype(dtype)
    return Ap, Aj, cols, first


def constant_values(rows, first):
    return np.tile(first, rows)


def tile_rows(Ap, V, t):
    row_start = ut.partition(Ap, V)[0]
    return int(row_start[t]), int(row_start[t + 1])
