"""Test infrastructure for csr_wavev's shift-invariant tiles: a numpy restatement of the marking, of the table and of its keep rule,
the kernel's column formula in the kernel's own unsigned arithmetic, and the seeded matrices that tests/test_shift_tiles_refs.py (CPU)
and tests/test_shift_tiles_gpu.py share.

The table (csrc/spmv_csr.hip, wavev_cols16_scan_kernel) is part of the plan's 16-bit column copy, on the wave partition of
tests/uniform_tiles_refs.py: tile t has the rows [rs, re), the entries [nz0, nz1) and nr = re - rs; L is the matrix's longest row.
Tile t is MARKED iff 1 <= L <= 8, nr >= 1, nz1 - nz0 == nr L (every row L long) and Aj[nz0 + r L + k] == Aj[nz0 + k] + r for every
0 <= r < nr, 0 <= k < L.  shift[t][k] = Aj[nz0 + k] - rs for k < L and 0 above; shift[t][0] = INT32_MIN on an unmarked tile.  The
table is kept iff the copy is granted and marked tiles >= 1/4 of the tiles that have entries.

The multiply forms, for every position q of a marked tile's vectors (they begin at the E-entry boundary at or below nz0 and end at the
one at or above nz1), p = q - nz0 as uint32, r = (p M) >> 16 with M = ceil(65536 / L) and 24-bit multiplies, k = p - r L, and
column = min(uint32(rs + r + shift[t][k & 7]), num_cols - 1)."""
import numpy as np

import cols16_refs as c16
import uniform_tiles_refs as ut

V_ALL = ut.V_ALL
MAX_LEN = 8
UNMARKED = int(np.iinfo(np.int32).min)
U32, U24 = 0xFFFFFFFF, 0xFFFFFF


def div_mul(L):
    return (65536 + L - 1) // L


def table(Ap, Aj, V):
    """(marked bool[tiles], shift int32[tiles][8], tiles that have entries), vectorised over the entries."""
    Aj = np.asarray(Aj, np.int64)
    row_start, nz, L, _ = ut.partition(Ap, V)
    tiles = len(nz) - 1
    nr, cnt = np.diff(row_start), np.diff(nz)
    shift = np.zeros((tiles, 8), np.int32)
    shift[:, 0] = UNMARKED
    marked = np.zeros(tiles, bool)
    if 1 <= L <= MAX_LEN:
        cand = (nr >= 1) & (cnt == nr * L)
        tile = np.repeat(np.arange(tiles), cnt)
        p = np.arange(len(Aj)) - nz[tile]
        r, k = p // L, p % L
        first = np.minimum(nz[tile] + k, len(Aj) - 1)  # (a tile of shorter rows: the index may leave the tile, which is no candidate then)
        off = np.flatnonzero(Aj != Aj[first] + r)
        broken = np.zeros(tiles, bool)
        broken[tile[off]] = True
        marked = cand & ~broken
        at = np.flatnonzero(marked)
        shift[at, 0] = 0
        shift[at[:, None], np.arange(L)[None, :]] = Aj[nz[at][:, None] + np.arange(L)[None, :]] - row_start[at][:, None]
    return marked, shift, int((cnt > 0).sum())


def brute_force(Ap, Aj, V):
    """Marked tiles by walking every row of every tile."""
    Ap = np.asarray(Ap, np.int64)
    row_start, _, L, _ = ut.partition(Ap, V)
    out = []
    for t in range(len(row_start) - 1):
        a, b = int(row_start[t]), int(row_start[t + 1])
        ok = 1 <= L <= MAX_LEN and b > a and all(int(Ap[r + 1] - Ap[r]) == L for r in range(a, b))
        if ok:
            first = [int(c) for c in Aj[Ap[a]:Ap[a] + L]]
            ok = all(int(Aj[Ap[r] + k]) == first[k] + (r - a) for r in range(a, b) for k in range(L))
        out.append(bool(ok))
    return np.array(out, bool)


def kept(Ap, Aj, V):
    """(the plan keeps the table, marked tiles): the copy is granted and at least a quarter of the tiles that have entries are marked."""
    marked, _, with_entries = table(Ap, Aj, V)
    m = int(marked.sum())
    return bool(c16.encode(Ap, Aj, V)[0] and m >= 1 and 4 * m >= with_entries), m


def table_bytes(Ap, V):
    return 32 * (len(ut.partition(Ap, V)[1]) - 1)


def kernel_columns(Ap, Aj, V, E, num_cols):
    """{(tile, position): column} at every position the vectors of a marked tile on the vector path cover (the tile has entries and
    its last vector lies inside the arrays), in the kernel's arithmetic."""
    row_start, nz, L, _ = ut.partition(Ap, V)
    marked, shift, _ = table(Ap, Aj, V)
    nnz, M, out = int(np.asarray(Ap)[-1]), div_mul(max(L, 1)), {}
    for t in np.flatnonzero(marked):
        a, b, rs = int(nz[t]), int(nz[t + 1]), int(row_start[t])
        up = (b + E - 1) // E * E
        if b > a and up <= nnz:
            for q in range(a // E * E, up):
                p = (q - a) & U32
                r = (((p & U24) * (M & U24)) & U32) >> 16
                k = (p - (((r & U24) * L) & U32)) & U32
                col = (rs + r + int(shift[t][k & 7])) & U32
                out[(int(t), q)] = min(col, num_cols - 1)
    return out


# ---- the new cases ---------------------------------------------------------------------------------------------------------------
# name -> builder(V) -> (row lengths, Aj int32, columns), as in cols16_refs

OFFSETS = (7, -3, 0, 12, -9, 4, 1, -5, 9)  # fixed, unsorted; + 9 keeps row 0 inside the matrix


def _toeplitz_cols(rows, offs, first_col=9):
    return (np.repeat(np.arange(rows), len(offs)) + np.tile(np.array(offs), rows) + first_col).astype(np.int32)


def _toeplitz(L, rows=3003, offs=None, first_col=9, cols=None):
    offs = OFFSETS[:L] if offs is None else offs
    lens = np.full(rows, len(offs), np.int64)
    return lambda V: (lens, _toeplitz_cols(rows, offs, first_col), rows + first_col + 13 if cols is None else cols)


NEAR_MISS_ROW = 500


def _near_miss(V):
    """toeplitz rows of 5 with one entry of row 500 -- inside a tile, not its first row, at every V -- moved by one column."""
    lens, Aj, cols = _toeplitz(5, rows=1001)(V)
    Aj = Aj.copy()
    Aj[5 * NEAR_MISS_ROW + 3] += 1
    return lens, Aj, cols


def _uniform_not_shift(V):
    lens = np.full(1001, 5, np.int64)
    return lens, c16._band(lens, 1001, 40, 105), 1001


FAR_NEAR_OFFS = (6, 2, 1, 4, 0)  # the largest first, the smallest last: the positions next to a tile's ends leave x on either side
FAR_NEAR_COLS = 70500


def _far_near(V):
    """1001 x 70500, rows of 5, every tile shift-invariant: even tiles start at column 0 (their first row holds it), odd tiles end
    exactly at the last column (their last row holds it)."""
    lens = np.full(1001, 5, np.int64)
    row_start = ut.partition(c16._ap(lens), V)[0]
    Aj = np.zeros(5005, np.int64)
    for t in range(len(row_start) - 1):
        a, b = int(row_start[t]), int(row_start[t + 1])
        if b > a:
            first = 0 if t % 2 == 0 else FAR_NEAR_COLS - 1 - (b - a - 1) - max(FAR_NEAR_OFFS)
            Aj[5 * a:5 * b] = first + np.repeat(np.arange(b - a), 5) + np.tile(np.array(FAR_NEAR_OFFS), b - a)
    return lens, Aj.astype(np.int32), FAR_NEAR_COLS


def _keep_rule(over):
    """Rows of 5 over 1001 rows: the first m tiles shift-invariant, seeded band columns elsewhere; m = the smallest count with
    4 m >= tiles that have entries (`over`), or one fewer."""
    def make(V):
        lens = np.full(1001, 5, np.int64)
        row_start, nz, _, _ = ut.partition(c16._ap(lens), V)
        with_entries = int((np.diff(nz) > 0).sum())
        m = (with_entries + 3) // 4 - (0 if over else 1)
        Aj = c16._band(lens, 1001, 40, 131).astype(np.int64)
        end = int(row_start[m])
        Aj[:5 * end] = _toeplitz_cols(end, OFFSETS[:5])
        return lens, Aj.astype(np.int32), 1001 + 22
    return make


BUILDERS = {f"toeplitz_{L}": _toeplitz(L) for L in range(1, 9)}
BUILDERS.update({
    "toeplitz_duplicate": _toeplitz(5, offs=(3, -2, 3, 0, 6)),
    "toeplitz_9": _toeplitz(9),
    "near_miss": _near_miss,
    "uniform_not_shift": _uniform_not_shift,
    "far_near": _far_near,
    "shift_60000": _toeplitz(5, first_col=60000, cols=64000),
    "keep_under": _keep_rule(False), "keep_over": _keep_rule(True),
    "ends_odd_entries": _toeplitz(5, rows=1001),  # 5005 entries: the last tile's last vector reaches past the arrays at E = 2 and 4
})
NEW_CASES = tuple(BUILDERS)
ALL_MARKED = tuple(f"toeplitz_{L}" for L in range(1, 9)) + ("toeplitz_duplicate", "far_near", "shift_60000", "ends_odd_entries", "rank_block", "single_row")
NONE_MARKED = ("toeplitz_9", "uniform_not_shift", "poisson5pt_37x41", "equal_1", "equal_2", "equal_3", "unsorted", "empty_runs", "opposite_ends",
               "span_65535", "span_65536", "scattered", "rows_1_16_band_2000", "single_tile_odd_entries")
NOT_KEPT = NONE_MARKED + ("keep_under",)
CASES = c16.CASES + NEW_CASES


def structure(name, V):
    """(Ap int32, Aj int32, columns) of a case of cols16_refs or of a new one."""
    if name in c16.BUILDERS:
        return c16.structure(name, V)
    lens, Aj, cols = BUILDERS[name](V)
    Ap = c16._ap(lens)
    assert len(Aj) == int(Ap[-1]) and Aj.dtype == np.int32 and Aj.min() >= 0 and Aj.max() < cols
    return Ap, Aj, cols


def vectors(name, V, dtype):
    """Seeded (Ax, x, y0, w) of a case in `dtype`: normal deviates, so hardly any product or sum is exact."""
    if name in c16.BUILDERS:
        return c16.vectors(name, V, dtype)
    Ap, _, cols = structure(name, V)
    rng = np.random.default_rng(13000 + NEW_CASES.index(name))
    rows, nnz = len(Ap) - 1, int(Ap[-1])
    return (rng.standard_normal(nnz).astype(dtype), rng.standard_normal(cols).astype(dtype), rng.standard_normal(rows).astype(dtype),
            rng.standard_normal(rows).astype(dtype))
