"""Test infrastructure for csr_wavev's equal-length tiles: a numpy restatement of the plan's wave partition and of the kernel's
uniform-tile predicate, and the seeded matrices that tests/test_uniform_tiles_refs.py (CPU) and tests/test_uniform_tiles_gpu.py share.

The partition (csrc/spmv_csr.hip, wave_partition_kernel): with L the longest row and Q = 256 V - L - 3, wave tile t holds the rows
whose FIRST entry lies in [t Q, (t + 1) Q); there are entries // Q + 1 tiles.  The kernel takes a tile of nr rows and
cnt = nz1 - nz0 entries as uniform -- row r of the tile is [nz0 + r L, nz0 + (r + 1) L), no row offset is read -- iff
L > 0 and cnt == nr L.  Every row is at most L long, so the sum reaches nr L only when every row is exactly L long."""
import numpy as np

V_ALL = (1, 2, 4)


def admits(max_len, V):
    """The plan's own rule for csr_wavev: the longest row may take at most half a tile."""
    return 2 * (max_len + 3) <= 256 * V


def partition(Ap, V):
    """(first row, first entry) of every wave tile plus the closing sentinel, as the plan builds them: int64 arrays of tiles + 1."""
    Ap = np.asarray(Ap, np.int64)
    rows, nnz = len(Ap) - 1, int(Ap[-1])
    max_len = int(np.diff(Ap).max()) if rows else 0
    Q = 256 * V - max_len - 3
    assert Q >= 1 and nnz > 0
    tiles = nnz // Q + 1
    row_start = np.searchsorted(Ap[:-1] // Q, np.arange(tiles + 1), side="left")  # (the first entries never decrease)
    row_start[tiles] = rows  # the sentinel row closes every remaining tile
    return row_start, Ap[row_start], max_len, Q


def uniform_mask(Ap, V):
    """Per tile that owns rows: (nr, cnt, nz0, the kernel's predicate)."""
    row_start, nz, max_len, _ = partition(Ap, V)
    nr, cnt = np.diff(row_start), np.diff(nz)
    own = nr > 0
    uni = (max_len > 0) & (cnt == nr * max_len)
    return nr[own], cnt[own], nz[:-1][own], uni[own]


def brute_force_mask(Ap, V):
    """The same by looking at every row of every tile: all rows of the tile have the longest row's length."""
    Ap = np.asarray(Ap, np.int64)
    row_start, _, max_len, _ = partition(Ap, V)
    lens = np.diff(Ap)
    out = []
    for t in range(len(row_start) - 1):
        a, b = int(row_start[t]), int(row_start[t + 1])
        if b > a:
            out.append(bool(max_len > 0 and all(int(n) == max_len for n in lens[a:b])))
    return np.array(out, bool)


def tile_counts(Ap, V):
    """(uniform tiles, other tiles) among the tiles that own rows."""
    uni = uniform_mask(Ap, V)[3]
    return int(uni.sum()), int((~uni).sum())


# ---- the cases -------------------------------------------------------------------------------------------------------------------

def _poisson_lens(nx, ny):
    """Row lengths of the 5-point matrix on an nx x ny grid, x fastest."""
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    n = 1 + (i > 0) + (i < nx - 1) + (j > 0) + (j < ny - 1)
    return n.reshape(-1).astype(np.int64)


def _poisson_cols(nx, ny):
    cols = []
    for j in range(ny):
        for i in range(nx):
            r = j * nx + i
            c = []
            if j > 0: c.append(r - nx)
            if i > 0: c.append(r - 1)
            c.append(r)
            if i < nx - 1: c.append(r + 1)
            if j < ny - 1: c.append(r + nx)
            cols.extend(c)
    return np.array(cols, np.int32)


def _with_empty_runs(body_rows, runs):
    """Rows of 5; `runs` = [(position in the body, number of empty rows)], position 0 = the very start, body_rows = the very end."""
    out, at = [], 0
    for pos, n in sorted(runs):
        out += [5] * (pos - at) + [0] * n
        at = pos
    out += [5] * (body_rows - at)
    return np.array(out, np.int64)


def _lens():
    """name -> (row lengths, what the case claims).  Claims: 'both' = at least 3 uniform and 3 other tiles at every V;
    'uniform' = every tile uniform; 'none' = no tile uniform; 'lookalike' = none uniform, at least 3 tiles with cnt == 5 nr;
    'turns' = every tile uniform and some tile of more than 64 rows; None = nothing beyond predicate == brute force."""
    c = {}
    # the issue's poisson5pt(37, 41): a grid line is 203 entries, shorter than any tile (Q >= 248), so every tile holds a boundary row
    c["poisson5pt_37x41"] = (_poisson_lens(41, 37), "none")
    # ... resized to grid lines of 451 rows (2240 interior entries > 2 Q at V = 4): uniform and boundary tiles interleaved
    c["poisson5pt_9x451"] = (_poisson_lens(451, 9), "both")
    for K in (1, 2, 3):  # more than 64 rows per tile: the later turns of the row loop (3003 rows: several tiles at V = 4 too)
        c[f"equal_{K}"] = (np.full(3003, K, np.int64), "turns")
    for K in (5, 8, 16, 61):
        c[f"equal_{K}"] = (np.full(1001, K, np.int64), "uniform")
    # 5005 entries: odd (f64) and not a multiple of 4 (f32): the arrays' last vector reaches past the end on a uniform tile
    c["equal_5_odd_entries"] = (np.full(1001, 5, np.int64), "uniform")
    c["lookalike_4_6"] = (np.tile(np.array([4, 6], np.int64), 1000), "lookalike")
    one7 = np.full(1001, 5, np.int64); one7[500] = 7
    c["one_row_of_7"] = (one7, "none")
    one3 = np.full(1001, 5, np.int64); one3[500] = 3
    c["one_row_of_3"] = (one3, None)
    c["empty_runs"] = (_with_empty_runs(4000, [(0, 70), (600, 1), (1200, 70), (1800, 1), (2400, 300), (3200, 1), (4000, 300)]), "both")
    c["single_row"] = (np.array([5], np.int64), "uniform")
    c["single_tile"] = (np.full(40, 5, np.int64), "uniform")
    return c


CASES = tuple(_lens().keys())


def structure(name):
    """(Ap int32, Aj int32, columns, claim) of a case: seeded random columns, the real stencil columns for the Poisson cases."""
    lens, claim = _lens()[name]
    Ap = np.r_[0, np.cumsum(lens)].astype(np.int32)
    rows, nnz = len(lens), int(Ap[-1])
    cols = rows + 17
    if name.startswith("poisson5pt_"):
        ny, nx = (int(s) for s in name.split("_")[1].split("x"))
        Aj = _poisson_cols(nx, ny)
    else:
        Aj = np.random.default_rng(7000 + CASES.index(name)).integers(0, cols, size=nnz).astype(np.int32)
    assert len(Aj) == nnz
    return Ap, Aj, cols, claim


def vectors(name, dtype):
    """Seeded (Ax, x, y0, w) of a case in `dtype`: normal deviates, so hardly any product or sum is exact."""
    Ap, _, cols, _ = structure(name)
    rng = np.random.default_rng(9000 + CASES.index(name))
    rows, nnz = len(Ap) - 1, int(Ap[-1])
    return (rng.standard_normal(nnz).astype(dtype), rng.standard_normal(cols).astype(dtype), rng.standard_normal(rows).astype(dtype),
            rng.standard_normal(rows).astype(dtype))
