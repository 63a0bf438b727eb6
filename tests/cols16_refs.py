"""Test infrastructure for csr_wavev's plan-owned 16-bit column copy: a numpy restatement of the encoding and of its grant rule, and
the seeded matrices that tests/test_cols16_refs.py (CPU) and tests/test_cols16_gpu.py share.

The copy (csrc/spmv_csr.hip, wavev_cols16_build): on the wave partition of tests/uniform_tiles_refs.py -- tile t holds the entries
[nz[t], nz[t + 1]) -- base[t] is the smallest column among the tile's entries (0 for a tile without entries) and
cols16[e] = Aj[e] - base[tile of e] as uint16.  All or nothing: granted iff every tile has max - min <= 65535 (and no column is
negative).  The multiply forms column = min(base[t] + cols16[p], num_cols - 1) for every position p of tile t's vectors, which
begin at the E-entry boundary at or below nz[t] and end at the one at or above nz[t + 1] (E = 2 for f64, 4 for f32): up to E - 1
positions at either end belong to a neighbouring tile and were encoded against ITS base."""
import numpy as np

import uniform_tiles_refs as ut

V_ALL = ut.V_ALL
LIMIT = 65535


def tile_of_entry(Ap, V):
    """(tile of every entry, first entry per tile + sentinel, number of tiles)."""
    _, nz, _, _ = ut.partition(Ap, V)
    nnz = int(np.asarray(Ap)[-1])
    return np.searchsorted(nz[1:], np.arange(nnz), side="right"), nz, len(nz) - 1


def encode(Ap, Aj, V):
    """(granted, base int64[tiles], span int64[tiles] (-1: no entry), cols16 uint16[nnz] or None when refused)."""
    Aj = np.asarray(Aj, np.int64)
    tile, _, tiles = tile_of_entry(Ap, V)
    lo = np.full(tiles, np.iinfo(np.int64).max)
    hi = np.full(tiles, np.iinfo(np.int64).min)
    np.minimum.at(lo, tile, Aj)
    np.maximum.at(hi, tile, Aj)
    has = hi >= lo
    base = np.where(has, lo, 0)
    span = np.where(has, hi - lo, -1)
    granted = bool((span <= LIMIT).all() and (Aj.size == 0 or Aj.min() >= 0))
    return granted, base, span, ((Aj - base[tile]).astype(np.uint16) if granted else None)


def decode(Ap, V, base, cols16):
    tile, _, _ = tile_of_entry(Ap, V)
    return base[tile] + cols16.astype(np.int64)


def brute_force(Ap, Aj, V):
    """(granted, base, span) by walking the rows of every tile."""
    Ap = np.asarray(Ap, np.int64)
    row_start, _, _, _ = ut.partition(Ap, V)
    base, span = [], []
    for t in range(len(row_start) - 1):
        cols = [int(Aj[e]) for r in range(int(row_start[t]), int(row_start[t + 1])) for e in range(int(Ap[r]), int(Ap[r + 1]))]
        base.append(min(cols) if cols else 0)
        span.append(max(cols) - min(cols) if cols else -1)
    return all(s <= LIMIT for s in span) and all(int(c) >= 0 for c in Aj), np.array(base, np.int64), np.array(span, np.int64)


def foreign_positions(Ap, V, E):
    """Positions the kernel's vectors of tile t cover outside [nz[t], nz[t + 1]): [(tile, position)], for the tiles that take the
    vector path (entries, and the last vector inside the arrays)."""
    _, nz, tiles = tile_of_entry(Ap, V)
    nnz = int(np.asarray(Ap)[-1])
    out = []
    for t in range(tiles):
        a, b = int(nz[t]), int(nz[t + 1])
        up = (b + E - 1) // E * E
        if b > a and up <= nnz:
            out += [(t, p) for p in range(a // E * E, a)] + [(t, p) for p in range(b, up)]
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# name -> builder(V) -> (row lengths, Aj int32, columns); REFUSED: the cases whose copy is not granted (at every V)

def _ap(lens):
    return np.r_[0, np.cumsum(lens)].astype(np.int32)


def _band(lens, cols, width, seed, sort=True):
    """Seeded columns within +-width of the row's place on the diagonal of a rows x cols matrix."""
    lens = np.asarray(lens, np.int64)
    rng = np.random.default_rng(seed)
    rows = len(lens)
    centre = np.repeat(np.arange(rows) * cols // max(rows, 1), lens)
    Aj = np.clip(centre + rng.integers(-width, width + 1, size=int(lens.sum())), 0, cols - 1)
    if sort:
        Ap = np.r_[0, np.cumsum(lens)]
        for r in range(rows):
            Aj[Ap[r]:Ap[r + 1]].sort()
    return Aj.astype(np.int32)


def _poisson(ny, nx):
    return lambda V: (ut._poisson_lens(nx, ny), ut._poisson_cols(nx, ny), nx * ny)


def _equal(K):
    lens = np.full(3003, K, np.int64)
    return lambda V: (lens, _band(lens, 3003, 40, 100 + K), 3003)


def _rows_1_16(V):
    lens = np.random.default_rng(11).integers(1, 17, size=3000)
    return lens, _band(lens, 3000, 2000, 12), 3000


def _span(extra):
    def make(V):
        lens = np.full(1001, 5, np.int64)
        Aj = np.random.default_rng(13).integers(100, 5001, size=5005).astype(np.int32)
        Aj[2500:2505] = [100, 200, 300, 400, 100 + extra]  # one row: the same tile at every V; nothing else lies below 100
        return lens, Aj, 70001
    return make


def _opposite_ends(V):
    """Rows of 5: the tiles' first entries are multiples of 5 (odd ones, and ones that are no multiple of 4, among them); the
    columns of even tiles lie in [0, 3000), those of odd tiles in the last 1000 columns, [69500, 70500): an even tile's offset on an
    odd tile's base points past the end of x."""
    lens = np.full(1001, 5, np.int64)
    tile, _, _ = tile_of_entry(_ap(lens), V)
    rng = np.random.default_rng(14)
    Aj = np.where(tile % 2 == 1, 69500 + rng.integers(0, 1000, size=5005), rng.integers(0, 3000, size=5005))
    return lens, Aj.astype(np.int32), 70500


def _rank_block(V):
    """Rows 0..n of a sharded operator: the columns are the global ones, n0 + the row + small offsets."""
    n, n0 = 2000, 50000
    lens = np.full(n, 5, np.int64)
    Aj = n0 + np.repeat(np.arange(n), 5) + np.tile(np.array([-45, -1, 0, 1, 45]), n)
    return lens, np.clip(Aj, 0, n0 + n + 44).astype(np.int32), n0 + n + 45


def _unsorted(V):
    lens = np.random.default_rng(15).integers(3, 9, size=2000)
    return lens, _band(lens, 2600, 300, 16, sort=False), 2600


def _empty_runs(V):
    lens = ut._with_empty_runs(4000, [(0, 70), (600, 1), (1200, 70), (1800, 1), (2400, 300), (3200, 1), (4000, 300)])
    return lens, _band(lens, len(lens), 60, 17), len(lens)


def _single_row(V):
    return np.array([5], np.int64), np.array([3, 1, 4, 1, 5], np.int32), 9


def _single_tile(V):
    lens = np.full(41, 5, np.int64)  # 205 entries: odd, and no multiple of 4 -- the arrays' last vector
    return lens, _band(lens, 41, 6, 18), 41


def _scattered(V):
    lens = np.full(1001, 5, np.int64)
    return lens, np.random.default_rng(19).integers(0, 80000, size=5005).astype(np.int32), 80000


BUILDERS = {
    "poisson5pt_37x41": _poisson(37, 41), "poisson5pt_9x451": _poisson(9, 451),
    "equal_1": _equal(1), "equal_2": _equal(2), "equal_3": _equal(3),
    "rows_1_16_band_2000": _rows_1_16,
    "span_65535": _span(65535), "span_65536": _span(65536),
    "opposite_ends": _opposite_ends, "rank_block": _rank_block, "unsorted": _unsorted, "empty_runs": _empty_runs,
    "single_row": _single_row, "single_tile_odd_entries": _single_tile, "scattered": _scattered,
}
CASES = tuple(BUILDERS)
REFUSED = ("span_65536", "scattered")  # every other case is granted, at every V


def structure(name, V):
    """(Ap int32, Aj int32, columns) of a case at V index vectors per lane (only `opposite_ends` depends on V)."""
    lens, Aj, cols = BUILDERS[name](V)
    Ap = _ap(lens)
    assert len(Aj) == int(Ap[-1]) and Aj.dtype == np.int32 and (len(Aj) == 0 or (Aj.min() >= 0 and Aj.max() < cols))
    return Ap, Aj, cols


def vectors(name, V, dtype):
    """Seeded (Ax, x, y0, w) of a case in `dtype`: normal deviates, so hardly any product or sum is exact."""
    Ap, _, cols = structure(name, V)
    rng = np.random.default_rng(9500 + CASES.index(name))
    rows, nnz = len(Ap) - 1, int(Ap[-1])
    return (rng.standard_normal(nnz).astype(dtype), rng.standard_normal(cols).astype(dtype), rng.standard_normal(rows).astype(dtype),
            rng.standard_normal(rows).astype(dtype))
