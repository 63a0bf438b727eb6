"""The shift-invariant tiles of tests/shift_tiles_refs.py against brute force (CPU only): the marking, the table, the keep rule, the
multiplier that stands for the division by the row length, the kernel's column formula at every position its vectors cover, and every
case contains what the GPU test needs it for."""
import numpy as np
import pytest

import cols16_refs as c16
import shift_tiles_refs as sh
import uniform_tiles_refs as ut


@pytest.mark.parametrize("name", sh.CASES)
def test_marking_equals_brute_force(name):
    for V in sh.V_ALL:
        Ap, Aj, cols = sh.structure(name, V)
        L = int(np.diff(Ap.astype(np.int64)).max())
        assert ut.admits(L, V), (name, V)  # every case runs at every V
        marked, shift, with_entries = sh.table(Ap, Aj, V)
        assert np.array_equal(marked, sh.brute_force(Ap, Aj, V)), (name, V)
        row_start, nz, _, _ = ut.partition(Ap, V)
        uni = (np.diff(row_start) > 0) & (np.diff(nz) == np.diff(row_start) * L)
        assert not (marked & ~uni).any(), (name, V)  # a marked tile is always one of the kernel's equal-length tiles
        assert with_entries == int((np.diff(nz) > 0).sum()) >= 1
        for t in range(len(marked)):
            if marked[t]:
                a, rs = int(nz[t]), int(row_start[t])
                assert [int(v) for v in shift[t][:L]] == [int(Aj[a + k]) - rs for k in range(L)] and not shift[t][L:].any(), (name, V, t)
                assert int(shift[t][0]) != sh.UNMARKED
            else:
                assert int(shift[t][0]) == sh.UNMARKED and not shift[t][1:].any(), (name, V, t)
        if name in sh.ALL_MARKED:
            assert marked.all(), (name, V)
        if name in sh.NONE_MARKED:
            assert not marked.any(), (name, V)
        keep, m = sh.kept(Ap, Aj, V)
        assert m == int(marked.sum())
        assert keep == (name not in sh.NOT_KEPT), (name, V, m, with_entries)


def test_multiplier_is_the_division():
    """(p M) >> 16 == p // L with M = ceil(65536 / L) for every p < 4096 and L = 1..8 -- in 24-bit operands and a 32-bit product."""
    p = np.arange(4096, dtype=np.uint64)
    for L in range(1, sh.MAX_LEN + 1):
        M = sh.div_mul(L)
        assert M <= sh.U24 and int(p.max()) * M <= sh.U32
        assert np.array_equal((p * np.uint64(M)) >> np.uint64(16), p // np.uint64(L)), L


@pytest.mark.parametrize("name", sh.CASES)
def test_columns_at_every_position(name):
    """Exact inside the tile, inside [0, num_cols) at the foreign positions of either end."""
    for V in sh.V_ALL:
        Ap, Aj, cols = sh.structure(name, V)
        marked = sh.table(Ap, Aj, V)[0]
        _, nz, _ = c16.tile_of_entry(Ap, V)
        for E in (2, 4):
            got = sh.kernel_columns(Ap, Aj, V, E, cols)
            foreign = {(t, q) for t, q in c16.foreign_positions(Ap, V, E) if marked[t]}
            assert foreign <= set(got)
            for (t, q), col in got.items():
                if nz[t] <= q < nz[t + 1]:
                    assert col == int(Aj[q]), (name, V, E, t, q)
                else:
                    assert (t, q) in foreign and 0 <= col < cols, (name, V, E, t, q, col)


def test_named_properties():
    for V in sh.V_ALL:
        # the counts of the cases shared with the 16-bit copy's tests
        Ap, Aj, _ = sh.structure("poisson5pt_9x451", V)
        marked = sh.table(Ap, Aj, V)[0]
        assert (int(marked.sum()), len(marked)) == {1: (56, 79), 2: (24, 39), 4: (9, 20)}[V]
        assert np.array_equal(marked[np.diff(ut.partition(Ap, V)[0]) > 0], ut.uniform_mask(Ap, V)[3])  # every uniform tile of the stencil
        # unsorted columns inside the rows, a duplicated column, rows of 9
        Aj = sh.structure("toeplitz_5", V)[1]
        assert (np.diff(Aj[:5].astype(np.int64)) < 0).any()
        assert len(set(sh.structure("toeplitz_duplicate", V)[1][:5].tolist())) == 4
        assert int(np.diff(sh.structure("toeplitz_9", V)[0]).max()) == 9
        # the near miss: exactly the tile of the edited row is unmarked, and the row is not the tile's first
        Ap, Aj, _ = sh.structure("near_miss", V)
        marked = sh.table(Ap, Aj, V)[0]
        row_start = ut.partition(Ap, V)[0]
        t = int(np.searchsorted(row_start, sh.NEAR_MISS_ROW, side="right")) - 1
        assert row_start[t] < sh.NEAR_MISS_ROW < row_start[t + 1] - 1
        assert not marked[t] and marked.sum() == len(marked) - 1 and len(marked) >= 3
        # uniform but not shift-invariant
        Ap, Aj, _ = sh.structure("uniform_not_shift", V)
        assert ut.uniform_mask(Ap, V)[3].all()
        # far end then near end: granted, alternating, and foreign positions of both kinds whose signed formula leaves x
        Ap, Aj, cols = sh.structure("far_near", V)
        granted, base, span, _ = c16.encode(Ap, Aj, V)
        marked, shift, _ = sh.table(Ap, Aj, V)
        row_start, nz, L, _ = ut.partition(Ap, V)
        assert granted and int(span.max()) <= c16.LIMIT and cols == 70500 and len(marked) >= 3
        assert int(Aj.min()) == 0 and int(Aj.max()) == cols - 1
        for t in range(len(marked)):
            tile_cols = Aj[nz[t]:nz[t + 1]]
            assert (int(tile_cols.min()) == 0) if t % 2 == 0 else (int(tile_cols.max()) == cols - 1)
        for E in (2, 4):
            signed = {}
            for t, q in c16.foreign_positions(Ap, V, E):
                p = q - int(nz[t])
                signed[(t, q)] = int(row_start[t]) + p // L + int(shift[t][p % L])
            assert any(c < 0 and t % 2 == 0 and q < nz[t] for (t, q), c in signed.items()), (V, E)      # before a near tile
            assert any(c >= cols and t % 2 == 1 and q >= nz[t + 1] for (t, q), c in signed.items()), (V, E)  # past a far tile
        # shifts that do not fit 16 bits
        Ap, Aj, cols = sh.structure("shift_60000", V)
        shift = sh.table(Ap, Aj, V)[1]
        assert int(shift[:, :5].min()) > 59000 and c16.encode(Ap, Aj, V)[0]
        # the keep rule on both sides of 1/4
        for name, want in (("keep_under", False), ("keep_over", True)):
            Ap, Aj, _ = sh.structure(name, V)
            marked, _, with_entries = sh.table(Ap, Aj, V)
            m = int(marked.sum())
            assert m >= 1 and marked[:m].all() and c16.encode(Ap, Aj, V)[0]
            assert (4 * m >= with_entries) == want and (4 * (m + 1) >= with_entries) and (4 * (m - 1) < with_entries), (name, V, m, with_entries)
        # the ends: a marked first tile, and a marked last tile whose last vector reaches past the arrays (the kernel's scalar path)
        Ap, Aj, cols = sh.structure("ends_odd_entries", V)
        marked = sh.table(Ap, Aj, V)[0]
        nnz = int(Ap[-1])
        assert marked[0] and marked[-1] and nnz % 2 == 1 and nnz % 4 != 0
        for E in (2, 4):
            assert (len(marked) - 1) not in {t for t, _ in sh.kernel_columns(Ap, Aj, V, E, cols)}
