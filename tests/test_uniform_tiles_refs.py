"""The cases of tests/uniform_tiles_refs.py contain what they claim (CPU only): csr_wavev's uniform-tile predicate, restated in
numpy, equals "every row of the tile has the longest row's length" on every tile of every case, and every case has the tiles the
GPU test needs it for."""
import numpy as np
import pytest

import uniform_tiles_refs as ut


def _admitted(name):
    Ap = ut.structure(name)[0]
    max_len = int(np.diff(Ap.astype(np.int64)).max())
    return [V for V in ut.V_ALL if ut.admits(max_len, V)]


@pytest.mark.parametrize("name", ut.CASES)
def test_predicate_is_equal_lengths_on_every_tile(name):
    Ap = ut.structure(name)[0]
    Vs = _admitted(name)
    assert Vs == list(ut.V_ALL), (name, Vs)  # every case runs at every V
    for V in Vs:
        nr, cnt, _, uni = ut.uniform_mask(Ap, V)
        assert np.array_equal(uni, ut.brute_force_mask(Ap, V)), (name, V)
        assert int(nr.sum()) == len(Ap) - 1 and int(cnt.sum()) == int(Ap[-1]), (name, V)  # the tiles cover the matrix once


@pytest.mark.parametrize("name", ut.CASES)
def test_case_contains_what_it_claims(name):
    Ap, Aj, cols, claim = ut.structure(name)
    assert Aj.min() >= 0 and Aj.max() < cols
    for V in ut.V_ALL:
        nr, cnt, nz0, uni = ut.uniform_mask(Ap, V)
        n_uni, n_other = ut.tile_counts(Ap, V)
        assert (n_uni, n_other) == (int(uni.sum()), int((~uni).sum()))
        if claim == "both":
            assert n_uni >= 3 and n_other >= 3, (name, V, n_uni, n_other)
        elif claim in ("uniform", "turns"):
            assert n_uni >= 1 and n_other == 0, (name, V, n_uni, n_other)
            if claim == "turns":
                assert nr.max() > 64, (name, V, int(nr.max()))
        elif claim == "none":
            assert n_uni == 0 and n_other >= 1, (name, V, n_uni)
        elif claim == "lookalike":
            assert n_uni == 0 and int((cnt == 5 * nr).sum()) >= 3, (name, V, int((cnt == 5 * nr).sum()))


def test_named_properties():
    for V in ut.V_ALL:
        # uniform and boundary tiles interleaved, a uniform tile that starts at an odd entry (f64: not at a 16-byte boundary)
        _, _, nz0, uni = ut.uniform_mask(ut.structure("poisson5pt_9x451")[0], V)
        assert (nz0[uni] % 2 == 1).any() and (nz0[uni] % 4 != 0).any(), V
        flips = int((uni[1:] != uni[:-1]).sum())
        assert flips >= 4, (V, flips)
        # the arrays' last vector on a uniform tile: entries odd and no multiple of 4, the last tile uniform
        Ap = ut.structure("equal_5_odd_entries")[0]
        assert int(Ap[-1]) % 2 == 1 and int(Ap[-1]) % 4 != 0 and ut.uniform_mask(Ap, V)[3][-1]
        # the mirror case: max_len stays 5, exactly the tile with the short row is not uniform
        assert ut.tile_counts(ut.structure("one_row_of_3")[0], V)[1] == 1
        # tiles full of empty rows: many rows, few entries; empty rows in the first and in the last tile
        Ap = ut.structure("empty_runs")[0]
        nr, cnt, _, uni = ut.uniform_mask(Ap, V)
        assert nr.max() >= 300 and not uni[0] and not uni[-1]
        assert Ap[70] == 0 and Ap[-301] == Ap[-1]
        assert (nr[~uni].astype(np.int64) * 5 > cnt[~uni]).all()
    assert ut.tile_counts(ut.structure("single_row")[0], 1) == (1, 0)
    assert ut.tile_counts(ut.structure("single_tile")[0], 1) == (1, 0)
