"""The 16-bit column encoding of tests/cols16_refs.py against brute force (CPU only): per-tile base and span, the grant rule,
decode(encode(Aj)) == Aj wherever granted, and every case contains what the GPU test needs it for."""
import numpy as np
import pytest

import cols16_refs as c16
import uniform_tiles_refs as ut


@pytest.mark.parametrize("name", c16.CASES)
def test_encoding_equals_brute_force(name):
    for V in c16.V_ALL:
        Ap, Aj, cols = c16.structure(name, V)
        assert ut.admits(int(np.diff(Ap.astype(np.int64)).max()), V), (name, V)  # every case runs at every V
        granted, base, span, cols16 = c16.encode(Ap, Aj, V)
        want_granted, want_base, want_span = c16.brute_force(Ap, Aj, V)
        assert granted == want_granted and np.array_equal(base, want_base) and np.array_equal(span, want_span), (name, V)
        assert granted == (name not in c16.REFUSED), (name, V, int(span.max()))
        if granted:
            assert cols16.dtype == np.uint16 and np.array_equal(c16.decode(Ap, V, base, cols16), Aj.astype(np.int64)), (name, V)
            assert ((base >= 0) & (base < cols)).all(), (name, V)  # an in-range gather address for a foreign position set to its tile's base
        else:
            assert cols16 is None


def test_named_properties():
    for V in c16.V_ALL:
        # the grant rule's boundary: 65535 is granted, 65536 is not, and only that one tile decides
        for name, top in (("span_65535", 65535), ("span_65536", 65536)):
            Ap, Aj, cols = c16.structure(name, V)
            span = c16.encode(Ap, Aj, V)[2]
            assert cols >= 70000 and int(span.max()) == top and int((span > 5000).sum()) == 1, (name, V)
        # uniform and non-uniform tiles in the Poisson cases (the kernel's two row-bound paths)
        assert ut.tile_counts(c16.structure("poisson5pt_9x451", V)[0], V)[0] >= 3 and ut.tile_counts(c16.structure("poisson5pt_9x451", V)[0], V)[1] >= 3
        assert ut.tile_counts(c16.structure("poisson5pt_37x41", V)[0], V)[1] >= 3
        # more than 64 rows in a tile
        for K in (1, 2, 3):
            assert ut.uniform_mask(c16.structure(f"equal_{K}", V)[0], V)[0].max() > 64
        # opposite ends: granted, neighbouring windows 68 000+ columns apart, tiles that begin off the vector boundary, and foreign
        # positions whose unclamped column (their offset on the WRONG base) leaves x -- what the kernel's clamp is for
        Ap, Aj, cols = c16.structure("opposite_ends", V)
        granted, base, span, cols16 = c16.encode(Ap, Aj, V)
        tile, nz, tiles = c16.tile_of_entry(Ap, V)
        assert granted and cols >= 70000 and tiles >= 3 and (np.abs(np.diff(base[:tiles - 1])) > 68000).all(), V
        for E in (2, 4):
            assert (nz[1:tiles] % E != 0).any(), (V, E)
            foreign = c16.foreign_positions(Ap, V, E)
            assert len(foreign) >= 2, (V, E)
            wrong = [int(base[t]) + int(cols16[p]) for t, p in foreign]
            assert max(wrong) >= cols, (V, E, max(wrong))
            assert all(0 <= min(c, cols - 1) < cols for c in wrong)
        # the rank block: every column beyond the row count
        Ap, Aj, cols = c16.structure("rank_block", V)
        assert Aj.min() > len(Ap) - 1 and cols > Aj.max()
        # unsorted columns inside rows
        Ap, Aj, _ = c16.structure("unsorted", V)
        assert any((np.diff(Aj[Ap[r]:Ap[r + 1]].astype(np.int64)) < 0).any() for r in range(len(Ap) - 1))
        # runs of empty rows at the start, inside and at the end; tiles without any entry get base 0
        Ap, Aj, _ = c16.structure("empty_runs", V)
        assert Ap[70] == 0 and Ap[-301] == Ap[-1] and int((np.diff(Ap) == 0).sum()) >= 700
        # the arrays' last vector
        for name in ("single_row", "single_tile_odd_entries"):
            Ap = c16.structure(name, V)[0]
            assert int(Ap[-1]) % 2 == 1 and int(Ap[-1]) % 4 != 0 and c16.tile_of_entry(Ap, V)[2] == 1
