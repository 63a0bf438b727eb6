"""CPU tests of the constant tiles' restatement (tests/const_tiles_refs.py): what is marked and what is not, the keep rule at its boundary, the
headline matrix's counts, the new C-ABI entries' declarations and refusals, and the stream-contract inventory with the new header.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import const_tiles_refs as ct
import shift_tiles_refs as sh
import uniform_tiles_refs as ut
from conftest import ROOT

INVALID = 1
HEADER = os.path.join(ROOT, "include", "cusp_mi355x.h")


def _case(L, rows=1001, dtype=np.float64):
    Ap, Aj, cols, first = ct.toeplitz(rows, L, dtype)
    return Ap, Aj, ct.constant_values(rows, first)


@pytest.mark.parametrize("V", ut.V_ALL)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_identical_rows_are_marked_in_every_tile(dtype, V):
    for L in range(1, 9):
        Ap, Aj, Ax = _case(L, rows=3003, dtype=dtype)  # (at least two tiles at every L and V)
        const, with_entries, skipped = ct.marks(Ap, Aj, Ax, V)
        assert const.all() and len(const) >= 2 and skipped == len(Ax), (L, V)
        assert np.array_equal(const, ct.brute_force(Ap, Aj, Ax, V))
        assert ct.kept(Ap, Aj, Ax, V) == (True, with_entries)


def _flip_last_bit(Ax, e):
    w = ct.bits(Ax).copy()
    w[e] ^= 1
    return w.view(Ax.dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_one_last_bit_zero_sign_and_nan_payload_unmark_their_tile_only(dtype):
    Ap, Aj, Ax = _case(5, dtype=dtype)
    tiles = len(ut.partition(Ap, 1)[1]) - 1
    a, e = ct.tile_rows(Ap, 1, 2)
    last = 5 * (e - 1) + 3  # the tile's last row, fourth value
    const = ct.marks(Ap, Aj, _flip_last_bit(Ax, last), 1)[0]
    assert not const[2] and const.sum() == tiles - 1 and np.array_equal(const, ct.brute_force(Ap, Aj, _flip_last_bit(Ax, last), 1))
    # the tile's FIRST row edited: every other row differs from it
    assert not ct.marks(Ap, Aj, _flip_last_bit(Ax, 5 * a), 1)[0][2]
    # +0 against -0: equal as floats, different words
    Z = Ax.copy()
    Z[3::5] = 0.0
    assert ct.marks(Ap, Aj, Z, 1)[0].all()
    Z[last] = -0.0
    assert Z[last] == Z[last - 5] and not ct.marks(Ap, Aj, Z, 1)[0][2] and ct.marks(Ap, Aj, Z, 1)[0].sum() == tiles - 1
    # NaN: the same payload everywhere is constant (never equal as floats); another payload is not
    N = Ax.copy()
    N[1::5] = np.nan
    assert ct.marks(Ap, Aj, N, 1)[0].all() and np.array_equal(ct.marks(Ap, Aj, N, 1)[0], ct.brute_force(Ap, Aj, N, 1))
    other = _flip_last_bit(N, 5 * (e - 1) + 1)
    assert np.isnan(other[5 * (e - 1) + 1]) and not ct.marks(Ap, Aj, other, 1)[0][2]


def test_only_tiles_the_shift_table_marks_are_candidates():
    """Constant values on rows whose columns are not shift-invariant, and on rows of 9: nothing is marked."""
    for name in ("uniform_not_shift", "toeplitz_9"):
        Ap, Aj, _ = sh.structure(name, 1)
        Ax = np.full(len(Aj), 1.5)
        const, _, skipped = ct.marks(Ap, Aj, Ax, 1)
        assert not const.any() and skipped == 0 and ct.kept(Ap, Aj, Ax, 1) == (False, 0)


def test_keep_rule_at_the_quarter():
    assert not ct.keep_rule(0, 0) and not ct.keep_rule(0, 3) and ct.keep_rule(1, 4) and not ct.keep_rule(1, 5) and ct.keep_rule(2, 8) and not ct.keep_rule(2, 9)
    # rows of 5 over 1001 rows, every tile shift-invariant, the first m tiles constant and seeded values elsewhere
    Ap, Aj, _, first = ct.toeplitz(1001, 5, np.float64)
    row_start, nz, _, _ = ut.partition(Ap, 1)
    with_entries = int((np.diff(nz) > 0).sum())
    for over in (False, True):
        m = (with_entries + 3) // 4 - (0 if over else 1)
        Ax = np.random.default_rng(7).standard_normal(len(Aj))
        Ax[:5 * int(row_start[m])] = ct.constant_values(int(row_start[m]), first)
        assert ct.kept(Ap, Aj, Ax, 1) == (over, m), over


def test_headline_matrix_counts(orc):
    """poisson5pt 3162 x 3162 at V = 1: 198 265 of the 201 527 wave tiles are constant, and 49 169 720 of the 49 978 572 values are never streamed."""
    Ap, Aj, Ax = orc.poisson5pt_csr(3162, 3162)
    row_start, nz, L, _ = ut.partition(Ap, 1)
    assert L == 5 and len(nz) - 1 == 201527
    # the shift table's marks from the rows (the entry-wide restatement of shift_tiles_refs needs several GB here): a tile of full rows in which every
    # row's columns are its predecessor's plus one
    Ap64 = np.asarray(Ap, np.int64)
    full = np.diff(Ap64) == 5
    r = np.flatnonzero(full[1:] & full[:-1]) + 1
    moved = np.ones(len(full), bool)
    ok = np.ones(len(r), bool)
    for k in range(5):
        ok &= Aj[Ap64[r] + k] == Aj[Ap64[r - 1] + k] + 1
    moved[r] = ~ok
    run = np.concatenate(([0], np.cumsum(moved)))
    notfull = np.concatenate(([0], np.cumsum(~full)))
    a, e = row_start[:-1], row_start[1:]
    marked = (e > a) & (notfull[e] - notfull[a] == 0) & (run[e] - run[np.minimum(a + 1, e)] == 0)
    assert int(marked.sum()) == 198265
    const, with_entries, skipped = ct.marks(Ap, Aj, Ax, 1, marked=marked)
    assert (int(const.sum()), skipped, with_entries) == (198265, 49169720, 201527)
    assert ct.keep_rule(int(const.sum()), with_entries) and ct.mark_bytes(Ap, 1) == 4 * 6298


# ---- the C-ABI: the setter without a stream, the count, and the inventory --------------------------------------------------------------
def _params(name):
    text = open(HEADER).read()
    m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/cusp_mi355x.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_symbols_prototypes_and_wrappers(cmi):
    L = cmi.lib()
    assert len(L.cmi_plan_drop_const_tiles.argtypes) == 1 and len(L.cmi_plan_const_tiles.argtypes) == 2
    assert callable(cmi.plan_drop_const_tiles) and cmi.binding.plan_drop_const_tiles is cmi.plan_drop_const_tiles
    assert callable(cmi.Plan.const_tiles) and callable(cmi.Plan.drop_const_tiles)


def test_declarations_take_no_stream():
    assert _params("cmi_plan_drop_const_tiles") == ["cmi_plan *plan"]
    assert _params("cmi_plan_const_tiles") == ["const cmi_plan *plan", "int64_t *tiles"]
    assert _params("cmi_plan_validate_values") == ["const cmi_plan *plan", "const void *values", "void *stream", "int *valid_host"]  # (unchanged)


def test_null_plan_is_refused_without_a_device_call(cmi):
    L = cmi.lib()
    assert L.cmi_plan_drop_const_tiles(None) == INVALID
    assert b"null plan" in L.cmi_last_error(), L.cmi_last_error()
    n = ctypes.c_int64(-1)
    assert L.cmi_plan_const_tiles(None, ctypes.byref(n)) == INVALID and n.value == -1
    with pytest.raises(cmi.CmiError) as e:
        cmi.plan_drop_const_tiles(None)
    assert e.value.status == INVALID


def test_stream_contract_inventory_is_unedited_and_complete():
    """The new entries take no stream, so the table of tests/stream_contract.py has neither a missing nor a stale row with this header."""
    import collections

    import stream_contract as SC
    families = SC.header_families(open(HEADER).read())
    assert "cmi_plan_drop_const_tiles" not in families and "cmi_plan_const_tiles" not in families
    count = collections.Counter(r.family for r in SC.ROWS)
    assert set(families) == set(count) and all(c == 1 for c in count.values())
