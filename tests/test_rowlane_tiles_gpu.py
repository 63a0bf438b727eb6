"""csr_wavev's marked (shift-invariant) tiles with x loaded per ROW lane on an MI355X: a marked tile asks for x[rs + r + shift[k]],
k < L, with the lane that sums row r, in the batch of its value requests, parks the VALUES in LDS and forms the products in the row
lane (csrc/spmv_csr.hip, wavev_rowlane_tile).  The cases are the smallest shapes at which that path can go wrong: the turn boundary of
the row loop (1, 63, 64, 65 rows in one tile), tiles of several turns (their x of turn >= 1 is loaded inside the loop), every slot
count up to 8, a matrix with fewer columns than rows (a lane without a row asks for the tile's last row's x), windows that end exactly
at column 0 and at the last column with NaN guard cells around x, IEEE special values in Ax and x, and a near miss whose one tile runs
the 16-bit column path between marked neighbours.

Every case runs through an explicit CSR_STREAM_WAVEV config with nontemporal 3 | 8 in f64 and f32 at V = 1, 2, 4 -- plain,
accumulating (y pre-filled with normal deviates) and with the fused <y, w> -- and y is compared bit for bit to the oracle host loop,
obtained as tests/test_shift_tiles_gpu.py obtains it.  Every case first asserts that the plan's count of marked tiles equals the
restatement's (tests/shift_tiles_refs.py::table), so no case silently runs the unmarked path.

A tile takes the row-lane path only when its last vector ends inside the arrays; the LAST tile of a matrix whose entry count is no
multiple of the vector width (2 in f64, 4 in f32) sums its rows straight from the arrays instead.  The single-tile cases with rows of 3
are the issue's; the same with rows of 2 (one tile at every V; a whole number of vectors in f64) and of 4 (a whole number of vectors
in f64 and f32; one tile at V = 2 and 4, 63 rows and the rest at V = 1) put the same row counts on the row-lane path."""
import math

import numpy as np
import pytest

import cols16_refs as c16
import shift_tiles_refs as sh
import special_values as sv
import uniform_tiles_refs as ut
from test_cols16_gpu import COLS16, _dev

TURN_ROWS = (1, 63, 64, 65)  # around the 64 rows of one turn of the row loop


def _fewer_columns(V):
    """300 empty rows, then 700 rows of 5 with column = row + (-300, -299, -298, -297, -296): 1000 x 705.  The tile that holds the
    empty rows is no equal-length tile; every later one is marked."""
    lens = np.r_[np.zeros(300, np.int64), np.full(700, 5, np.int64)]
    Aj = np.repeat(np.arange(300, 1000), 5) + np.tile(np.arange(-300, -295), 700)
    return lens, Aj.astype(np.int32), 705


BUILDERS = {f"one_tile_{L}x{rows}": sh._toeplitz(L, rows=rows) for L in (3, 2, 4) for rows in TURN_ROWS}
BUILDERS.update({f"turns_{L}": sh._toeplitz(L, rows=1001) for L in (1, 2, 3, 5)})  # tiles of up to 252 V rows: several turns
BUILDERS.update({f"slots_{L}": sh._toeplitz(L, rows=1001) for L in (7, 8)})
BUILDERS.update({
    "fewer_columns": _fewer_columns,
    "guard_cells": sh.BUILDERS["far_near"],
    "special_values": sh._toeplitz(5, rows=1001),
    "near_miss": sh.BUILDERS["near_miss"],
})
CASES = tuple(BUILDERS)
V_DEPENDENT = ("guard_cells",)
GUARD = 64  # cells of NaN on either side of x (512 / 256 bytes: x keeps its alignment)

_REF = {}


def _special(a, start, step, dtype):
    """+-0, +-inf, NaN, the smallest and a larger subnormal, the smallest normal, at a[start::step] in turn."""
    info = np.finfo(dtype)
    deck = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, info.smallest_subnormal, -info.tiny / 4, info.tiny], dtype)
    at = np.arange(start, len(a), step)
    a[at] = deck[np.arange(len(at)) % len(deck)]


def reference(orc, name, V, tag):
    """Inputs and the host loop's results of a case, computed once and shared (read-only)."""
    key = (name, V if name in V_DEPENDENT else 0, tag)
    if key not in _REF:
        dtype = np.float64 if tag == "f64" else np.float32
        lens, Aj, cols = BUILDERS[name](V)
        Ap = c16._ap(lens)
        assert len(Aj) == int(Ap[-1]) and Aj.dtype == np.int32 and Aj.min() >= 0 and Aj.max() < cols
        rng = np.random.default_rng(21000 + CASES.index(name))
        rows, nnz = len(Ap) - 1, int(Ap[-1])
        Ax, x, y0, w = (rng.standard_normal(n).astype(dtype) for n in (nnz, cols, rows, rows))
        if name == "special_values":
            _special(Ax, 11, 97, dtype)
            _special(x, 5, 61, dtype)
        with np.errstate(all="ignore"):
            want, want_acc = orc.spmv_csr(Ap, Aj, Ax, x), orc.spmv_csr(Ap, Aj, Ax, x, y0.copy())
            prod = want.astype(np.float64) * w.astype(np.float64)
        finite = bool(np.isfinite(prod).all())
        item = dict(Ap=Ap, Aj=Aj, cols=cols, Ax=Ax, x=x, y0=y0, w=w, want=want, want_acc=want_acc,
                    dot=math.fsum(prod.tolist()) if finite else math.nan, dot_abs=math.fsum(np.abs(prod).tolist()) if finite else math.nan)
        for v in item.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = item
    return _REF[key]


def _structure(name, V, R):
    """(marked tiles, tiles that have entries) of a case by the restatement, after checking that the case is what its name says."""
    Ap, Aj = R["Ap"], R["Aj"]
    marked, _, tiles = sh.table(Ap, Aj, V)
    count = int(marked.sum())
    assert sh.kept(Ap, Aj, V) == (True, count), (name, V)  # the copy is granted and the table kept: the count is the plan's
    if name == "near_miss":
        assert count == tiles - 1 and tiles >= 3, (name, V, count, tiles)
    elif name == "fewer_columns":
        assert count == tiles - 1 and not marked[0] and tiles >= 4, (name, V, count, tiles)
    else:
        assert count == tiles, (name, V, count, tiles)
    if name.startswith("one_tile") and (V >= 2 or not name.startswith("one_tile_4")):
        assert tiles == 1, (name, V)
    if name in ("turns_1", "turns_2", "turns_3") and V == 1 or name == "turns_5" and V >= 2:
        assert int(np.diff(ut.partition(Ap, V)[0]).max()) > 64, (name, V)  # a tile of more than one turn
    return count, tiles


def _x_on_device(R, tdt, guarded):
    """x on the device; `guarded`: inside a larger buffer whose cells outside [0, columns) are NaN (returned too: it owns the memory)."""
    import torch
    if not guarded:
        return _dev(R["x"]), None
    cols = R["cols"]
    big = torch.full((cols + 2 * GUARD,), math.nan, dtype=tdt, device="cuda")
    big[GUARD:GUARD + cols] = _dev(R["x"])
    return big[GUARD:GUARD + cols], big


def _three_ways(cmi, plan, R, dAp, dAj, dAx, dx, tdt, what):
    """Plain, accumulating and with the fused <y, w>: y bit for bit; the dot to the fold's bound, or NaN where the host's products are."""
    import torch
    rows, cols = len(R["Ap"]) - 1, R["cols"]
    y = torch.full((rows,), 9.0, dtype=tdt, device="cuda")
    cmi.spmv_csr_plan(plan, dAp, dAj, dAx, dx, y)
    sv.same_bits(y.cpu().numpy(), R["want"], what)
    y = _dev(R["y0"])
    cmi.spmv_csr_plan(plan, dAp, dAj, dAx, dx, y, accumulate=True)
    sv.same_bits(y.cpu().numpy(), R["want_acc"], what + " accumulate")
    res = torch.zeros(1, dtype=torch.float64, device="cuda")
    y = torch.full((rows,), 9.0, dtype=tdt, device="cuda")
    cmi.spmv_csr_dot(rows, cols, dAp, dAj, dAx, dx, y, _dev(R["w"]), res, cmi.blas_workspace(), plan=plan)
    sv.same_bits(y.cpu().numpy(), R["want"], what + " fused dot: y")
    if math.isnan(R["dot"]):
        assert not math.isfinite(res.item()), (what, res.item())
    else:
        assert abs(res.item() - R["dot"]) <= 1e-9 * R["dot_abs"] + 1e-300, (what, res.item(), R["dot"])


@pytest.mark.gpu
@pytest.mark.parametrize("V", sh.V_ALL)
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_rowlane_tiles_bit_exact(cmi, orc, tag, V):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    tdt = torch.float64 if tag == "f64" else torch.float32
    for name in CASES:
        R = reference(orc, name, V, tag)
        Ap, Aj = R["Ap"], R["Aj"]
        count, tiles = _structure(name, V, R)
        what = f"{name} {tag} V={V} ({count} of {tiles} tiles with entries marked)"
        dAp, dAj, dAx = _dev(Ap), _dev(Aj), _dev(R["Ax"])
        dx, owner = _x_on_device(R, tdt, guarded=(name == "guard_cells"))
        plan = cmi.Plan.csr(tdt, len(Ap) - 1, R["cols"], dAp, dAj,
                            cfg=cmi.Config(kernel=cmi.CSR_STREAM_WAVEV, items_per_thread=V, nontemporal=3 | COLS16))
        c = plan.config()
        assert (c.kernel, c.items_per_thread, c.nontemporal) == (cmi.CSR_STREAM_WAVEV, V, 3 | COLS16), (what, c)
        assert plan.shifted_tiles() == count, (what, plan.shifted_tiles())
        _three_ways(cmi, plan, R, dAp, dAj, dAx, dx, tdt, what)
        if owner is not None:  # the guards are still what they were, and no row of y saw one (y is the host loop's, bit for bit, above)
            assert bool(torch.isnan(owner[:GUARD]).all()) and bool(torch.isnan(owner[GUARD + R["cols"]:]).all()), what
            assert not np.isnan(R["want"]).any() and not np.isnan(R["want_acc"]).any(), what


def test_rowlane_cases_are_what_their_names_say(orc):
    """The structure every GPU case asserts before it runs, checked without a GPU too: marks, keep rule, tile and turn counts."""
    for V in sh.V_ALL:
        for name in CASES:
            _structure(name, V, reference(orc, name, V, "f64"))


def test_rowlane_guard_cells_windows_touch_both_ends(orc):
    """What the guard-cell case claims about its own structure: at every V there is a marked tile whose first row holds column 0 and
    one whose last row holds the last column, so a window one cell too wide on either side reads a NaN."""
    for V in sh.V_ALL:
        R = reference(orc, "guard_cells", V, "f64")
        row_start = ut.partition(R["Ap"], V)[0]
        marked = sh.table(R["Ap"], R["Aj"], V)[0]
        firsts = [int(R["Aj"][5 * int(row_start[t]):5 * int(row_start[t]) + 5].min()) for t in np.flatnonzero(marked)]
        lasts = [int(R["Aj"][5 * int(row_start[t + 1]) - 5:5 * int(row_start[t + 1])].max()) for t in np.flatnonzero(marked)]
        assert 0 in firsts and R["cols"] - 1 in lasts, V
