"""csr_wavev forming the columns of shift-invariant tiles from their first row on an MI355X.  Every case of tests/shift_tiles_refs.py
(tests/test_shift_tiles_refs.py shows what each contains: the cases of the 16-bit column copy plus Toeplitz rows of 1..9 entries, a
near miss, far and near ends of x, shifts beyond 16 bits, the keep rule's two sides, the arrays' ends) runs through an explicit
CSR_STREAM_WAVEV config with nontemporal 3 | 8 in f64 and f32 at V = 1, 2, 4 and through the checks of tests/test_cols16_gpu.py: plain,
accumulating and the fused <y, w>, y compared bit for bit to the oracle host loop.  The plan reports the restatement's count of marked
tiles exactly when the restatement keeps the table, and its device bytes grow by 32 per tile exactly then."""
import math

import numpy as np
import pytest

import cols16_refs as c16
import shift_tiles_refs as sh
import uniform_tiles_refs as ut
from test_cols16_gpu import COLS16, _dev, _three_ways

pytestmark = pytest.mark.gpu

_REF = {}
V_DEPENDENT = ("opposite_ends", "far_near", "keep_under", "keep_over")


def reference(orc, name, V, tag):
    """Inputs and the host loop's results of a case, computed once and shared (read-only)."""
    key = (name, V if name in V_DEPENDENT else 0, tag)
    if key not in _REF:
        dtype = np.float64 if tag == "f64" else np.float32
        Ap, Aj, cols = sh.structure(name, V)
        Ax, x, y0, w = sh.vectors(name, V, dtype)
        want, want_acc = orc.spmv_csr(Ap, Aj, Ax, x), orc.spmv_csr(Ap, Aj, Ax, x, y0.copy())
        prod = (want.astype(np.float64) * w.astype(np.float64)).tolist()
        item = dict(Ap=Ap, Aj=Aj, cols=cols, Ax=Ax, x=x, y0=y0, w=w, want=want, want_acc=want_acc, dot=math.fsum(prod),
                    dot_abs=math.fsum(map(abs, prod)))
        for v in item.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = item
    return _REF[key]


def _plans(cmi, tdt, R, V, dAp, dAj):
    rows, cols = len(R["Ap"]) - 1, R["cols"]
    plain = cmi.Plan.csr(tdt, rows, cols, dAp, dAj, cfg=cmi.Config(kernel=cmi.CSR_STREAM_WAVEV, items_per_thread=V, nontemporal=3))
    plan = cmi.Plan.csr(tdt, rows, cols, dAp, dAj, cfg=cmi.Config(kernel=cmi.CSR_STREAM_WAVEV, items_per_thread=V, nontemporal=3 | COLS16))
    return plain, plan


@pytest.mark.parametrize("V", sh.V_ALL)
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_shift_tiles_bit_exact(cmi, orc, tag, V):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    tdt = torch.float64 if tag == "f64" else torch.float32
    for name in sh.CASES:
        R = reference(orc, name, V, tag)
        Ap, Aj = R["Ap"], R["Aj"]
        nnz = int(Ap[-1])
        granted = c16.encode(Ap, Aj, V)[0]
        keep, marked = sh.kept(Ap, Aj, V)
        assert keep == (name not in sh.NOT_KEPT) and (granted or not keep)
        what = f"{name} {tag} V={V} ({marked} marked, table {'kept' if keep else 'not kept'})"
        dAp, dAj, dAx, dx = _dev(Ap), _dev(Aj), _dev(R["Ax"]), _dev(R["x"])
        plain, plan = _plans(cmi, tdt, R, V, dAp, dAj)
        c = plan.config()
        assert (c.kernel, c.items_per_thread, c.nontemporal) == (cmi.CSR_STREAM_WAVEV, V, 3 | COLS16 if granted else 3), (what, c)
        assert plan.shifted_tiles() == (marked if keep else 0) and plain.shifted_tiles() == 0, (what, plan.shifted_tiles())
        tiles = len(ut.partition(Ap, V)[1]) - 1
        grown = plan.device_bytes() - plain.device_bytes()
        assert grown == ((2 * (nnz + 8) + 4 * tiles + (sh.table_bytes(Ap, V) if keep else 0)) if granted else 0), (what, grown)
        assert plan.validate(dAp, dAj), what
        _three_ways(cmi, plan, R, dAp, dAj, dAx, dx, tdt, what)


def test_shift_tiles_near_miss_runs_through_its_cols16(cmi, orc):
    """The edited row's tile is the only unmarked one (the plan's count says so), and y is exact: that tile reads the 16-bit copy."""
    import torch
    for V in sh.V_ALL:
        R = reference(orc, "near_miss", V, "f64")
        dAp, dAj, dAx, dx = _dev(R["Ap"]), _dev(R["Aj"]), _dev(R["Ax"]), _dev(R["x"])
        _, plan = _plans(cmi, torch.float64, R, V, dAp, dAj)
        marked = sh.table(R["Ap"], R["Aj"], V)[0]
        assert plan.shifted_tiles() == len(marked) - 1 == int(marked.sum()), V
        _three_ways(cmi, plan, R, dAp, dAj, dAx, dx, torch.float64, f"near_miss V={V}")


def test_shift_tiles_plan_is_stale_after_a_column_edit(cmi, orc):
    import torch
    R = reference(orc, "toeplitz_5", 1, "f64")
    dAp, dAj = _dev(R["Ap"]), _dev(R["Aj"])
    plain, plan = _plans(cmi, torch.float64, R, 1, dAp, dAj)
    assert plan.shifted_tiles() > 0 and plan.validate(dAp, dAj)
    e = len(R["Aj"]) // 2  # inside a marked tile (every tile of this case is marked)
    dAj[e] = int(R["Aj"][e]) + 1  # one column, in place
    assert not plan.validate(dAp, dAj)
    assert plain.validate(dAp, dAj)  # a plan without bit 8 holds nothing derived from the columns
    dAj[e] = int(R["Aj"][e])
    assert plan.validate(dAp, dAj)


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_shift_tiles_need_the_columns(cmi, orc, tag):
    """A plan made from the row offsets alone, asked for bit 8: cleared, no table, y exact."""
    import torch
    tdt = torch.float64 if tag == "f64" else torch.float32
    R = reference(orc, "toeplitz_5", 1, tag)
    rows, cols, nnz = len(R["Ap"]) - 1, R["cols"], int(R["Ap"][-1])
    dAp, dAj, dAx, dx = _dev(R["Ap"]), _dev(R["Aj"]), _dev(R["Ax"]), _dev(R["x"])
    plan = cmi.Plan(cmi.FORMAT_CSR, tdt, rows, cols, nnz, dAp, cmi.Config(kernel=cmi.CSR_STREAM_WAVEV, items_per_thread=1, nontemporal=3 | COLS16))
    c = plan.config()
    assert (c.kernel, c.items_per_thread, c.nontemporal) == (cmi.CSR_STREAM_WAVEV, 1, 3), c
    assert plan.shifted_tiles() == 0 and plan.device_bytes() < 2 * nnz
    _three_ways(cmi, plan, R, dAp, dAj, dAx, dx, tdt, f"toeplitz_5 {tag} without the columns")


def test_shift_tiles_auto_plan_at_the_cache_gate(cmi):
    """poisson5pt(2400, 2400) in f64, the smallest 5-point matrix past the stencil rule's cache gate: the AUTO plan made with the
    columns is still (CSR_STREAM_WAVEV, 1, 3 | 8), marks what the restatement's vectorised count marks, and y equals the stencil's
    closed form (x = 1: 4 minus the number of neighbours)."""
    import torch
    n = 2400
    A = cmi.poisson5pt(n, n, "csr", device=torch.device("cuda", 0))
    N = n * n
    plan = cmi.Plan.csr(torch.float64, N, N, A.row_offsets, A.column_indices)
    c = plan.config()
    assert (c.kernel, c.items_per_thread, c.nontemporal) == (cmi.CSR_STREAM_WAVEV, 1, 3 | COLS16), c
    Ap, Aj = A.row_offsets.cpu().numpy(), A.column_indices.cpu().numpy()
    marked, _, with_entries = sh.table(Ap, Aj, 1)  # (the copy is granted: the config says so)
    assert 4 * int(marked.sum()) >= with_entries and plan.shifted_tiles() == int(marked.sum()) > 0
    x = torch.ones(N, dtype=torch.float64, device="cuda")
    y = torch.full((N,), 9.0, dtype=torch.float64, device="cuda")
    cmi.spmv_csr_plan(plan, A.row_offsets, A.column_indices, A.values, x, y)
    i = torch.arange(n, device="cuda")
    edge = ((i == 0).to(torch.float64) + (i == n - 1).to(torch.float64))
    want = (edge[:, None] + edge[None, :]).reshape(-1)  # 4 - neighbours: 0 inside, 1 on an edge, 2 in a corner
    assert torch.equal(y, want)
