"""csr_wavev's constant tiles on an MI355X: a marked tile whose rows all hold the first row's values is multiplied from that one row, read live
from the caller's array.  Plans are made with the values (Plan.csr_values): on small matrices through the explicit CSR_STREAM_WAVEV config with
nontemporal 3 | 8 (f64 at V = 1, f32 at V = 2 -- the AUTO route's shapes), on poisson5pt 2400 x 2400 -- the smallest 5-point matrix past the
stencil rule's cache gate -- through the container's multiply_plan().  y is compared bit for bit with the oracle host loop, plain,
accumulating and with the fused <y, w>; the plan's count of constant tiles is the restatement's (tests/const_tiles_refs.py) exactly when the
restatement keeps the marks, and its device bytes grow by one bit per tile exactly then."""
import math

import numpy as np
import pytest

import const_tiles_refs as ct
import shift_tiles_refs as sh
import special_values as sv
import uniform_tiles_refs as ut
from test_cols16_gpu import COLS16, _dev, _three_ways

pytestmark = pytest.mark.gpu

TAGS = {"f64": (np.float64, 1), "f32": (np.float32, 2)}  # value type -> (numpy type, V of the AUTO route)
_REF = {}


def _torch():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch


def _cfg(cmi, V):
    return cmi.Config(kernel=cmi.CSR_STREAM_WAVEV, items_per_thread=V, nontemporal=3 | COLS16)


def _reference(orc, key, build):
    """Inputs and the host loop's results of a case, computed once and shared (read-only).  build() -> (Ap, Aj, cols, Ax, x)."""
    if key not in _REF:
        Ap, Aj, cols, Ax, x = build()
        rows = len(Ap) - 1
        rng = np.random.default_rng(2701)
        y0, w = rng.standard_normal(rows).astype(Ax.dtype), rng.standard_normal(rows).astype(Ax.dtype)
        want, want_acc = orc.spmv_csr(Ap, Aj, Ax, x), orc.spmv_csr(Ap, Aj, Ax, x, y0.copy())
        prod = (want.astype(np.float64) * w.astype(np.float64)).tolist()
        finite = bool(np.isfinite(want).all())
        item = dict(Ap=Ap, Aj=Aj, cols=cols, Ax=Ax, x=x, y0=y0, w=w, want=want, want_acc=want_acc, dot=math.fsum(prod) if finite else None,
                    dot_abs=math.fsum(map(abs, prod)) if finite else None)
        for v in item.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = item
    return _REF[key]


def _toeplitz_case(orc, rows, L, tag, values="constant"):
    dtype, V = TAGS[tag]

    def build():
        Ap, Aj, cols, first = ct.toeplitz(rows, L, dtype)
        Ax = ct.constant_values(rows, first)
        if values == "last_bit":  # the second tile's last row differs from the others in one value's last bit (one tile: the only tile's last row)
            t = 1 if len(ut.partition(Ap, V)[1]) - 1 > 1 else 0
            e = L * (ct.tile_rows(Ap, V, t)[1] - 1) + L // 2
            w = ct.bits(Ax).copy()
            w[e] ^= 1
            Ax = w.view(dtype)
        x = np.random.default_rng(2702 + L).standard_normal(cols).astype(dtype)
        return Ap, Aj, cols, Ax, x
    return _reference(orc, (rows, L, tag, values), build)


def _plan_and_check(cmi, R, tag, what, want_kept=None):
    """Makes the plan with the values, checks its counts against the restatement and its three multiplies against the host loop; returns it."""
    torch = _torch()
    dtype, V = TAGS[tag]
    tdt = torch.float64 if tag == "f64" else torch.float32
    rows, cols = len(R["Ap"]) - 1, R["cols"]
    dAp, dAj, dAx, dx = _dev(R["Ap"]), _dev(R["Aj"]), _dev(R["Ax"]), _dev(R["x"])
    plan = cmi.Plan.csr_values(rows, cols, dAp, dAj, dAx, cfg=_cfg(cmi, V))
    without = cmi.Plan.csr(tdt, rows, cols, dAp, dAj, cfg=_cfg(cmi, V))
    keep, n = ct.kept(R["Ap"], R["Aj"], R["Ax"], V)
    if want_kept is not None:
        assert keep == want_kept, what
    c = plan.config()
    assert (c.kernel, c.items_per_thread, c.nontemporal) == (cmi.CSR_STREAM_WAVEV, V, 3 | COLS16), (what, c)  # (no bit, no kernel of its own)
    assert plan.const_tiles() == (n if keep else 0) and plan.info().get("constant_tiles", 0) == (n if keep else 0), (what, plan.const_tiles(), n, keep)
    assert without.const_tiles() == 0 and "constant_tiles" not in without.info() and plan.shifted_tiles() == without.shifted_tiles(), what
    assert plan.device_bytes() - without.device_bytes() == (ct.mark_bytes(R["Ap"], V) if keep else 0), what
    assert plan.validate_values(dAx) and without.validate_values(dAx), what
    if R["dot"] is not None:
        _three_ways(cmi, plan, R, dAp, dAj, dAx, dx, tdt, what)
    else:  # NaN / inf in y: no dot to compare, y by its bits in all three calls
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
    return plan, (dAp, dAj, dAx, dx)


@pytest.mark.parametrize("tag", list(TAGS))
@pytest.mark.parametrize("rows", [1, 63, 64, 65])
def test_one_tile_of_few_rows(cmi, orc, tag, rows):
    _plan_and_check(cmi, _toeplitz_case(orc, rows, 5, tag), tag, f"one tile of {rows} rows {tag}", want_kept=True)


@pytest.mark.parametrize("tag", list(TAGS))
@pytest.mark.parametrize("L", [1, 2, 3, 5, 7, 8])
def test_rows_of_L_over_1001_rows(cmi, orc, tag, L):
    """L <= 3: tiles of more than 64 rows (several turns of the row loop; x is loaded per turn, the values are kept).  1001 L entries: for odd L
    the last tile's last vector reaches past the arrays' end, so that tile -- constant or not -- sums straight from the arrays."""
    R = _toeplitz_case(orc, 1001, L, tag)
    nr = np.diff(ut.partition(R["Ap"], TAGS[tag][1])[0])
    assert (nr.max() > 64) == (L <= 3 or (tag == "f32" and L <= 7)), (L, tag, int(nr.max()))
    _plan_and_check(cmi, R, tag, f"rows of {L} {tag}", want_kept=True)


@pytest.mark.parametrize("tag", list(TAGS))
def test_a_constant_tile_beside_one_whose_last_row_differs_in_a_last_bit(cmi, orc, tag):
    R = _toeplitz_case(orc, 1001, 5, tag, "last_bit")
    const = ct.marks(R["Ap"], R["Aj"], R["Ax"], TAGS[tag][1])[0]
    assert const[0] and not const[1] and const.sum() == len(const) - 1
    plan, _ = _plan_and_check(cmi, R, tag, f"last bit {tag}", want_kept=True)
    assert plan.const_tiles() == len(const) - 1


@pytest.mark.parametrize("tag", list(TAGS))
def test_special_values_and_guard_cells(cmi, orc, tag):
    """Tiles whose constant rows hold +0 / -0, +inf / -inf, NaN; x holds 0, inf and -inf too, and NaN in the cells no row refers to (a row lane
    that read outside its tile's true columns, or a lane without a row that stored, would show)."""
    dtype, V = TAGS[tag]

    def build():
        rows, L = 1001, 5
        lens, Aj, cols = sh._toeplitz(L, rows=rows, first_col=20, cols=rows + 20 + 12 + 9)(V)
        Ap = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
        row_start = ut.partition(Ap, V)[0]
        palette = np.array([[0.0, -0.0, 1.5, -2.0, 3.0], [np.inf, 1.0, -np.inf, 2.0, 0.5], [1.0, np.nan, 2.0, -0.0, 0.0], [-0.0, -0.0, 0.0, 0.0, -0.0],
                            [0.25, -np.inf, 4.0, np.inf, -1.0]], dtype)
        Ax = np.empty(rows * L, dtype)
        for t in range(len(row_start) - 1):
            a, e = int(row_start[t]), int(row_start[t + 1])
            Ax[L * a:L * e] = np.tile(palette[t % len(palette)], e - a)
        x = np.random.default_rng(2703).standard_normal(cols).astype(dtype)
        x[40::97], x[41::193], x[42::389], x[43::211] = 0.0, np.inf, -np.inf, -0.0
        used = np.zeros(cols, bool)
        used[Aj] = True
        assert (~used).sum() >= 16 and not used[:11].any() and not used[-8:].any()
        x[~used] = np.nan
        return Ap, Aj, cols, Ax, x
    R = _reference(orc, ("special", tag), build)
    assert np.isnan(R["want"]).any() and np.isinf(R["want"]).any() and np.isfinite(R["want"]).any()
    plan, _ = _plan_and_check(cmi, R, tag, f"special values {tag}", want_kept=True)
    assert plan.const_tiles() == len(ut.partition(R["Ap"], V)[1]) - 1


@pytest.mark.parametrize("tag", list(TAGS))
def test_tile_that_ends_at_the_arrays_last_vector(cmi, orc, tag):
    """1000 rows of 4 and of 8: the last tile's last vector is the arrays' last, exactly (the constant body runs on it)."""
    for L in (4, 8):
        R = _toeplitz_case(orc, 1000, L, tag)
        assert int(R["Ap"][-1]) % 4 == 0
        _plan_and_check(cmi, R, tag, f"ends at the last vector L={L} {tag}", want_kept=True)


@pytest.mark.parametrize("tag", list(TAGS))
def test_below_the_quarter_nothing_is_kept(cmi, orc, tag):
    """Every tile shift-invariant, one tile short of a quarter constant: info() reports no constant tiles, the bytes are the plan's without the
    values, and y is exact."""
    dtype, V = TAGS[tag]

    def build():
        Ap, Aj, cols, first = ct.toeplitz(3003, 5, dtype)
        row_start, nz, _, _ = ut.partition(Ap, V)
        m = (int((np.diff(nz) > 0).sum()) + 3) // 4 - 1
        assert m >= 1
        Ax = np.random.default_rng(2704).standard_normal(len(Aj)).astype(dtype)
        Ax[:5 * int(row_start[m])] = ct.constant_values(int(row_start[m]), first)
        return Ap, Aj, cols, Ax, np.random.default_rng(2705).standard_normal(cols).astype(dtype)
    R = _reference(orc, ("under", tag), build)
    plan, _ = _plan_and_check(cmi, R, tag, f"below the quarter {tag}", want_kept=False)
    assert plan.info().get("constant_tiles", 0) == 0


def test_uniform_edit_in_place_needs_no_rebuild_and_a_hidden_edit_is_caught(cmi, orc):
    """values.mul_(2): the same plan gives the doubled matrix's bits and still validates.  One value changed through a view that does not share
    torch's version counter: validate_values says so; after drop_const_tiles() the plan multiplies the edited matrix exactly."""
    torch = _torch()
    R = _toeplitz_case(orc, 1001, 5, "f64")
    plan, (dAp, dAj, dAx, dx) = _plan_and_check(cmi, R, "f64", "before the edits", want_kept=True)
    rows = len(R["Ap"]) - 1
    y = torch.full((rows,), 9.0, dtype=torch.float64, device="cuda")
    dAx.mul_(2)
    cmi.spmv_csr_plan(plan, dAp, dAj, dAx, dx, y)
    sv.same_bits(y.cpu().numpy(), orc.spmv_csr(R["Ap"], R["Aj"], 2 * R["Ax"], R["x"]), "values.mul_(2)")
    assert plan.validate_values(dAx) and plan.const_tiles() > 0
    version = dAx._version
    e = 5 * 500 + 2
    dAx.data[e] = 0.375
    assert dAx._version == version, "the edit was meant to be invisible to torch"
    assert not plan.validate_values(dAx) and plan.const_tiles() > 0  # (validation tells; it changes nothing)
    edited = 2 * R["Ax"]
    edited[e] = 0.375
    plan.drop_const_tiles()
    assert plan.const_tiles() == 0 and "constant_tiles" not in plan.info() and plan.validate_values(dAx)
    cmi.spmv_csr_plan(plan, dAp, dAj, dAx, dx, y)
    sv.same_bits(y.cpu().numpy(), orc.spmv_csr(R["Ap"], R["Aj"], edited, R["x"]), "after drop_const_tiles")
    plan.drop_const_tiles()  # (a plan without marks: nothing happens)


def test_captured_multiply_replays(cmi, orc):
    torch = _torch()
    R = _toeplitz_case(orc, 1001, 5, "f64")
    rows, cols = len(R["Ap"]) - 1, R["cols"]
    dAp, dAj, dAx, dx = _dev(R["Ap"]), _dev(R["Aj"]), _dev(R["Ax"]), _dev(R["x"])
    plan = cmi.Plan.csr_values(rows, cols, dAp, dAj, dAx, cfg=_cfg(cmi, 1))
    assert plan.const_tiles() > 0
    y = torch.full((rows,), 7.0, dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        cmi.spmv_csr_plan(plan, dAp, dAj, dAx, dx, y, stream=side)
    for scale in (1.0, 2.0):  # the second replay reads the values as they are THEN: a uniform edit needs no new capture
        y.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        sv.same_bits(y.cpu().numpy(), orc.spmv_csr(R["Ap"], R["Aj"], scale * R["Ax"], R["x"]), f"replay, values x {scale}")
        dAx.mul_(2)


# ---- the AUTO plan and the container: poisson5pt 2400 x 2400, the smallest 5-point matrix past the stencil rule's cache gate -------------
N_GATE = 2400


def _closed_form(torch, scale=1.0):
    """A x for x = 1 on the 5-point stencil: (4 - neighbours) x scale -- 0 inside, 1 on an edge, 2 in a corner."""
    i = torch.arange(N_GATE, device="cuda")
    edge = ((i == 0).to(torch.float64) + (i == N_GATE - 1).to(torch.float64))
    return (edge[:, None] + edge[None, :]).reshape(-1) * scale


def _interior_entry(A):
    """(row, entry) of the diagonal value of a row in the middle of the grid: inside a constant tile."""
    row = (N_GATE // 2) * N_GATE + N_GATE // 2
    return row, int(A.row_offsets[row].item()) + 2


def test_container_validates_after_an_edit_and_drops_the_marks_when_it_must(cmi, monkeypatch):
    """multiply() goes through multiply_plan(): the plan made with the values, bound to them by address and version.  plan() stays the plan of
    the structure, without marks, for callers who pass values of their own to spmv_csr_plan."""
    torch = _torch()
    monkeypatch.delenv("CMI_CSR_CONST_TILES", raising=False)
    A = cmi.poisson5pt(N_GATE, N_GATE, "csr", device=torch.device("cuda", 0))
    N = N_GATE * N_GATE
    x = torch.ones(N, dtype=torch.float64, device="cuda")
    y = torch.full((N,), 9.0, dtype=torch.float64, device="cuda")
    cmi.multiply(A, x, y)
    assert A._plan is None  # (the structure plan is made when somebody asks for it)
    plan = A.multiply_plan()
    c = plan.config()
    assert (c.kernel, c.items_per_thread, c.nontemporal) == (cmi.CSR_STREAM_WAVEV, 1, 3 | COLS16), c
    n = plan.const_tiles()
    assert 0 < n <= plan.shifted_tiles() and plan.info()["constant_tiles"] == n and 4 * n >= plan.shifted_tiles()
    without = A.plan()
    assert without is not plan and without.const_tiles() == 0 and "constant_tiles" not in without.info()
    assert without.config().as_dict() == c.as_dict() and without.shifted_tiles() == plan.shifted_tiles()
    assert plan.device_bytes() - without.device_bytes() == ct.mark_bytes(A.row_offsets.cpu().numpy(), 1)
    assert torch.equal(y, _closed_form(torch))
    key, held = A._plan_args
    assert held is plan and len(key) == 11 and key[:9] == A._plan_key and key[-2:] == (A.values.data_ptr(), A.values._version)
    # plan() serves ANY values: another array through it, bit for bit what the marks-free kernel gives
    other = A.values * (1.0 + torch.arange(A.num_entries, dtype=torch.float64, device="cuda") / A.num_entries)
    y2 = torch.empty_like(y)
    cmi.spmv_csr_plan(without, A.row_offsets, A.column_indices, other, x, y)
    cmi.spmv_csr(N, N, A.row_offsets, A.column_indices, other, x, y2, cfg=cmi.Config(kernel=cmi.CSR_SCALAR))
    assert torch.equal(y, y2)
    # a uniform edit through torch: validated at the next multiply, the plan and its marks stay
    A.values.mul_(2)
    cmi.multiply(A, x, y)
    assert A.multiply_plan() is plan and plan.const_tiles() == n and A._plan_args[0][-1] == A.values._version
    assert torch.equal(y, _closed_form(torch, 2.0))
    # a copy of the container that resets its plan fields (what a benchmark's cold sets do) makes a plan of its own, marks included
    import copy
    B2 = copy.copy(A)
    B2._plan = B2._plan_key = B2._plan_args = None
    cmi.multiply(B2, x, y)
    assert B2.multiply_plan() is not plan and B2.multiply_plan().const_tiles() == n and torch.equal(y, _closed_form(torch, 2.0))
    # one value edited through torch: the container validates, drops the marks, keeps the plan; later edits cost nothing
    row, e = _interior_entry(A)
    A.values[e] = 11.0
    cmi.multiply(A, x, y)
    want = _closed_form(torch, 2.0)
    want[row] = 11.0 - 8.0  # the diagonal 8 became 11, the four neighbours stay -2
    assert plan.const_tiles() == 0 and A._plan_args == (A._plan_key, None) and A.multiply_plan() is A.plan() is without
    assert torch.equal(y, want)
    A.values[e] = 8.0
    cmi.multiply(A, x, y)
    assert A.multiply_plan() is without and torch.equal(y, _closed_form(torch, 2.0))
    A.invalidate()
    assert A._plan is None and A._plan_args is None


def test_switch_off_is_the_plan_without_the_values(cmi, monkeypatch):
    torch = _torch()
    monkeypatch.setenv("CMI_CSR_CONST_TILES", "0")
    A = cmi.poisson5pt(N_GATE, N_GATE, "csr", device=torch.device("cuda", 0))
    N = N_GATE * N_GATE
    x = torch.ones(N, dtype=torch.float64, device="cuda")
    y = torch.full((N,), 9.0, dtype=torch.float64, device="cuda")
    cmi.multiply(A, x, y)
    plan = A.multiply_plan()
    assert plan is A.plan() is A._plan and A._plan_args is None
    without = cmi.Plan.csr(torch.float64, N, N, A.row_offsets, A.column_indices)
    assert plan.const_tiles() == 0 and plan.shifted_tiles() == without.shifted_tiles() > 0 and len(A._plan_key) == 9
    assert plan.config().as_dict() == without.config().as_dict() and plan.device_bytes() == without.device_bytes() and plan.info() == without.info()
    assert torch.equal(y, _closed_form(torch))


def test_small_matrix_through_the_container(cmi, orc):
    """poisson5pt 70 x 40 through the container: below the stencil route's gate the AUTO plan keeps no shift table, so no marks; the call made
    with the values gives the plan Plan.csr gives, and y is exact."""
    torch = _torch()
    Ap, Aj, Ax = orc.poisson5pt_csr(70, 40)
    n = 70 * 40
    x = np.random.default_rng(2706).standard_normal(n)
    A = cmi.poisson5pt(70, 40, "csr", device=torch.device("cuda", 0))
    y = torch.full((n,), 9.0, dtype=torch.float64, device="cuda")
    cmi.multiply(A, _dev(x), y)
    sv.same_bits(y.cpu().numpy(), orc.spmv_csr(Ap, Aj, Ax, x), "poisson5pt 70 x 40")
    without = cmi.Plan.csr(torch.float64, n, n, A.row_offsets, A.column_indices)
    assert A.multiply_plan() is A.plan() and A.plan().const_tiles() == 0  # no marks: one plan
    assert A.plan().config().as_dict() == without.config().as_dict() and A.plan().info() == without.info()
    # ... and with the marks, through the explicit config: the boundary rows' tiles are not constant, the interior's are
    plan = cmi.Plan.csr_values(n, n, A.row_offsets, A.column_indices, A.values, cfg=_cfg(cmi, 1))
    keep, want_n = ct.kept(Ap, Aj, Ax, 1)
    assert plan.const_tiles() == (want_n if keep else 0)
    y.fill_(9.0)
    cmi.spmv_csr_plan(plan, A.row_offsets, A.column_indices, A.values, _dev(x), y)
    sv.same_bits(y.cpu().numpy(), orc.spmv_csr(Ap, Aj, Ax, x), "poisson5pt 70 x 40, explicit config")
