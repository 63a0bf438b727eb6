"""csr_wavev reading the plan's 16-bit column copy on an MI355X (cfg.nontemporal bit 8).  Every case of tests/cols16_refs.py
(tests/test_cols16_refs.py shows what each contains) runs through an explicit CSR_STREAM_WAVEV config with the bit in f64 and f32
at V = 1, 2, 4, plain, accumulating onto a seeded y and through the fused <y, w> entry of the CG loop; y must have the oracle host
loop's bits (reference arithmetic: cusp/system/detail/sequential/multiply/csr_spmv.h:42-74), the dot the fused-dot tolerance of
tests/test_round4_gpu.py against math.fsum.  The plan's config carries the bit exactly where the numpy restatement grants the copy;
a refused plan multiplies through the 32-bit kernel, with the same bits."""
import math

import numpy as np
import pytest

import cols16_refs as c16
import special_values as sv

pytestmark = pytest.mark.gpu

COLS16 = 8  # the memory-policy bit: csr_wavev reads the plan's 16-bit column copy
_REF = {}


def reference(orc, name, V, tag):
    """Inputs and the host loop's results of a case, computed once and shared (read-only)."""
    key = (name, V if name == "opposite_ends" else 0, tag)
    if key not in _REF:
        dtype = np.float64 if tag == "f64" else np.float32
        Ap, Aj, cols = c16.structure(name, V)
        Ax, x, y0, w = c16.vectors(name, V, dtype)
        want, want_acc = orc.spmv_csr(Ap, Aj, Ax, x), orc.spmv_csr(Ap, Aj, Ax, x, y0.copy())
        prod = (want.astype(np.float64) * w.astype(np.float64)).tolist()
        item = dict(Ap=Ap, Aj=Aj, cols=cols, Ax=Ax, x=x, y0=y0, w=w, want=want, want_acc=want_acc, dot=math.fsum(prod),
                    dot_abs=math.fsum(map(abs, prod)))
        for v in item.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = item
    return _REF[key]


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared references stay read-only)


def _three_ways(cmi, plan, R, dAp, dAj, dAx, dx, tdt, what):
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
    assert abs(res.item() - R["dot"]) <= 1e-9 * R["dot_abs"] + 1e-300, (what, res.item(), R["dot"])


@pytest.mark.parametrize("V", c16.V_ALL)
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_cols16_bit_exact(cmi, orc, tag, V):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    tdt = torch.float64 if tag == "f64" else torch.float32
    for name in c16.CASES:
        R = reference(orc, name, V, tag)
        Ap, Aj = R["Ap"], R["Aj"]
        rows, cols, nnz = len(Ap) - 1, R["cols"], int(Ap[-1])
        granted = c16.encode(Ap, Aj, V)[0]
        assert granted == (name not in c16.REFUSED)
        what = f"{name} {tag} V={V} ({'granted' if granted else 'refused'})"
        dAp, dAj, dAx, dx = _dev(Ap), _dev(Aj), _dev(R["Ax"]), _dev(R["x"])
        plain = cmi.Plan.csr(tdt, rows, cols, dAp, dAj, cfg=cmi.Config(kernel=cmi.CSR_STREAM_WAVEV, items_per_thread=V, nontemporal=3))
        plan = cmi.Plan.csr(tdt, rows, cols, dAp, dAj, cfg=cmi.Config(kernel=cmi.CSR_STREAM_WAVEV, items_per_thread=V, nontemporal=3 | COLS16))
        c, c0 = plan.config(), plain.config()
        assert (c.kernel, c.items_per_thread, c.nontemporal & 3) == (cmi.CSR_STREAM_WAVEV, V, 3), (what, c)
        assert (c0.kernel, c0.items_per_thread, c0.nontemporal) == (cmi.CSR_STREAM_WAVEV, V, 3), (what, c0)
        assert bool(c.nontemporal & COLS16) == granted, (what, c.nontemporal)
        # the copy is counted: two bytes per entry and four per tile, or nothing at all
        grown = plan.device_bytes() - plain.device_bytes()
        assert (grown >= 2 * nnz) if granted else (grown == 0), (what, grown)
        # ... and guarded: the plan is made from the columns, so it validates against them
        assert plan.validate(dAp, dAj), what
        _three_ways(cmi, plan, R, dAp, dAj, dAx, dx, tdt, what)


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_cols16_policy_bits_and_bit_alone(cmi, orc, tag):
    """The bit with every cache policy, and the bit alone (the policy is then the plan's own choice)."""
    import torch
    tdt = torch.float64 if tag == "f64" else torch.float32
    name, V = "poisson5pt_9x451", 1
    R = reference(orc, name, V, tag)
    rows, cols = len(R["Ap"]) - 1, R["cols"]
    dAp, dAj, dAx, dx = _dev(R["Ap"]), _dev(R["Aj"]), _dev(R["Ax"]), _dev(R["x"])
    for pol in (0, 1, 2, 3):
        plan = cmi.Plan.csr(tdt, rows, cols, dAp, dAj, cfg=cmi.Config(kernel=cmi.CSR_STREAM_WAVEV, items_per_thread=V, nontemporal=pol | COLS16))
        c = plan.config()
        assert c.nontemporal & COLS16 and (pol == 0 or (c.nontemporal & 3) == pol), (pol, c.nontemporal)
        _three_ways(cmi, plan, R, dAp, dAj, dAx, dx, tdt, f"{name} {tag} policy {pol} + 8")


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_cols16_needs_the_columns(cmi, orc, tag):
    """A plan made from the row offsets alone, asked for the bit: cleared, and y exact through the 32-bit kernel."""
    import torch
    tdt = torch.float64 if tag == "f64" else torch.float32
    for name, V in (("poisson5pt_9x451", 1), ("rows_1_16_band_2000", 2)):
        R = reference(orc, name, V, tag)
        rows, cols, nnz = len(R["Ap"]) - 1, R["cols"], int(R["Ap"][-1])
        dAp, dAj, dAx, dx = _dev(R["Ap"]), _dev(R["Aj"]), _dev(R["Ax"]), _dev(R["x"])
        plan = cmi.Plan(cmi.FORMAT_CSR, tdt, rows, cols, nnz, dAp, cmi.Config(kernel=cmi.CSR_STREAM_WAVEV, items_per_thread=V, nontemporal=3 | COLS16))
        c = plan.config()
        assert (c.kernel, c.items_per_thread, c.nontemporal) == (cmi.CSR_STREAM_WAVEV, V, 3), c
        assert plan.device_bytes() < 2 * nnz
        _three_ways(cmi, plan, R, dAp, dAj, dAx, dx, tdt, f"{name} {tag} V={V} without the columns")


def test_cols16_plan_is_stale_after_a_column_edit(cmi, orc):
    import torch
    R = reference(orc, "rows_1_16_band_2000", 1, "f64")
    rows, cols = len(R["Ap"]) - 1, R["cols"]
    dAp, dAj = _dev(R["Ap"]), _dev(R["Aj"])
    plan = cmi.Plan.csr(torch.float64, rows, cols, dAp, dAj, cfg=cmi.Config(kernel=cmi.CSR_STREAM_WAVEV, items_per_thread=1, nontemporal=3 | COLS16))
    assert plan.config().nontemporal & COLS16 and plan.validate(dAp, dAj)
    e = len(R["Aj"]) // 2
    dAj[e] = (int(R["Aj"][e]) + 1) % cols  # one column, in place
    assert not plan.validate(dAp, dAj)
    dAj[e] = int(R["Aj"][e])
    assert plan.validate(dAp, dAj)
    # a plan without the copy holds nothing derived from the columns: the same edit leaves it valid
    plain = cmi.Plan.csr(torch.float64, rows, cols, dAp, dAj, cfg=cmi.Config(kernel=cmi.CSR_STREAM_WAVEV, items_per_thread=1, nontemporal=3))
    dAj[e] = (int(R["Aj"][e]) + 1) % cols
    assert plain.validate(dAp, dAj)


def test_cols16_auto_plan_at_the_cache_gate(cmi):
    """The smallest 5-point matrix that passes the stencil rule's cache gate, poisson5pt(2400, 2400) in f64 (28.8 M entries, 345 MB of
    streams against the gate's 335.5 MB): an AUTO plan made with the columns takes the copy by itself, one made from the row offsets
    alone does not, and both y equal the stencil's closed form (x = 1: 4 minus the number of neighbours)."""
    import torch
    n = 2400
    A = cmi.poisson5pt(n, n, "csr", device=torch.device("cuda", 0))
    N, nnz = n * n, A.column_indices.numel()
    with_cols = cmi.Plan.csr(torch.float64, N, N, A.row_offsets, A.column_indices)
    without = cmi.Plan(cmi.FORMAT_CSR, torch.float64, N, N, nnz, A.row_offsets)
    c, c0 = with_cols.config(), without.config()
    assert (c.kernel, c.items_per_thread, c.nontemporal) == (cmi.CSR_STREAM_WAVEV, 1, 3 | COLS16), c
    assert (c0.kernel, c0.items_per_thread, c0.nontemporal) == (cmi.CSR_STREAM_WAVEV, 1, 3), c0
    assert with_cols.device_bytes() - without.device_bytes() >= 2 * nnz
    x = torch.ones(N, dtype=torch.float64, device="cuda")
    y, y0 = torch.full((N,), 9.0, dtype=torch.float64, device="cuda"), torch.full((N,), 9.0, dtype=torch.float64, device="cuda")
    cmi.spmv_csr_plan(with_cols, A.row_offsets, A.column_indices, A.values, x, y)
    cmi.spmv_csr_plan(without, A.row_offsets, A.column_indices, A.values, x, y0)
    i = torch.arange(n, device="cuda")
    edge = ((i == 0).to(torch.float64) + (i == n - 1).to(torch.float64))
    want = (edge[:, None] + edge[None, :]).reshape(-1)  # 4 - neighbours: 0 inside, 1 on an edge, 2 in a corner
    assert torch.equal(y, y0) and torch.equal(y, want)
