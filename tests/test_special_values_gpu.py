"""Every multiply path on IEEE special values (-m gpu), through the C-ABI binding.

The matrices and input decks come from tests/special_values.py (NaN / inf next to the columns a kernel over-fetches, signed zeros,
subnormals, an overflow that only storage order turns into +inf); tests/test_special_values_refs.py proves on the CPU that the decks
can see the bugs they are meant for.  The comparison is same_bits: bit patterns, with NaN positions compared as a set.

EXACT below is the table of paths that claim storage-order sums: every entry must be granted by its plan (a refusal fails the test)
and must return the oracle's bits on all five decks, both value types, y = A x and y += A x.  REASSOCIATED lists the paths that add
in another order: NaNs exactly where the reference has them, finite rows within test_fuzz_gpu.py's bar, and equal VALUES on the two
decks whose sums are exact in any order.
"""
import os
import re

import numpy as np
import pytest

import special_values as sv

pytestmark = pytest.mark.gpu

TAGS = ("f64", "f32")
DT = {"f64": np.float64, "f32": np.float32}
TOL = {np.dtype(np.float64): 1e-6, np.dtype(np.float32): 1e-5}   # tests/test_fuzz_gpu.py's bar: |err| <= TOL * sum_j |a_ij x_j|
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch


# ------------------------------------------------------------------------------------------------
# the table: (name, kernel id, matrices, how to run it).  K(...) is the cmi_config of the case.
# ------------------------------------------------------------------------------------------------
def K(**kw):
    return kw


# how: csr (plan-less), plan (cmi_plan_create: row offsets only), plan_cols (cmi_plan_create_csr), plan_values
# (cmi_plan_create_csr_values), ell, ellr, dia, coo_plan, coo_plan_cols, hyb (one launch, width in the entry)
EXACT = [
    ("csr_scalar", "CSR_SCALAR", ("irregular", "runs"), "csr", K()),
    ("csr_stream one lane", "CSR_STREAM", ("irregular", "runs", "poisson100"), "csr", K(threads_per_row=1)),
    ("csr_stream_pipe", "CSR_STREAM_PIPE", ("irregular", "runs"), "csr", K()),
    ("auto plan", "KERNEL_AUTO", ("poisson100", "runs", "band", "banded"), "plan", K()),
    ("auto plan with columns", "KERNEL_AUTO", ("poisson100", "runs", "band", "banded"), "plan_cols", K()),
    ("csr_wave", "CSR_STREAM_WAVE", ("poisson100",), "plan", K()),
    ("csr_wavev V1", "CSR_STREAM_WAVEV", ("runs",), "plan", K(items_per_thread=1)),
    ("csr_wavev V2", "CSR_STREAM_WAVEV", ("runs",), "plan", K(items_per_thread=2)),
    ("csr_wavev V4", "CSR_STREAM_WAVEV", ("runs", "irregular_short"), "plan", K(items_per_thread=4)),
    ("csr_wavex V2", "CSR_STREAM_WAVEX", ("band",), "plan", K(items_per_thread=2, rows_per_block=2048)),
    ("csr_wavex V4", "CSR_STREAM_WAVEX", ("band",), "plan", K(items_per_thread=4, rows_per_block=2048)),
] + [
    (f"csr_waver V{v} cap{cap}", "CSR_STREAM_WAVER", ("runs",), "plan_cols", K(items_per_thread=v, threads_per_row=cap))
    for v in (1, 2, 4) for cap in (3, 4)
] + [
    ("packed tiles", "CSR_STREAM_PACKED", ("runs",), "plan_values", K()),
    ("16-bit columns", "CSR_STREAM_C16", ("poisson100", "runs"), "plan_cols", K()),
    ("ell one lane", "ELL_ROW", ("poisson100", "runs"), "ell", K(threads_per_row=1, items_per_thread=1)),
    ("ell one lane, two rows", "ELL_ROW", ("poisson100", "runs"), "ell", K(threads_per_row=1, items_per_thread=2)),
    ("ellr", "ELL_ROW", ("poisson100", "runs"), "ellr", K(threads_per_row=1, items_per_thread=1)),
    ("dia", "DIA_ROW", ("poisson100", "banded"), "dia", K(items_per_thread=1)),
    ("dia two rows", "DIA_ROW", ("poisson100", "banded"), "dia", K(items_per_thread=2)),
    ("coo tile", "COO_TILE", ("poisson100", "runs"), "coo_plan", K()),
    ("coo plan (row offsets)", "KERNEL_AUTO", ("poisson100", "runs"), "coo_plan_auto", K()),
    ("hyb width 0", "ELL_ROW", ("poisson100", "runs"), "hyb", K(width=0)),
    ("hyb width 3", "ELL_ROW", ("poisson100", "runs"), "hyb", K(width=3)),
    ("hyb width max", "ELL_ROW", ("poisson100", "runs"), "hyb", K(width=-1)),
]

REASSOCIATED = [
    ("csr_vector 8", "CSR_VECTOR", ("irregular", "runs"), "csr", K(threads_per_row=8)),
    ("csr_vector 32", "CSR_VECTOR", ("irregular", "runs"), "csr", K(threads_per_row=32)),
    ("csr_stream long-row instance", "CSR_STREAM", ("irregular", "runs"), "csr", K(threads_per_row=0)),
    ("csr_stream 4 lanes", "CSR_STREAM", ("irregular", "runs"), "csr", K(threads_per_row=4)),
    ("csr_balanced", "CSR_BALANCED", ("irregular", "runs"), "csr", K()),
    ("the table's choice", "KERNEL_AUTO", ("irregular", "runs", "poisson100"), "csr_table", K()),
    ("ell 4 lanes", "ELL_ROW", ("runs",), "ell", K(threads_per_row=4)),
    ("coo segmented", "COO_SEGMENTED", ("irregular", "runs"), "coo", K()),
    ("coo lane4", "COO_LANE4", ("irregular", "runs"), "coo", K()),
    ("coo unsorted", "KERNEL_AUTO", ("irregular", "runs"), "coo_unsorted", K()),
]

SPMM = [
    ("spmm auto", "KERNEL_AUTO", K()),
    ("spmm rows 1", "CSR_SPMM_ROWS", K(threads_per_row=1)),
    ("spmm rows 8", "CSR_SPMM_ROWS", K(threads_per_row=8)),
    ("spmm cols", "CSR_SPMM_COLS", K()),
]

# fused multiply + dot: entries of EXACT by name (the plain multiply's path), run through the *_dot entry point of their format
DOT = ["csr_scalar", "csr_stream one lane", "auto plan", "auto plan with columns", "csr_wave", "csr_wavev V2", "csr_wavex V4",
       "csr_waver V4 cap3", "packed tiles", "16-bit columns", "ell one lane", "ellr", "dia", "coo plan (row offsets)",
       "hyb width 0", "hyb width 3", "hyb width max"]


def test_table_names_every_kernel(cmi):
    """Every kernel id of enum cmi_kernel (include/cusp_mi355x.h) = every kernel constant of the binding has a special-value case."""
    b = cmi.binding
    header = open(os.path.join(ROOT, "include", "cusp_mi355x.h")).read()
    enum = re.search(r"typedef enum cmi_kernel \{(.*?)\} cmi_kernel;", header, re.S).group(1)
    in_header = {name: int(v) for name, v in re.findall(r"\bCMI_((?:KERNEL|CSR|ELL|DIA|COO)_[A-Z0-9_]+) = (\d+)", enum)}
    in_binding = {n: getattr(b, n) for n in dir(b) if re.fullmatch(r"(KERNEL_AUTO|(CSR|ELL|DIA|COO)_[A-Z0-9_]+)", n) and isinstance(getattr(b, n), int)}
    assert in_header == in_binding and len(in_header) >= 19
    in_table = {k for _, k, *_ in EXACT + REASSOCIATED} | {k for _, k, _ in SPMM}
    assert in_table == set(in_binding), set(in_binding) ^ in_table
    assert set(DOT) <= {name for name, *_ in EXACT}


# ------------------------------------------------------------------------------------------------
# inputs and references, made once
# ------------------------------------------------------------------------------------------------
_cache = {}


def matrix(name, tag):
    if name == "irregular_short":
        key = (name, tag)
        if key not in _cache:
            _cache[key] = sv.without_long_rows(sv.matrices(DT[tag])["irregular"], 500)
        return _cache[key]
    return sv.matrices(DT[tag])[name]


def deck(name, tag, dname):
    key = ("deck", name, tag)
    if key not in _cache:
        _cache[key] = sv.decks(matrix(name, tag), DT[tag])
    return _cache[key][dname]


class Inputs:
    """One (matrix, type, deck) on the host in every format, with the oracle's results; device copies are made per use."""

    def __init__(self, orc, name, tag, dname):
        self.orc, self.M, self.tag, self.dname = orc, matrix(name, tag), tag, dname
        self.Ax, self.x, self.y0 = deck(name, tag, dname)
        self.what = f"{name} {dname} {tag}"
        self._fmt = {}

    def want(self, accumulate, fmt="csr", width=None):
        """The oracle's host loop of the format the kernel replaces (DIA: every in-range slot, explicit zeros included)."""
        key = ("want", fmt, width, accumulate)
        if key not in self._fmt:
            M, y0 = self.M, self.y0 if accumulate else None
            if fmt == "dia":
                pitch, off, vals = self.dia()
                r = self.orc.spmv_dia(M.rows, M.cols, pitch, off, vals, self.x, y0)
            else:  # CSR, COO, ELL, HYB: the same chain per row (asserted on the CPU by test_special_values_refs.py)
                r = self.orc.spmv_csr(M.Ap, M.Aj, self.Ax, self.x, y0)
            self._fmt[key] = r
        return self._fmt[key]

    def ell(self):
        if "ell" not in self._fmt:
            width = int(self.M.row_lengths().max())
            self._fmt["ell"] = (width,) + self.orc.csr_to_ell(self.M.Ap, self.M.Aj, self.Ax, width)
        return self._fmt["ell"]

    def hyb(self, width):
        if ("hyb", width) not in self._fmt:
            self._fmt[("hyb", width)] = self.orc.csr_to_hyb(self.M.Ap, self.M.Aj, self.Ax, width)
        return self._fmt[("hyb", width)]

    def dia(self):
        if "dia" not in self._fmt:
            self._fmt["dia"] = self.orc.csr_to_dia(self.M.rows, self.M.cols, self.M.Ap, self.M.Aj, self.Ax)
        return self._fmt["dia"]


def inputs(orc, name, tag, dname):
    key = ("in", name, tag, dname)
    if key not in _cache:
        _cache[key] = Inputs(orc, name, tag, dname)
    return _cache[key]


def dev(a, torch):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def config(b, kernel, kw):
    return b.Config(kernel=getattr(b, kernel), **{k: v for k, v in kw.items() if k != "width"})


class Runner:
    """One table entry bound to one Inputs: builds what the path needs once (device arrays, the plan -- asserting that the plan
    grants the kernel and declares storage-order sums where `exact`), then multiplies any number of times."""

    def __init__(self, cmi, torch, I, entry, exact, monkeypatch):
        self.b, self.torch, self.I = cmi.binding, torch, I
        b, M = self.b, I.M
        self.name, self.kernel, _, self.how, self.kw = entry
        self.what = f"{self.name}: {I.what}"
        self.fmt = "dia" if self.how == "dia" else "csr"
        self.dx = dev(I.x, torch)
        self.tdt = self.dx.dtype
        cfg = None if self.kernel == "KERNEL_AUTO" else config(b, self.kernel, self.kw)
        self.cfg, self.plan = cfg, None
        how = self.how
        if how in ("csr", "csr_table", "plan", "plan_cols", "plan_values"):
            self.dAp, self.dAj, self.dAx = dev(M.Ap, torch), dev(M.Aj, torch), dev(I.Ax, torch)
            if how == "plan":
                self.plan = b.Plan(b.FORMAT_CSR, self.tdt, M.rows, M.cols, M.nnz, self.dAp, cfg)
            elif how == "plan_cols":
                self.plan = b.Plan.csr(self.tdt, M.rows, M.cols, self.dAp, self.dAj, cfg=cfg)
            elif how == "plan_values":
                self.plan = b.Plan.csr_values(M.rows, M.cols, self.dAp, self.dAj, self.dAx, cfg=cfg)
        elif how in ("ell", "ellr"):
            self.width, self.pitch, eAj, eAx = I.ell()
            self.deAj, self.deAx = dev(eAj, torch), dev(eAx, torch)
            self.rl = dev(M.row_lengths().astype(np.int32), torch) if how == "ellr" else None
        elif how == "dia":
            self.pitch, off, vals = I.dia()
            self.doff, self.dvals = dev(off, torch), dev(vals, torch)
        elif how in ("coo", "coo_plan", "coo_plan_auto", "coo_unsorted"):
            order = np.random.default_rng(7).permutation(M.nnz) if how == "coo_unsorted" else np.arange(M.nnz)
            self.order = order
            self.dAi, self.dAj, self.dAx = dev(M.Ai[order], torch), dev(M.Aj[order], torch), dev(I.Ax[order], torch)
            if how.startswith("coo_plan"):
                self.plan = b.Plan(b.FORMAT_COO, self.tdt, M.rows, M.cols, M.nnz, self.dAi, cfg)
                assert self.plan.info()["coo_sorted"] is True, self.what
        elif how == "hyb":
            self.width = int(M.row_lengths().max()) if self.kw["width"] < 0 else self.kw["width"]
            self.pitch, eAj, eAx, cAi, cAj, cAx = I.hyb(self.width)
            self.h = [dev(a, torch) for a in (eAj, eAx, cAi, cAj, cAx)]
            monkeypatch.setenv("CMI_HYB_ONE_LAUNCH", "1")   # read when the plan is made: one launch whatever the COO part weighs
            self.plan = b.Plan.hyb(self.tdt, M.rows, M.cols, self.width, self.h[2], cfg_ell=b.Config(kernel=b.ELL_ROW, threads_per_row=1))
            monkeypatch.delenv("CMI_HYB_ONE_LAUNCH")
            assert self.plan.hyb_launches() == 1, self.what + ": the plan refused the one-launch kernel"
        else:
            raise AssertionError(how)
        if self.plan is not None and exact:
            if self.kernel != "KERNEL_AUTO" and how != "hyb":
                got = self.plan.config().kernel
                assert got == getattr(b, self.kernel), f"{self.what}: the plan refused the kernel it was listed for (runs kernel {got})"
            assert self.plan.info()["storage_order_sums"], self.what + ": the plan does not declare storage-order sums"

    def y_start(self, accumulate):
        if accumulate:
            return dev(self.I.y0, self.torch)
        return self.torch.full((self.I.M.rows,), 10.0, dtype=self.tdt, device="cuda")   # poisoned: every row must be written

    def multiply(self, accumulate):
        b, M, how, y = self.b, self.I.M, self.how, self.y_start(accumulate)
        if how in ("csr", "csr_table"):
            b.spmv_csr(M.rows, M.cols, self.dAp, self.dAj, self.dAx, self.dx, y, accumulate=accumulate, cfg=self.cfg)
        elif how in ("plan", "plan_cols", "plan_values"):
            b.spmv_csr_plan(self.plan, self.dAp, self.dAj, self.dAx, self.dx, y, accumulate=accumulate)
        elif how in ("ell", "ellr"):
            b.spmv_ell(M.rows, M.cols, self.width, self.pitch, self.deAj, self.deAx, self.dx, y, row_lengths=self.rl, accumulate=accumulate, cfg=self.cfg)
        elif how == "dia":
            b.spmv_dia(M.rows, M.cols, self.doff.numel(), self.pitch, self.doff, self.dvals, self.dx, y, accumulate=accumulate, cfg=self.cfg)
        elif how in ("coo", "coo_unsorted"):
            b.spmv_coo(M.rows, M.cols, self.dAi, self.dAj, self.dAx, self.dx, y, accumulate=accumulate, cfg=self.cfg)
        elif how.startswith("coo_plan"):
            b.spmv_coo_plan(self.plan, self.dAi, self.dAj, self.dAx, self.dx, y, accumulate=accumulate)
        elif how == "hyb":
            b.spmv_hyb_plan(self.plan, self.pitch, *self.h, self.dx, y, accumulate=accumulate)
        return y.cpu().numpy()

    def multiply_dot(self, w, res, ws):
        """The fused entry point of this path's format: y and <y, w>."""
        b, M, how, y = self.b, self.I.M, self.how, self.y_start(False)
        if how == "csr":
            b.spmv_csr_dot(M.rows, M.cols, self.dAp, self.dAj, self.dAx, self.dx, y, w, res, ws, cfg=self.cfg)
        elif how in ("plan", "plan_cols", "plan_values"):
            b.spmv_csr_dot(M.rows, M.cols, self.dAp, self.dAj, self.dAx, self.dx, y, w, res, ws, plan=self.plan)
        elif how in ("ell", "ellr"):
            b.spmv_ell_dot(M.rows, M.cols, self.width, self.pitch, self.deAj, self.deAx, self.dx, y, w, res, ws, row_lengths=self.rl, cfg=self.cfg)
        elif how == "dia":
            b.spmv_dia_dot(M.rows, M.cols, self.doff.numel(), self.pitch, self.doff, self.dvals, self.dx, y, w, res, ws, cfg=self.cfg)
        elif how.startswith("coo_plan"):
            b.spmv_coo_dot_plan(self.plan, self.dAi, self.dAj, self.dAx, self.dx, y, w, res, ws)
        elif how == "hyb":
            b.spmv_hyb_dot_plan_args(b.hyb_plan_args(self.plan, self.pitch, *self.h), self.dx, y, w, res, ws)
        else:
            raise AssertionError(how)
        return y.cpu().numpy(), float(res.cpu()[0])


def ids(table):
    return [e[0].replace(" ", "_") for e in table]


# ------------------------------------------------------------------------------------------------
# paths that claim storage-order sums: the oracle's bits, on every deck
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("entry", EXACT, ids=ids(EXACT))
def test_storage_order_paths_return_the_reference_bits(cmi, torch_cuda, orc, monkeypatch, entry, tag):
    for name in entry[2]:
        for dname in sv.DECKS:
            I = inputs(orc, name, tag, dname)
            run = Runner(cmi, torch_cuda, I, entry, True, monkeypatch)
            for accumulate in (False, True):
                sv.same_bits(run.multiply(accumulate), I.want(accumulate, run.fmt), f"{run.what} accumulate {accumulate}")


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("name", DOT, ids=[n.replace(" ", "_") for n in DOT])
def test_fused_dot(cmi, torch_cuda, orc, monkeypatch, name, tag):
    """y as the plain multiply's reference, bit for bit; <y, w> (a double) NaN / inf exactly when the index-order float64 sum of
    the reference is (w > 0: that does not depend on the order on these decks), and on the finite decks within the bar of the
    dot tests in tests/test_spmv_gpu.py: 1e-12 * sum |y_i w_i| (w holds small integers: products and sums are exact there)."""
    torch = torch_cuda
    entry = next(e for e in EXACT if e[0] == name)
    ws = cmi.blas_workspace()
    res = torch.zeros(1, dtype=torch.float64, device="cuda")
    for mname in entry[2]:
        M = matrix(mname, tag)
        w = np.random.default_rng(11).integers(1, 5, size=M.rows).astype(DT[tag])
        dw = dev(w, torch)
        for dname in sv.DECKS:
            I = inputs(orc, mname, tag, dname)
            run = Runner(cmi, torch, I, entry, True, monkeypatch)
            want = I.want(False, run.fmt)
            res.fill_(12345.0)
            y, dot = run.multiply_dot(dw, res, ws)
            sv.same_bits(y, want, run.what + " (fused dot): y")
            with np.errstate(all="ignore"):
                terms = want.astype(np.float64) * w.astype(np.float64)
                ref = float(np.cumsum(terms)[-1])                     # index order
            print(f"{run.what}: dot {dot!r} reference {ref!r}")
            assert np.isnan(dot) == np.isnan(ref), run.what
            if dname == "nan_near_miss":
                assert np.isnan(ref)
            elif dname in sv.FINITE_DECKS:
                assert np.isfinite(ref) and abs(dot - ref) <= 1e-12 * float(np.abs(terms).sum()), (run.what, dot, ref)
            else:   # overflow_order: +inf rows and finite rows; inf_near_miss: NaN rows (0 * inf) -- neither depends on the order
                assert not np.isfinite(ref), run.what
                assert np.isinf(dot) == np.isinf(ref) and (np.isnan(ref) or np.sign(dot) == np.sign(ref)), (run.what, dot, ref)


# ------------------------------------------------------------------------------------------------
# SpMM: column c of Y is the SpMV of column c of X, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("name", ["runs", "irregular"])
@pytest.mark.parametrize("entry", SPMM, ids=ids(SPMM))
def test_spmm_columns_are_spmv_bits(cmi, torch_cuda, orc, entry, name, tag):
    """The matrix takes the values of each deck in turn; column c of X is the x of the deck c places further on (so the first
    column is the deck's own x and k = 8 holds all five), then ordinary columns, then the NaN deck's x again."""
    torch, b = torch_cuda, cmi.binding
    M, dtype = matrix(name, tag), DT[tag]
    cfg = None if entry[1] == "KERNEL_AUTO" else config(b, entry[1], entry[2])
    dAp, dAj = dev(M.Ap, torch), dev(M.Aj, torch)
    rng = np.random.default_rng(5)
    for d, dname in enumerate(sv.DECKS):
        Ax = deck(name, tag, dname)[0]
        dAx = dev(Ax, torch)
        X, Y0 = np.empty((M.cols, 8), dtype), np.empty((M.rows, 8), dtype)
        for c in range(8):
            if c < 5:
                _, X[:, c], Y0[:, c] = deck(name, tag, sv.DECKS[(d + c) % 5])
            elif c < 7:
                X[:, c], Y0[:, c] = rng.standard_normal(M.cols), rng.standard_normal(M.rows)
            else:
                _, X[:, c], Y0[:, c] = deck(name, tag, "nan_near_miss")
        want = {acc: np.stack([orc.spmv_csr(M.Ap, M.Aj, Ax, np.ascontiguousarray(X[:, c]), np.ascontiguousarray(Y0[:, c]) if acc else None)
                               for c in range(8)], 1) for acc in (False, True)}
        for k in (1, 3, 8):
            cols_of = list(range(k - 1)) + [7] if k == 8 else list(range(k))
            for layout in ("row", "col"):
                for acc in (False, True):
                    Xh, Yh = X[:, cols_of], (Y0[:, cols_of] if acc else np.full((M.rows, k), 10.0, dtype))
                    if layout == "row":
                        dX, dY = dev(Xh, torch), dev(Yh, torch)
                    else:
                        dX, dY = dev(Xh.T, torch).T, dev(Yh.T, torch).T
                    b.spmm_csr(M.rows, M.cols, dAp, dAj, dAx, dX, dY, accumulate=acc, cfg=cfg)
                    got = dY.cpu().numpy()
                    for i, c in enumerate(cols_of):
                        sv.same_bits(np.ascontiguousarray(got[:, i]), np.ascontiguousarray(want[acc][:, c]),
                                     f"{entry[0]}: {name} {tag} values of {dname}, k {k}, {layout}-major, accumulate {acc}, column {i}")


# ------------------------------------------------------------------------------------------------
# paths that re-associate
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("entry", REASSOCIATED, ids=ids(REASSOCIATED))
def test_reassociating_paths(cmi, torch_cuda, orc, monkeypatch, entry, tag):
    """NaNs exactly where the reference has them and the finite rows within TOL * sum_j |a_ij x_j| (tests/test_fuzz_gpu.py's rule);
    on signed_zeros and subnormals every sum is exact in any order, so the VALUES are the reference's (the sign of a zero is not
    compared here)."""
    dtype = np.dtype(DT[tag])
    for name in entry[2]:
        for dname in ("nan_near_miss",) + sv.FINITE_DECKS:
            I = inputs(orc, name, tag, dname)
            run = Runner(cmi, torch_cuda, I, entry, False, monkeypatch)
            for accumulate in (False, True):
                got, want = run.multiply(accumulate), I.want(accumulate)
                what = f"{run.what} accumulate {accumulate}"
                if dname == "nan_near_miss":
                    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: {int((np.isnan(got) != np.isnan(want)).sum())} rows differ in NaN-ness"
                    ok = ~np.isnan(want)
                    bound = orc.spmv_csr(I.M.Ap, I.M.Aj, np.abs(I.Ax), np.nan_to_num(np.abs(I.x), nan=0.0)) + (np.abs(I.y0) if accumulate else 0)
                    err = np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64))
                    lim = TOL[dtype] * np.maximum(bound[ok].astype(np.float64), np.finfo(dtype).tiny)
                    assert np.all(err <= lim), f"{what}: {int((err > lim).sum())} finite rows out of tolerance (worst {err.max():.3e})"
                else:
                    bad = ~(got == want)
                    assert not bad.any(), f"{what}: {int(bad.sum())} rows differ in value, first {np.flatnonzero(bad)[:5]}: {got[bad][:5]} against {want[bad][:5]}"


# ------------------------------------------------------------------------------------------------
# builders: the zero tests
# ------------------------------------------------------------------------------------------------
def special_mix(n, dtype, seed):
    """n values: ordinary ones with +0.0, -0.0, NaN, +-inf, the smallest subnormal (both signs) and finfo.tiny at seeded places."""
    fi = np.finfo(dtype)
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n).astype(dtype)
    specials = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, fi.smallest_subnormal, -fi.smallest_subnormal, fi.tiny], dtype)
    where = rng.permutation(n)[:n // 2]
    v[where] = specials[np.arange(len(where)) % len(specials)]
    return v


@pytest.mark.parametrize("tag", TAGS)
def test_count_zeros_on_special_values(cmi, torch_cuda, tag):
    """cmi_count_zeros_*: -0.0 is a zero; a subnormal and a NaN are not."""
    v = special_mix(10007, DT[tag], 3)
    want = int((v == 0).sum())
    assert want >= 1000 and np.signbit(v[v == 0]).any() and (np.abs(v[v != 0]) < np.finfo(DT[tag]).tiny).any()
    assert cmi.binding.count_zeros(dev(v, torch_cuda)) == want


@pytest.mark.parametrize("tag", TAGS)
def test_dia_to_csr_on_special_values(cmi, torch_cuda, tag):
    """cmi_dia_to_csr_* on the poisson5pt(9, 7) diagonals holding the mix: the kept entries are those with a column in range and
    v != 0 (so -0.0 goes, subnormals and NaNs stay), row-major, values bit for bit."""
    torch, b, dtype = torch_cuda, cmi.binding, DT[tag]
    m, n = 9, 7
    N, pitch = m * n, 64
    off = np.array([-m, -1, 0, 1, m], np.int32)
    vals = special_mix(5 * pitch, dtype, 4)
    V = vals.reshape(5, pitch)
    Ap, Aj, Ax = [0], [], []
    for r in range(N):
        for d in range(5):
            j = r + int(off[d])
            if 0 <= j < N and V[d, r] != 0:
                Aj.append(j)
                Ax.append(V[d, r])
        Ap.append(len(Aj))
    Ax = np.array(Ax, dtype)
    assert np.isnan(Ax).any() and (np.abs(Ax[~np.isnan(Ax)]) < np.finfo(dtype).tiny).any() and len(Ax) < 5 * N - 2 * (m + 1) - 20
    gAp, gAj, gAx = b.dia_to_csr(N, N, 5, pitch, dev(off, torch), dev(vals, torch))
    assert np.array_equal(gAp.cpu().numpy(), np.array(Ap, np.int32))
    assert np.array_equal(gAj.cpu().numpy(), np.array(Aj, np.int32))
    sv.same_bits(gAx.cpu().numpy(), Ax, f"dia -> csr {tag}: values")
