"""GPU tests (-m gpu) of the semiring multiply: cmi_spmv_{csr,coo,ell,dia}_semiring_* through the raw wrappers, bit for bit against the
plain-Python loops of tests/semiring_refs.py (sv.same_bits: NaN against NaN is equal, everything else by bit pattern); the Python-level
cmi.spmv_semiring on the five matrix classes; and tests/semiring/test_semiring_device.cpp (cusp::multiply / generalized_spmv on
device_memory against host_memory).

CSR, COO, ELL and HYB forms of one matrix have the same chain per row (tests/test_semiring_refs.py asserts it on the CPU), so they are
compared with the CSR loop's result; DIA with its own loop (every in-range slot takes part).

The CSR launch shape, restated from csrc/spmv_semiring.hip: K = 2 / 5 / 8 entries per lane for a mean row length <= 2 / <= 5 / above, 64 rows
per wave (fewer when the mean exceeds K).  A wave's tile of more than 64 K entries takes passes; long_rows() below puts rows of 64 K,
64 K + 1 and 5000 entries alone between empty rows for each K, and next to short rows."""
import os
import subprocess

import numpy as np
import pytest

import semiring_refs as R
import special_values as sv
from conftest import GOLDEN, ROOT, coo_to_csr, read_mtx, reference_data_files

pytestmark = pytest.mark.gpu
TAGS = ("f64", "f32")
DT = {"f64": np.float64, "f32": np.float32}
SOME_PAIRS = (("multiplies", "plus"), ("plus", "minimum"), ("multiplies", "maximum"), ("project2nd", "maximum"), ("project1st", "minimum"),
              ("minimum", "multiplies"), ("maximum", "plus"), ("project2nd", "minimum"))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch


class Csr:
    """A host CSR matrix in every format the kernels take."""

    def __init__(self, rows, cols, Ap, Aj, Ax, dia=None, hyb_width=None):
        self.rows, self.cols = int(rows), int(cols)
        self.Ap, self.Aj, self.Ax = np.ascontiguousarray(Ap, np.int32), np.ascontiguousarray(Aj, np.int32), np.ascontiguousarray(Ax)
        self.Ai = R.csr_to_coo(self.Ap)
        self.dia_spec, self.width = dia, hyb_width
        self._f = {}

    def operands(self, fmt):
        if fmt not in self._f:
            lens = np.diff(self.Ap)
            if fmt == "csr":
                v = (self.rows, self.cols, self.Ap, self.Aj, self.Ax)
            elif fmt == "coo":
                v = (self.rows, self.cols, self.Ai, self.Aj, self.Ax)
            elif fmt == "ell":
                v = (self.rows, self.cols) + R.csr_to_ell(self.Ap, self.Aj, self.Ax)
            elif fmt == "hyb":
                w = self.width if self.width is not None else max(1, int(np.ceil(lens.sum() / max(self.rows, 1))))
                v = (self.rows, self.cols) + R.csr_to_hyb(self.Ap, self.Aj, self.Ax, w)
            else:
                offsets, pitch = self.dia_spec
                v = (self.rows, self.cols, len(offsets), pitch, offsets, R.csr_to_dia(self.rows, self.cols, self.Ap, self.Aj, self.Ax, offsets, pitch))
            self._f[fmt] = v
        return self._f[fmt]

    def want(self, fmt, x, combine, reduce, y0=None, init=0.0, Ax="own"):
        Ax = self.Ax if isinstance(Ax, str) else Ax
        if fmt == "dia":
            _, _, _, pitch, offsets, vals = self.operands("dia")
            return R.semiring_dia(self.rows, self.cols, pitch, offsets, vals if Ax is not None else None, x, combine, reduce, y0, init)
        return R.semiring_csr(self.Ap, self.Aj, Ax, x, combine, reduce, y0, init)


def run(cmi, torch, A, fmt, x, combine, reduce, y0=None, init=0.0, dtype=None, inplace=False, no_values=False, no_vector=False):
    """One multiply on the device through the raw wrappers; y starts as NaN unless it is y0 itself (inplace)."""
    dtype = np.dtype(dtype or (x.dtype if x is not None else A.Ax.dtype))

    def D(a, drop=False):
        return None if a is None or drop else torch.from_numpy(np.ascontiguousarray(a)).cuda()

    dx = D(x, no_vector)
    if inplace:
        y = D(y0.astype(dtype))
        dy0 = y
    else:
        y = torch.full((A.rows,), float("nan"), dtype=getattr(torch, dtype.name), device="cuda")
        dy0 = D(y0)
    op = A.operands(fmt)
    if fmt == "csr":
        cmi.spmv_csr_semiring(A.rows, A.cols, D(op[2]), D(op[3], no_vector), D(op[4], no_values), dx, y, combine, reduce, dy0, init, num_entries=len(op[3]))
    elif fmt == "coo":
        cmi.spmv_coo_semiring(A.rows, A.cols, D(op[2]), D(op[3], no_vector), D(op[4], no_values), dx, y, combine, reduce, dy0, init)
    elif fmt == "ell":
        cmi.spmv_ell_semiring(A.rows, A.cols, op[2], op[3], D(op[4]), D(op[5], no_values), dx, y, combine, reduce, dy0, init)
    elif fmt == "dia":
        cmi.spmv_dia_semiring(A.rows, A.cols, op[2], op[3], D(np.asarray(op[4], np.int32)), D(op[5], no_values), dx, y, combine, reduce, dy0, init)
    else:  # HYB: the ELL part, then the COO part on top of it
        _, _, width, pitch, eAj, eAx, cAi, cAj, cAx = op
        cmi.spmv_ell_semiring(A.rows, A.cols, width, pitch, D(eAj), D(eAx, no_values), dx, y, combine, reduce, dy0, init)
        cmi.spmv_coo_semiring(A.rows, A.cols, D(cAi), D(cAj, no_vector), D(cAx, no_values), dx, y, combine, reduce, y, 0.0)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def check(cmi, torch, A, fmts, x, pairs, starts, y0, what, want_cache=None):
    """Every (format, pair, start) of the lists against the loops; `starts`: "y0", "inplace" or a constant."""
    want_cache = {} if want_cache is None else want_cache
    for combine, reduce in pairs:
        for start in starts:
            kw = {"y0": y0} if isinstance(start, str) else {"init": start}
            for fmt in fmts:
                key = ("dia" if fmt == "dia" else "csr", combine, reduce, str(start) if not isinstance(start, str) else "y0")
                if key not in want_cache:
                    want_cache[key] = A.want(fmt, x, combine, reduce, **kw)
                got = run(cmi, torch, A, fmt, x, combine, reduce, inplace=start == "inplace", **kw)
                sv.same_bits(got, want_cache[key], f"{what} {fmt} ({combine}, {reduce}) start {start}")


# ------------------------------------------------------------------------------------------------
# all 24 pairs on 5pt_10x10
# ------------------------------------------------------------------------------------------------
def five_point(dtype):
    rows, cols, I, J, V = read_mtx(os.path.join(GOLDEN, "5pt_10x10.mtx"))
    Ap, Aj, Ax = coo_to_csr(rows, I, J, V, dtype)
    return Csr(rows, cols, Ap, Aj, Ax, dia=(np.array([-10, -1, 0, 1, 10], np.int32), 112))


@pytest.mark.parametrize("tag", TAGS)
def test_all_24_pairs_on_5pt_10x10(cmi, torch_cuda, tag):
    """Every combine x reduce, from a constant and from y0, in the five formats (DIA: the slots across the grid's row ends are stored zeros
    that take part).  x holds a NaN, both zeros and an infinity."""
    T = DT[tag]
    A = five_point(T)
    rng = np.random.default_rng(3)
    x, y0 = rng.standard_normal(A.cols).astype(T), rng.standard_normal(A.rows).astype(T)
    x[[7, 33, 34, 61]] = [np.nan, 0.0, -0.0, np.inf]
    y0[[2, 50]] = [-0.0, np.inf]
    check(cmi, torch_cuda, A, ("csr", "coo", "ell", "dia", "hyb"), x, R.PAIRS, ("y0", 2.5), y0, f"5pt_10x10 {tag}")


# ------------------------------------------------------------------------------------------------
# the decks
# ------------------------------------------------------------------------------------------------
def deck_matrix(name, T):
    M = R.matrices(T)[name]
    return M, {"irregular": ("csr", "coo", "hyb"), "irregular_short": ("csr", "coo", "ell", "hyb"), "banded": ("dia", "csr", "coo", "ell", "hyb")}[name]


@pytest.mark.parametrize("dname", R.DECKS)
@pytest.mark.parametrize("name", ("irregular", "irregular_short", "banded"))
@pytest.mark.parametrize("tag", TAGS)
def test_decks(cmi, torch_cuda, tag, name, dname):
    """NaNs at the first / middle / last entry of rows, zero ties in both orders, stored zeros (in-range DIA slots on `banded`), ELL padding, HYB
    with a real split on every matrix (`banded`: width 6 of rows of 6 to 8; on `irregular` the 5000-entry row sits in the COO part); chains from y0
    and from +-inf, NaN and 2.5 in turn."""
    T = DT[tag]
    M, fmts = deck_matrix(name, T)
    Ax, x, y0 = R.decks(M, T)[dname]
    A = Csr(M.rows, M.cols, M.Ap, M.Aj, Ax, dia=(M.dia_offsets, M.dia_pitch) if hasattr(M, "dia_offsets") else None, hyb_width=R.hyb_width(M))
    _, _, width, _, eAj, _, cAi, _, _ = A.operands("hyb")     # a real split on every matrix: the chain crosses from the ELL part into the COO part
    assert 0 < width < M.row_lengths().max() and len(cAi) > 0 and (eAj != -1).sum() > 0 and (len(cAi) > 5000 - 64 or name != "irregular")
    if name == "banded":
        assert width == 6 and len(cAi) == R.hyb_parts(M)[1] >= M.rows      # rows of 6 to 8 entries: most rows continue in the COO part
    cache = {}
    for k, pair in enumerate(SOME_PAIRS):
        check(cmi, torch_cuda, A, fmts, x, (pair,), ("y0", R.INITS[k % 4]), y0, f"{name} {dname} {tag}", cache)


@pytest.mark.parametrize("tag", TAGS)
def test_random_10x10_set(cmi, torch_cuda, tag):
    """The reference's random_10x10 files, 000_nonzeros (no entry at all) included."""
    T = DT[tag]
    files = [f for f in reference_data_files() if os.sep + "random_10x10" + os.sep in f]
    assert any(f.endswith("000_nonzeros.mtx") for f in files) and len(files) >= 10
    rng = np.random.default_rng(10)
    x, y0 = rng.standard_normal(10).astype(T), rng.standard_normal(10).astype(T)
    x[4] = np.nan
    for f in files:
        rows, cols, I, J, V = read_mtx(f)
        A = Csr(rows, cols, *coo_to_csr(rows, I, J, V, T))
        check(cmi, torch_cuda, A, ("csr", "coo", "ell", "hyb"), x, SOME_PAIRS[:4], ("y0", -np.inf), y0, os.path.basename(f) + " " + tag)


# ------------------------------------------------------------------------------------------------
# shapes where the kernels can go wrong
# ------------------------------------------------------------------------------------------------
def random_rows(rows, cols, T, seed, max_len=9):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, rows)
    Ap = np.r_[0, np.cumsum(lens)].astype(np.int32)
    Aj = rng.integers(0, cols, int(lens.sum())).astype(np.int32)
    return Csr(rows, cols, Ap, Aj, rng.standard_normal(len(Aj)).astype(T))


@pytest.mark.parametrize("tag", TAGS)
def test_row_counts_and_one_column(cmi, torch_cuda, tag):
    T = DT[tag]
    for rows, cols in ((1, 5), (63, 66), (64, 67), (65, 68), (257, 260), (130, 1)):
        A = random_rows(rows, cols, T, rows)
        rng = np.random.default_rng(rows + 1)
        x, y0 = rng.standard_normal(cols).astype(T), rng.standard_normal(rows).astype(T)
        check(cmi, torch_cuda, A, ("csr", "coo", "ell", "hyb"), x, SOME_PAIRS[:5], ("y0", np.inf), y0, f"{rows} x {cols} {tag}")


LONG = (128, 129, 320, 321, 512, 513, 5000)     # 64 K and 64 K + 1 for K = 2, 5, 8, and many passes


def long_rows(rows, T, seed=0):
    """Tile t = 0 .. 6 (64 rows each) holds ONE row of LONG[t] entries between empty rows; tiles 7 .. 13 hold the same rows next to short rows
    (1 .. 3 entries) on both sides; every further row is empty, which sets the mean row length and with it K."""
    rng = np.random.default_rng(seed)
    lens = np.zeros(rows, np.int64)
    for t, n in enumerate(LONG):
        lens[64 * t + 5 + 7 * t] = n
        at = 64 * (7 + t) + 60 - 9 * t
        lens[at] = n
        lens[at - 3:at] = (1, 3, 2)
        lens[at + 1:at + 3] = (2, 1)
    cols = 6000
    Ap = np.r_[0, np.cumsum(lens)].astype(np.int32)
    Aj = rng.integers(0, cols, int(lens.sum())).astype(np.int32)
    return Csr(rows, cols, Ap, Aj, rng.standard_normal(len(Aj)).astype(T), hyb_width=2)


@pytest.mark.parametrize("rows,K", ((16000, 2), (5000, 5), (2100, 8), (900, 8)))
@pytest.mark.parametrize("tag", TAGS)
def test_pass_boundaries_and_the_carried_value(cmi, torch_cuda, tag, rows, K):
    """Rows of exactly 64 K, 64 K + 1 and 5000 entries between empty rows and beside short rows, at every K the launch rule chooses (900 rows: a
    mean beyond 8, fewer than 64 rows per wave).  NaNs sit in the long rows, so a chain joined out of order would show."""
    T = DT[tag]
    A = long_rows(rows, T)
    mean = len(A.Aj) / rows
    assert (2 if mean <= 2 else 5 if mean <= 5 else 8) == K and (mean > 8) == (rows == 900)
    rng = np.random.default_rng(rows)
    x, y0 = rng.standard_normal(A.cols).astype(T), rng.standard_normal(rows).astype(T)
    x[rng.integers(0, A.cols, 40)] = np.nan
    x[rng.integers(0, A.cols, 40)] = -0.0
    check(cmi, torch_cuda, A, ("csr", "coo", "hyb"), x, (("multiplies", "plus"), ("project2nd", "minimum"), ("plus", "maximum")), ("y0", np.inf), y0,
          f"long rows {rows} {tag}")


@pytest.mark.parametrize("tag", TAGS)
def test_empty_and_degenerate_shapes(cmi, torch_cuda, tag):
    T = DT[tag]
    rng = np.random.default_rng(8)
    pairs = SOME_PAIRS[:4]
    # all rows empty (ELL of width 0, HYB with both parts empty): every row gets its start
    rows, cols = 100, 70
    E = Csr(rows, cols, np.zeros(rows + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, T), dia=(np.zeros(0, np.int32), 112), hyb_width=0)
    x, y0 = rng.standard_normal(cols).astype(T), rng.standard_normal(rows).astype(T)
    assert E.operands("ell")[2] == 0
    check(cmi, torch_cuda, E, ("csr", "coo", "ell", "dia", "hyb"), x, pairs, ("y0", 2.5, np.nan), y0, f"all rows empty {tag}")
    # a DIA diagonal wholly outside the matrix (on either side), next to real ones
    rows, cols = 70, 50
    offsets = np.array([-rows - 5, -3, 0, 4, cols + 9, cols - 1, -(rows - 1)], np.int32)
    row_cols = [[i + int(k) for k in offsets if 0 <= i + int(k) < cols] for i in range(rows)]
    lens = np.array([len(r) for r in row_cols])
    Aj = np.concatenate([np.array(r, np.int32) for r in row_cols])
    A = Csr(rows, cols, np.r_[0, np.cumsum(lens)], Aj, rng.standard_normal(len(Aj)).astype(T), dia=(offsets, 80))
    x, y0 = rng.standard_normal(cols).astype(T), rng.standard_normal(rows).astype(T)
    check(cmi, torch_cuda, A, ("dia", "csr"), x, pairs, ("y0", -np.inf), y0, f"diagonals outside {tag}")
    # COO whose first and last rows are empty; HYB with an empty ELL part (width 0) and with an empty COO part (width = the longest row)
    A = random_rows(200, 90, T, 21)
    lens = np.diff(A.Ap)
    lens[[0, 1, 198, 199]] = 0
    keep = np.repeat(lens > 0, np.diff(A.Ap))
    x, y0 = rng.standard_normal(90).astype(T), rng.standard_normal(200).astype(T)
    for width in (None, 0, int(lens.max())):
        B = Csr(200, 90, np.r_[0, np.cumsum(lens)], A.Aj[keep], A.Ax[keep], hyb_width=width)
        assert width is None or (len(B.operands("hyb")[6]) == 0) == (width > 0)
        check(cmi, torch_cuda, B, ("coo", "hyb", "csr"), x, pairs, ("y0", np.inf), y0, f"empty first / last rows, hyb width {width} {tag}")


# ------------------------------------------------------------------------------------------------
# unread streams, aliasing, the arithmetic pair against cmi_spmv_csr_*, project2nd / maximum against cmi_csr_ring_max_u64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_streams_that_are_not_read_may_be_null(cmi, torch_cuda, tag):
    T = DT[tag]
    M = R.matrices(T)["irregular_short"]
    Ax, x, y0 = R.decks(M, T)["nan_positions"]
    B = R.matrices(T)["banded"]
    bAx, bx, by0 = R.decks(B, T)["stored_zeros"]
    cases = ((Csr(M.rows, M.cols, M.Ap, M.Aj, Ax, hyb_width=R.hyb_width(M)), ("csr", "coo", "ell", "hyb"), x, y0),
             (Csr(B.rows, B.cols, B.Ap, B.Aj, bAx, dia=(B.dia_offsets, B.dia_pitch), hyb_width=R.hyb_width(B)), ("dia", "hyb"), bx, by0))
    assert all(min(R.hyb_parts(m)) > 0 for m in (M, B))
    for A, fmts, xx, yy in cases:
        for reduce in ("maximum", "plus"):
            for fmt in fmts:
                want = A.want(fmt, xx, "project2nd", reduce, y0=yy)
                sv.same_bits(run(cmi, torch_cuda, A, fmt, xx, "project2nd", reduce, y0=yy, no_values=True), want, f"NULL values {fmt} {reduce} {tag}")
                want = A.want(fmt, xx, "project1st", reduce, init=-np.inf)
                got = run(cmi, torch_cuda, A, fmt, xx, "project1st", reduce, init=-np.inf, no_vector=True, dtype=T)
                sv.same_bits(got, want, f"NULL x {fmt} {reduce} {tag}")


@pytest.mark.parametrize("tag", TAGS)
def test_y0_may_be_y_or_x(cmi, torch_cuda, tag):
    T = DT[tag]
    M = sv.matrices(T)["poisson100"]
    Ax, x, _ = R.decks(M, T)["zero_ties"]
    rng = np.random.default_rng(2)
    x = np.where(rng.random(M.cols) < 0.5, x, rng.standard_normal(M.cols).astype(T)).astype(T)
    A = Csr(M.rows, M.cols, M.Ap, M.Aj, Ax, dia=(np.array([-100, -1, 0, 1, 100], np.int32), M.rows), hyb_width=3)
    y0 = rng.standard_normal(M.rows).astype(T)
    check(cmi, torch_cuda, A, ("csr", "coo", "ell", "dia", "hyb"), x, (("plus", "minimum"), ("multiplies", "plus")), ("inplace",), y0, f"y0 == y {tag}")
    torch = torch_cuda
    dx = torch.from_numpy(x).cuda()
    y = torch.empty_like(dx)
    D = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    cmi.spmv_csr_semiring(M.rows, M.cols, D(A.Ap), D(A.Aj), D(A.Ax), dx, y, "project2nd", "maximum", y0=dx)
    sv.same_bits(y.cpu().numpy(), A.want("csr", x, "project2nd", "maximum", y0=x), f"y0 == x {tag}")


@pytest.mark.parametrize("tag", TAGS)
def test_multiplies_plus_gives_the_bits_of_the_scalar_csr_kernel(cmi, torch_cuda, tag):
    """(multiplies, plus, 0) and (multiplies, plus, y0 = y) against cmi_spmv_csr_* under CSR_SCALAR (one lane per row, storage order)."""
    T, torch = DT[tag], torch_cuda
    for name in ("irregular", "poisson100"):
        M = sv.matrices(T)[name]
        Ax, x, y0 = R.decks(M, T)["ordinary"]
        D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        Ap, Aj, dAx, dx = D(M.Ap), D(M.Aj), D(Ax), D(x)
        for accumulate in (False, True):
            want, got = D(y0), D(y0)
            cmi.spmv_csr(M.rows, M.cols, Ap, Aj, dAx, dx, want, accumulate, cmi.Config(kernel=cmi.CSR_SCALAR))
            cmi.spmv_csr_semiring(M.rows, M.cols, Ap, Aj, dAx, dx, got, "multiplies", "plus", y0=got if accumulate else None, init=0.0)
            torch.cuda.synchronize()
            sv.same_bits(got.cpu().numpy(), want.cpu().numpy(), f"{name} accumulate {accumulate} {tag}")


def test_project2nd_maximum_agrees_with_the_ring_maximum_of_keys(cmi, torch_cuda):
    """Keys that are exact integers below 2^53: z[i] = max(x[i], x over row i) is cmi_csr_ring_max_u64's sweep; here with y0 = x and no values."""
    torch = torch_cuda
    M = sv.matrices(np.float64)["poisson100"]
    rng = np.random.default_rng(53)
    keys = rng.integers(0, 2**53, M.rows, dtype=np.int64)
    Ap, Aj = torch.from_numpy(M.Ap).cuda(), torch.from_numpy(M.Aj).cuda()
    z = cmi.csr_ring_max(M.rows, Ap, Aj, torch.from_numpy(keys).cuda())
    x = torch.from_numpy(keys.astype(np.float64)).cuda()
    assert np.array_equal(x.cpu().numpy().astype(np.int64), keys)
    y = torch.empty_like(x)
    cmi.spmv_csr_semiring(M.rows, M.cols, Ap, Aj, None, x, y, "project2nd", "maximum", y0=x)
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy().astype(np.int64), z.cpu().numpy())


# ------------------------------------------------------------------------------------------------
# cmi.spmv_semiring on the five matrix classes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_python_spmv_semiring_on_the_five_classes(cmi, torch_cuda, tag):
    torch = torch_cuda
    T = DT[tag]
    m, n = 13, 9
    dev = torch.device("cuda", 0)
    A = cmi.poisson5pt(m, n, "csr", device=dev, dtype=getattr(torch, np.dtype(T).name))
    Ap, Aj, Ax = (t.cpu().numpy() for t in (A.row_offsets, A.column_indices, A.values))
    N = m * n
    rng = np.random.default_rng(1)
    x, y0 = rng.standard_normal(N).astype(T), rng.standard_normal(N).astype(T)
    x[[5, 40]] = [np.nan, -0.0]
    dx = torch.from_numpy(x).to(dev)
    mats = {"csr": A, "coo": cmi.convert(A, "coo"), "ell": cmi.convert(A, "ell"), "dia": cmi.convert(A, "dia"),
            "hyb": cmi.convert(A, "hyb", num_entries_per_row=3)}
    assert mats["hyb"].coo.num_entries > 0
    D = mats["dia"]
    for combine, reduce, init in (("plus", "minimum", None), ("project2nd", "maximum", -np.inf), ("multiplies", "plus", 2.5), ("multiplies", "plus", None)):
        kw = {"y0": y0} if init is None else {"init": init}
        want = R.semiring_csr(Ap, Aj, Ax, x, combine, reduce, **kw)
        want_dia = R.semiring_dia(N, N, D.pitch, D.diagonal_offsets.cpu().numpy(), D.values.cpu().numpy(), x, combine, reduce, **kw)
        for fmt, B in mats.items():
            y = torch.from_numpy(y0).to(dev)
            assert cmi.spmv_semiring(B, dx, y, combine, reduce, init) is y
            sv.same_bits(y.cpu().numpy(), want_dia if fmt == "dia" else want, f"spmv_semiring {fmt} ({combine}, {reduce}) init {init} {tag}")
    C = mats["coo"]
    perm = torch.from_numpy(rng.permutation(C.num_entries)).to(dev)
    U = cmi.CooMatrix(N, N, C.num_entries, C.row_indices[perm].contiguous(), C.column_indices[perm].contiguous(), C.values[perm].contiguous())
    y = torch.from_numpy(y0).to(dev)
    with pytest.raises(ValueError, match="sort_by_row"):
        cmi.spmv_semiring(U, dx, y, "plus", "minimum")
    U.sort_by_row()
    cmi.spmv_semiring(U, dx, y, "project2nd", "maximum")     # (stable sort: the row's entries keep their shuffled order; maximum of x over the row)
    want = R.semiring_coo(N, U.row_indices.cpu().numpy(), U.column_indices.cpu().numpy(), U.values.cpu().numpy(), x, "project2nd", "maximum", y0=y0)
    sv.same_bits(y.cpu().numpy(), want, f"sorted COO {tag}")


# ------------------------------------------------------------------------------------------------
# the C++ layer on device_memory
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_program(cmi, tmp_path_factory):
    import test_semiring_host as H
    return H.build(tmp_path_factory.mktemp("semiring_device"), "test_semiring_device.cpp", "test_semiring_device")


def test_semiring_cpp_device_layer(device_program):
    """cusp::multiply / generalized_spmv with the named functors on device_memory against host_memory, five formats, a stream policy, the refusals
    (a user's functor, unsorted COO) and Bellman-Ford: see the program."""
    import test_semiring_host as H
    r = subprocess.run([str(device_program)], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert H.DEVICE_TESTS in r.stdout


def test_device_multiply_gives_the_host_bits_on_the_deck_file(device_program, tmp_path):
    """Every deck of tests/test_semiring_host.py through cusp::multiply / generalized_spmv on device_memory: the program compares each case with
    its host_memory run before it prints it (exit status 3 otherwise); the 5pt_10x10 decks (24 pairs x 5 formats x {y0, constant} and
    generalized_spmv) are compared with the loops here as well -- the others are, for the host path, in the CPU suite."""
    import test_semiring_host as H
    all_decks = H.decks()
    path = tmp_path / "decks.txt"
    H.write_decks(path, all_decks)
    r = subprocess.run([str(device_program), "decks", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = H.parse(r.stdout, all_decks)
    small = [k for k, d in enumerate(all_decks) if d.name == "5pt_10x10"]
    assert len(small) == 2
    H.compare([got[k] for k in small], [all_decks[k] for k in small], "device")


def test_bellman_ford_distances_are_dijkstras(device_program):
    """(plus, minimum) with y0 = y on poisson5pt 33 x 31 with weights |values| (integers: every sum exact): the program prints the device's
    distances after it has checked them against the host path's bits; they equal scipy's Dijkstra exactly."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import dijkstra
    r = subprocess.run([str(device_program), "bellman_ford"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.split("\n") if l.startswith("distances ")][0].split()
    sweeps, got = int(line[1]), np.array([float.fromhex(v) for v in line[2:]])
    mx, my = 33, 31
    N = mx * my
    assert len(got) == N and sweeps <= N
    idx = np.arange(N)
    ix, iy = idx % mx, idx // mx
    I, J, V = [idx], [idx], [np.full(N, 4.0)]
    for ok, off in ((iy > 0, -mx), (ix > 0, -1), (ix < mx - 1, 1), (iy < my - 1, mx)):
        I.append(idx[ok]); J.append(idx[ok] + off); V.append(np.ones(ok.sum()))
    G = sp.csr_matrix((np.concatenate(V), (np.concatenate(I), np.concatenate(J))), shape=(N, N))
    G.setdiag(0)
    G.eliminate_zeros()
    want = dijkstra(G, directed=True, indices=0)
    assert np.array_equal(got, want)
