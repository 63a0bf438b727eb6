"""cmi_ell_to_csr_*, cmi_dia_to_csr_* and cmi_hyb_to_csr_* at the C ABI (-m gpu): count per row, row offsets, scatter.

Every case is checked against a numpy restatement written here (keep the entries with a valid column -- DIA: a column inside the
matrix and a value != 0 -- row by row, slot by slot; HYB: a row's ELL entries, then its COO entries).  Row offsets, columns and the
entry count must be equal, the values bit-equal.  The row counts straddle the sizes at which a blocked prefix sum changes path
(2047 / 2048 / 2049, 4097) and 300 001 rows span many blocks of any scan; the rows mix empty, full and padded ones, hold a long
stretch of consecutive empty rows and end in a non-empty row.  Both calls of the sizing protocol run: Aj == NULL, then the fill.
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID_VALUE, NOT_SUPPORTED = 1, 3
DT = {"f64": np.float64, "f32": np.float32}
ROWS = (0, 1, 2047, 2048, 2049, 4097, 300001)
WIDTH = 3                      # ELL slots per row, and the number of diagonals
DIA_OFFSETS = (-1, 0, 2)
GUARD = 8                      # entries behind the capacity that the fill must leave alone


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch


def empty_stretch(n):
    """[lo, hi): consecutive rows that hold nothing -- 3000 of them where the matrix has the rows for it, half of it otherwise"""
    lo = n // 8
    return lo, lo + (3000 if n >= 4097 else n // 2)


@functools.lru_cache(maxsize=None)
def row_kinds(n):
    """per row: 0 empty, 1 full, 2 one entry, 3 two entries, 4 a hole in the middle slot; the last row is full"""
    i = np.arange(n)
    kind = (i * 7 + i // 5) % 5
    lo, hi = empty_stretch(n)
    kind[lo:hi] = 0
    if n:
        kind[-1] = 1
    return kind


def values_for(n, dtype):
    """[n, WIDTH] non-zero values, no two equal in a row"""
    i = np.arange(n, dtype=np.int64)[:, None]
    k = np.arange(WIDTH, dtype=np.int64)[None, :]
    return (((i * 3 + k * 31) % 197 + 1) * 0.37 * np.where((i + k) % 2 == 0, 1.0, -1.0)).astype(dtype)


@functools.lru_cache(maxsize=None)
def ell_case(n, tag):
    """(pitch, slots-major column and value arrays, the [n, WIDTH] views of them)"""
    kind = row_kinds(n)
    i = np.arange(n, dtype=np.int64)[:, None]
    k = np.arange(WIDTH, dtype=np.int64)[None, :]
    cols = ((i * 7 + k * 13) % (n + 5)).astype(np.int32)
    have = {0: [0, 0, 0], 1: [1, 1, 1], 2: [1, 0, 0], 3: [1, 1, 0], 4: [1, 0, 1]}
    mask = np.array([have[q] for q in range(5)], dtype=bool)[kind] if n else np.zeros((0, WIDTH), dtype=bool)
    cols = np.where(mask, cols, -1).astype(np.int32)
    vals = np.where(mask, values_for(n, DT[tag]), 0).astype(DT[tag])
    pitch = n + 5
    eAj = np.full((WIDTH, pitch), -1, dtype=np.int32)
    eAx = np.zeros((WIDTH, pitch), dtype=DT[tag])
    eAj[:, :n] = cols.T
    eAx[:, :n] = vals.T
    return pitch, eAj.ravel(), eAx.ravel(), cols, vals


def csr_of(n, row, col, val):
    """CSR of entries given in the order they are to be stored within their rows (a stable sort by row keeps it)"""
    order = np.argsort(row, kind="stable")
    Ap = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(row, minlength=n)[:n], out=Ap[1:])
    return Ap, col[order].astype(np.int32), val[order]


def want_ell(n, tag):
    _, _, _, cols, vals = ell_case(n, tag)
    keep = cols >= 0
    row = np.broadcast_to(np.arange(n)[:, None], cols.shape)[keep]
    return csr_of(n, row, cols[keep], vals[keep])


@functools.lru_cache(maxsize=None)
def dia_case(n, tag):
    """(num_cols, pitch, offsets, diagonal-major values): explicit zeros where a row kind has no entry, and non-zero values on
    positions whose column lies outside the matrix (those are dropped for their column, not for their value)"""
    kind = row_kinds(n)
    have = {0: [0, 0, 0], 1: [1, 1, 1], 2: [1, 0, 0], 3: [1, 1, 0], 4: [1, 0, 1]}
    mask = np.array([have[q] for q in range(5)], dtype=bool)[kind] if n else np.zeros((0, WIDTH), dtype=bool)
    vals = np.where(mask, values_for(n, DT[tag]), 0).astype(DT[tag])
    num_cols, pitch = n + 1, n + 3
    dv = np.zeros((WIDTH, pitch), dtype=DT[tag])
    dv[:, :n] = vals.T
    return num_cols, pitch, np.array(DIA_OFFSETS, dtype=np.int32), dv.ravel(), vals


def want_dia(n, tag):
    num_cols, _, off, _, vals = dia_case(n, tag)
    j = np.arange(n, dtype=np.int64)[:, None] + off[None, :].astype(np.int64)
    keep = (j >= 0) & (j < num_cols) & (vals != 0)
    row = np.broadcast_to(np.arange(n)[:, None], vals.shape)[keep]
    return csr_of(n, row, j[keep], vals[keep])


@functools.lru_cache(maxsize=None)
def hyb_coo(n, tag):
    """the COO part: one or two entries in every seventh row outside the empty stretch and one in the last row, sorted by row"""
    i = np.arange(n, dtype=np.int64)
    count = np.where(i % 7 == 3, i % 2 + 1, 0)
    lo, hi = empty_stretch(n)
    count[lo:hi] = 0
    if n:
        count[-1] += 1
    row = np.repeat(i, count)
    pos = np.arange(len(row), dtype=np.int64)
    col = ((row * 11 + pos * 3) % (n + 5)).astype(np.int32)
    val = ((pos % 89 + 2) * -0.61).astype(DT[tag])
    return row.astype(np.int32), col, val


def want_hyb(n, tag):
    _, _, _, cols, vals = ell_case(n, tag)
    cAi, cAj, cAx = hyb_coo(n, tag)
    keep = cols >= 0
    row = np.broadcast_to(np.arange(n)[:, None], cols.shape)[keep]
    return csr_of(n, np.concatenate([row, cAi.astype(np.int64)]), np.concatenate([cols[keep], cAj]), np.concatenate([vals[keep], cAx]))


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t.numel() else None


class Call:
    """one conversion at the C ABI: its device inputs, and run(Ap, Aj, Ax, capacity) -> (status, entry count)"""
    def __init__(self, cmi, torch, fmt, n, tag):
        self.L, self.torch, self.fmt, self.n = cmi.lib(), torch, fmt, n
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        fn = getattr(self.L, f"cmi_{fmt}_to_csr_{tag}")
        if fmt == "dia":
            num_cols, pitch, off, dv, _ = dia_case(n, tag)
            self.keep = (dev(off), dev(dv))
            self.front = (fn, n, num_cols, WIDTH, pitch, ptr(self.keep[0]), ptr(self.keep[1]))
        else:
            pitch, eAj, eAx, _, _ = ell_case(n, tag)
            self.keep = (dev(eAj), dev(eAx))
            self.front = (fn, n, WIDTH, pitch, ptr(self.keep[0]), ptr(self.keep[1]))
            if fmt == "hyb":
                coo = tuple(dev(a) for a in hyb_coo(n, tag))
                self.keep += coo
                self.front += (len(coo[0]),) + tuple(ptr(t) for t in coo)

    def run(self, Ap, Aj, Ax, capacity):
        count = ctypes.c_int64(-1)
        fn, *args = self.front
        st = fn(*args, ptr(Ap), None if Aj is None else ctypes.c_void_p(Aj.data_ptr()), None if Ax is None else ctypes.c_void_p(Ax.data_ptr()),
                capacity, ctypes.byref(count), ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream))
        return st, count.value

    def error(self):
        return self.L.cmi_last_error().decode()


WANT = {"ell": want_ell, "dia": want_dia, "hyb": want_hyb}


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("tag", ("f64", "f32"))
@pytest.mark.parametrize("fmt", ("ell", "dia", "hyb"))
def test_to_csr_matches_the_restatement(cmi, torch_cuda, fmt, tag, rows):
    torch = torch_cuda
    wAp, wAj, wAx = WANT[fmt](rows, tag)
    nnz = int(wAp[-1])
    if rows >= 4097:  # the structure the case is about
        lo, hi = empty_stretch(rows)
        assert hi - lo >= 3000 and wAp[hi] == wAp[lo] and wAp[rows] > wAp[rows - 1]
    call = Call(cmi, torch, fmt, rows, tag)
    tdt = torch.float64 if tag == "f64" else torch.float32
    # the sizing call: row offsets and the count, no entries
    Ap = torch.full((rows + 1,), -7, dtype=torch.int32, device="cuda")
    st, count = call.run(Ap, None, None, 0)
    assert st == 0, call.error()
    assert count == nnz
    assert np.array_equal(Ap.cpu().numpy(), wAp)
    # the fill call, at exactly that capacity; what lies behind it stays as it was
    Ap.fill_(-7)
    Aj = torch.full((nnz + GUARD,), -5, dtype=torch.int32, device="cuda")
    Ax = torch.full((nnz + GUARD,), 123.0, dtype=tdt, device="cuda")
    st, count = call.run(Ap, Aj, Ax, nnz)
    assert st == 0, call.error()
    assert count == nnz
    assert np.array_equal(Ap.cpu().numpy(), wAp)
    gAj, gAx = Aj.cpu().numpy(), Ax.cpu().numpy()
    assert np.array_equal(gAj[:nnz], wAj)
    bits = np.uint64 if tag == "f64" else np.uint32
    assert np.array_equal(gAx[:nnz].view(bits), wAx.view(bits))
    assert np.all(gAj[nnz:] == -5) and np.all(gAx[nnz:] == 123.0)


@pytest.mark.parametrize("fmt", ("ell", "dia", "hyb"))
def test_to_csr_refuses_a_capacity_one_below_the_count(cmi, torch_cuda, fmt):
    torch, rows = torch_cuda, 2049
    nnz = int(WANT[fmt](rows, "f64")[0][-1])
    call = Call(cmi, torch, fmt, rows, "f64")
    Ap = torch.empty(rows + 1, dtype=torch.int32, device="cuda")
    Aj = torch.full((nnz,), -5, dtype=torch.int32, device="cuda")
    Ax = torch.zeros(nnz, dtype=torch.float64, device="cuda")
    st, _ = call.run(Ap, Aj, Ax, nnz - 1)
    assert st == INVALID_VALUE
    assert call.error() == f"cmi_{fmt}_to_csr: capacity is smaller than the entry count"
    assert torch.all(Aj == -5).item()  # nothing was scattered


def test_hyb_to_csr_refuses_an_unsorted_coo_part(cmi, torch_cuda):
    torch, rows = torch_cuda, 2049
    call = Call(cmi, torch, "hyb", rows, "f64")
    cAi = call.keep[2]
    cAi[[5, 6]] = cAi[[6, 5]].clone()  # rows 24 and 31 (one entry and two): a descent
    assert cAi[5].item() > cAi[6].item()
    Ap = torch.empty(rows + 1, dtype=torch.int32, device="cuda")
    st, _ = call.run(Ap, None, None, 0)
    assert st == NOT_SUPPORTED
    assert "not sorted by row" in call.error()


def test_dia_to_csr_reports_more_than_int32_max_entries(cmi, torch_cuda):
    """1 048 577 rows x 2048 diagonals of ones, every slot inside the matrix: 2 147 485 696 entries, the smallest input whose count
    passes INT32_MAX with a diagonal count the size check admits.  Sizing call only: nothing is scattered, and no count comes back."""
    torch = torch_cuda
    free, _ = torch.cuda.mem_get_info()
    if free < 12 * 10**9:
        pytest.skip(f"needs one 8.6 GB tensor; {free / 1e9:.1f} GB of device memory are free")
    rows, nd = 1048577, 2048
    assert rows * nd == 2147485696 and rows * nd > 2**31 - 1
    L = cmi.lib()
    vals = torch.ones(rows * nd, dtype=torch.float32, device="cuda")
    off = torch.arange(nd, dtype=torch.int32, device="cuda")
    Ap = torch.empty(rows + 1, dtype=torch.int32, device="cuda")
    count = ctypes.c_int64(-1)
    st = L.cmi_dia_to_csr_f32(rows, rows + nd, nd, rows, ptr(off), ptr(vals), ptr(Ap), None, None, 0, ctypes.byref(count),
                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == NOT_SUPPORTED
    assert L.cmi_last_error().decode() == "conversion to CSR: more than INT32_MAX entries (int32 row offsets cannot address them)"
    assert count.value == -1  # no count is reported
