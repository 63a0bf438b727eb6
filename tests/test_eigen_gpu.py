"""GPU tests of cusp::eigen's kernels (csrc/eigen.hip) through binding.py, with every output between NaN guard elements, and of
the header layer on device_memory (tests/eigen/test_eigen_device.cpp).

Row sums are checked against the exactly rounded sum S of |a| over the row (math.fsum): |got - S| <= len * u * S with
u = 2^-53 (f64) / 2^-24 (f32) -- the standard bound for a sum of len non-negative terms in any order, so it needs no measurement;
rows of length <= 1 must be exact.  cmi_random_fill_* and cmi_blas_scal_recip_* are checked bit for bit against the numpy
restatements of tests/eigen_refs.py."""
import math
import os
import subprocess

import numpy as np
import pytest

import eigen_refs as E
from conftest import ROOT

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 3, 63, 64, 65, 255, 257, 1023, 1025, 4099, 70001)
GUARD = 4


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


def tdtype(torch, dtype):
    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


def dev(a, torch):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(torch, n, dtype, content=None, pad=GUARD):
    """(whole, view): n elements between `pad` NaN guard elements on either side."""
    whole = torch.full((n + 2 * pad,), float("nan"), dtype=tdtype(torch, dtype), device="cuda")
    view = whole[pad:pad + n]
    if content is not None:
        view.copy_(dev(np.asarray(content, dtype), torch))
    return whole, view


def guards_intact(whole, n, pad=GUARD):
    h = whole.cpu().numpy()
    return bool(np.all(np.isnan(h[:pad])) and np.all(np.isnan(h[pad + n:])))


def within_bound(got, S, lengths, dtype):
    """|got - S| <= len u S per row; exact for rows of length <= 1; a NaN / inf sum is matched as such."""
    u = 2.0 ** -53 if np.dtype(dtype) == np.float64 else 2.0 ** -24
    bad = []
    for i, (g, s, n) in enumerate(zip(got.astype(np.float64), S, lengths)):
        if math.isnan(s):
            ok = math.isnan(g)
        elif math.isinf(s):
            ok = g == s
        elif n <= 1:
            ok = g == float(np.dtype(dtype).type(s)) and not np.signbit(g)
        else:
            ok = abs(g - s) <= n * u * s
        if not ok:
            bad.append((i, g, s, int(n)))
    return bad


# ---- CSR ----------------------------------------------------------------------------------------------------------------
def csr_from_lengths(lengths, dtype, seed):
    rng = np.random.default_rng(seed)
    Ap = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    Ax = ((rng.random(int(Ap[-1])) - 0.5) * 16).astype(dtype)
    return Ap, Ax


def csr_cases(dtype):
    one = (np.array([0, 1], np.int32), np.array([-3.5], dtype))
    twos = csr_from_lengths(np.full(193, 2), dtype, 1)
    P = E.poisson5pt(37, 41, dtype)
    poisson = (np.concatenate([[0], np.cumsum((P != 0).sum(1))]).astype(np.int32), P[P != 0])
    lengths = np.random.default_rng(2).integers(0, 9, 300)
    lengths[[0, 7, 8, 150, 299]] = 0
    lengths[151] = 3000
    mixed = csr_from_lengths(lengths, dtype, 3)
    mixed[1][::5] = -0.0
    lengths = np.full(500, 3)
    lengths[257] = 100000
    long_row = csr_from_lengths(lengths, dtype, 4)
    special = csr_from_lengths(np.array([3, 70, 1, 0, 40, 2500, 4, 4]), dtype, 5)
    special[1][special[0][1] + 33] = -np.inf   # the row of 70
    special[1][special[0][4] + 39] = np.nan    # the row of 40
    special[1][special[0][5] + 2047] = np.inf  # the row of 2500: across a chunk
    return {"1x1": one, "193 rows of 2": twos, "poisson37x41": poisson, "empty rows, -0, a row of 3000": mixed,
            "a row of 100000 among rows of 3": long_row, "inf and nan rows": special}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("misalign", [0, 1])
def test_csr_abs_row_sums(cmi, torch_cuda, dtype, misalign):
    """Every case with Ax at a 16-byte boundary and one element past it (the chunk starts follow the alignment of Ax)."""
    torch = torch_cuda
    for name, (Ap, Ax) in csr_cases(dtype).items():
        n = len(Ap) - 1
        S = E.csr_abs_row_sums(Ap, Ax)
        store = torch.zeros(len(Ax) + 4, dtype=tdtype(torch, dtype), device="cuda")
        dAx = store[misalign:misalign + len(Ax)]
        dAx.copy_(dev(Ax, torch))
        assert dAx.data_ptr() % 16 == misalign * np.dtype(dtype).itemsize
        whole, out = guarded(torch, n, dtype)
        cmi.csr_abs_row_sums(n, dev(Ap, torch), dAx, out)
        got = out.cpu().numpy()
        assert guards_intact(whole, n), name
        bad = within_bound(got, S, E.row_lengths(Ap), dtype)
        assert not bad, (name, bad[:5])
        # accumulate: one add onto what the array holds
        before = ((np.arange(n) % 7) - 2.5).astype(dtype)
        whole, out = guarded(torch, n, dtype, before)
        cmi.csr_abs_row_sums(n, dev(Ap, torch), dAx, out, accumulate=True)
        assert guards_intact(whole, n), name
        with np.errstate(invalid="ignore"):
            assert np.array_equal(out.cpu().numpy(), before + got, equal_nan=True), name
        # the largest of them through cmi_blas_amax_*: the same bits
        if not np.any(np.isnan(got)):
            value = torch.full((1,), -1.0, dtype=tdtype(torch, dtype), device="cuda")
            cmi.blas_amax(dev(got, torch), value, None, cmi.blas_workspace())
            assert value.cpu().numpy()[0].tobytes() == got.max().tobytes(), name


# ---- ELL, DIA, HYB ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("width", [1, 5, 33])
def test_ell_abs_row_sums(cmi, torch_cuda, dtype, width):
    torch = torch_cuda
    rows, pitch = 301, 320
    rng = np.random.default_rng(width)
    Ax = ((rng.random(width * pitch) - 0.5) * 16).astype(dtype)
    lengths = rng.integers(0, width + 1, rows)
    for i in range(rows):
        Ax[np.arange(lengths[i], width) * pitch + i] = 0          # padding holds 0
    Ax.reshape(width, pitch)[:, rows:] = np.nan                     # beyond the rows: never read
    S = E.ell_abs_row_sums(rows, width, pitch, Ax)
    whole, out = guarded(torch, rows, dtype)
    cmi.ell_abs_row_sums(rows, rows, width, pitch, dev(Ax, torch), out)
    got = out.cpu().numpy()
    assert guards_intact(whole, rows)
    bad = within_bound(got, S, np.full(rows, width), dtype)
    assert not bad, bad[:5]
    # the fork's row lengths: the leading slots only (slots behind them hold NaN here)
    Ar = Ax.copy()
    for i in range(rows):
        Ar[np.arange(lengths[i], width) * pitch + i] = np.nan
    whole, out = guarded(torch, rows, dtype)
    cmi.ell_abs_row_sums(rows, rows, width, pitch, dev(Ar, torch), out, row_lengths=dev(lengths.astype(np.int32), torch))
    assert guards_intact(whole, rows)
    assert not within_bound(out.cpu().numpy(), E.ell_abs_row_sums(rows, width, pitch, Ar, lengths), lengths, dtype)
    # accumulate
    before = ((np.arange(rows) % 5) + 0.25).astype(dtype)
    whole, out = guarded(torch, rows, dtype, before)
    cmi.ell_abs_row_sums(rows, rows, width, pitch, dev(Ax, torch), out, accumulate=True)
    assert guards_intact(whole, rows) and np.array_equal(out.cpu().numpy(), before + got)


@pytest.mark.parametrize("tag,dtype", [("f64", np.float64), ("f32", np.float32)])
def test_dia_abs_row_sums_banded(cmi, torch_cuda, golden_banded, tag, dtype):
    """700 x 900, ten diagonals; NaN stored wherever the column falls outside the matrix and in the pitch rows: never read into a sum."""
    torch, g = torch_cuda, golden_banded
    rows, cols, pitch = int(g["rows"]), int(g["cols"]), int(g["pitch"])
    off = g["offsets"]
    vals = g[f"{tag}_vals"].copy()
    for d, o in enumerate(off):
        i = np.arange(pitch)
        vals[d * pitch + i[(i >= rows) | (i + int(o) < 0) | (i + int(o) >= cols)]] = np.nan
    S = E.dia_abs_row_sums(rows, cols, pitch, off, vals)
    assert not np.any(np.isnan(S)) and np.any(np.isnan(vals))
    lengths = np.array([sum(0 <= i + int(o) < cols for o in off) for i in range(rows)])
    whole, out = guarded(torch, rows, dtype)
    cmi.dia_abs_row_sums(rows, cols, len(off), pitch, dev(off, torch), dev(vals, torch), out)
    got = out.cpu().numpy()
    assert guards_intact(whole, rows)
    bad = within_bound(got, S, lengths, dtype)
    assert not bad, bad[:5]
    before = ((np.arange(rows) % 3) - 1.5).astype(dtype)
    whole, out = guarded(torch, rows, dtype, before)
    cmi.dia_abs_row_sums(rows, cols, len(off), pitch, dev(off, torch), dev(vals, torch), out, accumulate=True)
    assert guards_intact(whole, rows) and np.array_equal(out.cpu().numpy(), before + got)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_hyb_abs_row_sums(cmi, torch_cuda, dtype):
    """As ELL plus the COO part accumulated: a HYB matrix converted on the device from rows of 0..9 entries and one of 400."""
    torch = torch_cuda
    lengths = np.random.default_rng(9).integers(0, 10, 777)
    lengths[400] = 400
    Ap, Ax = csr_from_lengths(lengths, dtype, 10)
    Aj = np.concatenate([np.arange(n) for n in lengths]).astype(np.int32)
    A = cmi.CsrMatrix(777, 777, len(Ax), dev(Ap, torch), dev(Aj, torch), dev(Ax, torch))
    H = cmi.convert(A, "hyb", num_entries_per_row=4)
    assert H.coo.num_entries > 0 and H.ell.pitch > 777
    S = E.hyb_abs_row_sums(777, 4, H.ell.pitch, H.ell.values.cpu().numpy(), H.coo.row_indices.cpu().numpy(), H.coo.values.cpu().numpy())
    assert np.array_equal(S, E.csr_abs_row_sums(Ap, Ax))
    whole, out = guarded(torch, 777, dtype)
    assert cmi.abs_row_sums(H, out) is out
    assert guards_intact(whole, 777)
    bad = within_bound(out.cpu().numpy(), S, np.maximum(lengths, 4), dtype)   # the ELL part adds its padding zeros too
    assert not bad, bad[:5]
    assert cmi.disks_spectral_radius(H) == float(out.max().item())


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("fmt", ["csr", "coo", "ell", "dia", "hyb"])
def test_disks_spectral_radius_poisson(cmi, torch_cuda, fmt, dtype):
    A = cmi.poisson5pt(37, 41, fmt, dtype=tdtype(torch_cuda, dtype))
    assert cmi.disks_spectral_radius(A) == 8.0


# ---- the start vector and the normalise step ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_random_fill(cmi, torch_cuda, dtype):
    torch = torch_cuda
    for n in SIZES:
        filled = []
        for seed in (0, 0x123456789ABCDEF):
            for pad in (GUARD, 3):   # 16-byte aligned or not: the values depend on the position alone
                whole, x = guarded(torch, n, dtype, pad=pad)
                cmi.random_fill(x, seed)
                got = x.cpu().numpy()
                assert guards_intact(whole, n, pad), (n, seed)
                assert got.tobytes() == E.random_fill(n, seed, dtype).tobytes(), (n, seed)
                assert np.all(got >= 0) and np.all(got < 1)
            filled.append(got)
        if n >= 2:
            assert not np.array_equal(filled[0], filled[1])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("squared", [False, True])
def test_blas_scal_recip(cmi, torch_cuda, dtype, squared):
    """s a value of the vector's type (cmi_blas_amax_*'s result) or a double holding a squared norm (cmi_blas_axpy_dot_*'s result with
    u = w): the bits of the host sequence beta = nrm2(w); scal(w, T(1) / beta)."""
    torch = torch_cuda
    ws = cmi.blas_workspace()
    for n in SIZES:
        for pad in (GUARD, 3):
            x0 = ((E.random_fill(n, 5, dtype) - dtype(0.25)) * dtype(6)).astype(dtype)
            whole, x = guarded(torch, n, dtype, x0, pad=pad)
            if squared:
                s = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
                cmi.blas_axpy_dot(None, None, x, x, s, ws)
            else:
                s = torch.full((1,), -1.0, dtype=tdtype(torch, dtype), device="cuda")
                cmi.blas_amax(x, s, None, ws)
            s_host = s.cpu().numpy()[0]
            if n == 0:
                s_host = np.float64(4.0)   # nothing to take a norm of: any scalar
                s.fill_(4.0)
            s_out = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
            cmi.blas_scal_recip(s, x, squared, s_out)
            assert guards_intact(whole, n, pad), n
            assert x.cpu().numpy().tobytes() == E.scal_recip(x0, s_host, squared).tobytes(), (n, pad)
            want_s = np.dtype(dtype).type(np.sqrt(np.float64(s_host))) if squared else np.dtype(dtype).type(s_host)
            assert s_out.cpu().numpy()[0] == np.float64(want_s), n
    # without s_out
    whole, x = guarded(torch, 65, dtype, np.full(65, 3.0))
    cmi.blas_scal_recip(dev(np.array([4.0], np.float64 if squared else dtype), torch), x, squared)
    assert guards_intact(whole, 65) and np.array_equal(x.cpu().numpy(), np.full(65, 1.5 if squared else 0.75, dtype))


# ---- the header layer ---------------------------------------------------------------------------------------------------
def test_eigen_cpp_device_layer(cmi, tmp_path):
    """tests/eigen/test_eigen_device.cpp: the host program's matrices and criterion in device_memory, all five formats, f32 and f64."""
    import test_eigen_host as H
    exe = tmp_path / "test_eigen_device"
    r = subprocess.run(["g++", *H.CXXFLAGS, os.path.join(ROOT, "tests", "eigen", "test_eigen_device.cpp"), "-o", str(exe), *H.LDFLAGS],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert H.HOST_TESTS in r.stdout
