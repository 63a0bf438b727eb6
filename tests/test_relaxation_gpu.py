"""The fused CSR sweeps of spmv_csr_epilogue.hip and cusp::relaxation on the MI355X (-m gpu): cmi_spmv_csr_axpby_*,
cmi_csr_jacobi_sweep_* and cmi_relax_jacobi_update_* against the numpy restatements of tests/relaxation_refs.py (proved on
the CPU by tests/test_relaxation_refs.py), compared by bit pattern with same_bits; then the C++ device layer's program.

The sweep tiles 256 rows per workgroup and streams their entries through LDS 2048 at a time: the seeded matrices sit one
below, at and one above both sizes.  alpha / beta / omega are 1/3, 0.7 and 2/3 (inexact products, so a contraction or a
reordered epilogue shows) next to the two pairs the smoothers use."""
import os
import subprocess

import numpy as np
import pytest

import relaxation_refs as R
import special_values as sv
from conftest import ROOT, GOLDEN
from special_values import same_bits

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
TILE_ROWS, CHUNK = 256, 2048
SCALARS = ((-1.0, 1.0), (1.0, 0.7), (1.0 / 3.0, 0.7))   # residual, a polynomial step, both products inexact
OMEGAS = (1.0, 2.0 / 3.0)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch


# ------------------------------------------------------------------------------------------------
# matrices: name -> (rows, cols, Ap, Aj), structure only; values and vectors are seeded per type
# ------------------------------------------------------------------------------------------------
def _with_diagonal(rows, lens, seed):
    """Square, every non-empty row holds its diagonal entry (so the Jacobi quotient is finite there); empty rows stay empty."""
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(lens):
        n = int(n)
        if n == 0:
            out.append(np.zeros(0, np.int64))
            continue
        others = rng.choice(np.delete(np.arange(rows), i), size=min(n - 1, rows - 1), replace=False)
        out.append(np.sort(np.r_[others, i]))
    lens = [len(c) for c in out]
    return rows, rows, np.r_[0, np.cumsum(lens)].astype(np.int32), np.concatenate(out + [np.zeros(0, np.int64)]).astype(np.int32)


def _entries_exactly(total, rows, seed):
    """Row lengths 0..(2 * mean) that add up to `total` entries exactly."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 2 * total // rows + 1, size=rows)
    lens[-1] = 0
    while lens.sum() > total:
        lens[int(rng.integers(0, rows - 1))] //= 2
    lens[-1] = total - lens.sum()
    return lens


def _structures():
    out = {}
    g = np.load(os.path.join(GOLDEN, "poisson_100x100.npz"))      # the fixture holds the grid's size (and vectors): the 5-point stencil on it
    m, n = int(g["m"]), int(g["n"])
    r = np.arange(m * n)
    ix, iy = r % m, r // m
    cand = np.stack([r - m, r - 1, r, r + 1, r + m], 1)
    keep = np.stack([iy > 0, ix > 0, np.ones_like(r, bool), ix < m - 1, iy < n - 1], 1)
    out["poisson_100x100"] = (m * n, m * n, np.r_[0, np.cumsum(keep.sum(1))].astype(np.int32), cand[keep].astype(np.int32))
    rng = np.random.default_rng(99)
    for rows in (TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1, 2 * TILE_ROWS + 1):       # around the row tile
        out[f"rows{rows}"] = _with_diagonal(rows, rng.integers(0, 12, size=rows), rows)
    for total in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1):                      # one workgroup, around the LDS pass
        out[f"entries{total}"] = _with_diagonal(200, _entries_exactly(total, 200, total), total)
        assert out[f"entries{total}"][2][-1] == total
    out["empty_rows"] = _with_diagonal(300, np.where(np.arange(300) % 3 == 0, 0, 4), 5)
    out["all_rows_empty"] = (70, 70, np.zeros(71, np.int32), np.zeros(0, np.int32))
    out["one_row"] = _with_diagonal(1, [1], 6)
    out["rows65"] = _with_diagonal(65, np.full(65, 3), 7)
    lens = np.full(3100, 2)
    lens[700] = 3000
    out["long_row"] = _with_diagonal(3100, lens, 8)                                 # one row of 3000 entries among short ones
    return out


def _irregular(dtype):
    g = np.load(os.path.join(GOLDEN, "irregular_1500x1237.npz"))
    p = "f64" if dtype == np.float64 else "f32"
    return int(g["rows"]), int(g["cols"]), g[p + "_Ap"].astype(np.int32), g[p + "_Aj"].astype(np.int32)


_cache = {}


def case(name, dtype):
    """(rows, cols, Ap, Aj, Ax, x, z, diag, b) for a matrix and value type, seeded; made once."""
    key = (name, np.dtype(dtype).name)
    if key not in _cache:
        if "structures" not in _cache:
            _cache["structures"] = _structures()
        rows, cols, Ap, Aj = _irregular(dtype) if name == "irregular_1500x1237" else _cache["structures"][name]
        rng = np.random.default_rng(sum(map(ord, name)))
        Ax = rng.standard_normal(len(Aj)).astype(dtype)
        x, z, b = (rng.standard_normal(n).astype(dtype) for n in (cols, rows, rows))
        diag = R.extract_diagonal(Ap, Aj, Ax) if rows == cols else None
        _cache[key] = (rows, cols, Ap, Aj, Ax, x, z, diag, b)
    return _cache[key]


def want_axpby(name, dtype, alpha, beta):
    key = ("axpby", name, np.dtype(dtype).name, alpha, beta)
    if key not in _cache:
        rows, cols, Ap, Aj, Ax, x, z, _, _ = case(name, dtype)
        _cache[key] = R.spmv_axpby(Ap, Aj, Ax, x, alpha, beta, z)
    return _cache[key]


def want_jacobi(name, dtype, omega):
    key = ("jacobi", name, np.dtype(dtype).name, omega)
    if key not in _cache:
        rows, cols, Ap, Aj, Ax, x, _, diag, b = case(name, dtype)
        _cache[key] = R.jacobi_sweep(Ap, Aj, Ax, diag, b, x, omega)
    return _cache[key]


SQUARE = ["poisson_100x100", "rows255", "rows256", "rows257", "rows513", "entries2047", "entries2048", "entries2049", "entries4097",
          "empty_rows", "all_rows_empty", "one_row", "rows65", "long_row"]
ALL = SQUARE + ["irregular_1500x1237"]


def dev(a, torch):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def plans_for(cmi, torch, name, dtype, rows, cols, dAp, dAj):
    """The sweep keeps its own tiling: a plan is checked for format and value type and otherwise not used, so every plan runs the
    same kernel.  What is tested is that no valid plan class is refused or changes the result -- on the stencil only: made from
    the row offsets alone, with the columns (what csr_matrix::plan() makes), with the opt-in 16-bit column copy, and the wave
    tiles and run-compressed columns asked for by name.  Every other matrix runs without a plan."""
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    out = [("no plan", None)]
    if name == "poisson_100x100":
        out += [("plan", cmi.Plan(cmi.FORMAT_CSR, tdt, rows, cols, len(dAj), dAp)),
                ("plan with columns", cmi.Plan.csr(tdt, rows, cols, dAp, dAj)),
                ("16-bit columns", cmi.Plan.csr(tdt, rows, cols, dAp, dAj, cfg=cmi.Config(kernel=cmi.CSR_STREAM_C16))),
                ("wave tiles", cmi.Plan(cmi.FORMAT_CSR, tdt, rows, cols, len(dAj), dAp, cmi.Config(kernel=cmi.CSR_STREAM_WAVE))),
                ("run-compressed columns", cmi.Plan.csr(tdt, rows, cols, dAp, dAj, cfg=cmi.Config(kernel=cmi.CSR_STREAM_WAVER, items_per_thread=1)))]
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ALL)
def test_axpby_form_bit_exact(cmi, torch_cuda, name, dtype):
    torch = torch_cuda
    rows, cols, Ap, Aj, Ax, x, z, _, _ = case(name, dtype)
    dAp, dAj, dAx, dx, dz = (dev(a, torch) for a in (Ap, Aj, Ax, x, z))
    for pname, plan in plans_for(cmi, torch, name, dtype, rows, cols, dAp, dAj):
        for alpha, beta in SCALARS:
            want = want_axpby(name, dtype, alpha, beta)
            out = torch.full_like(dz, 7.0)
            cmi.spmv_csr_axpby(rows, cols, dAp, dAj, dAx, dx, alpha, beta, dz, out, plan=plan)
            same_bits(out.cpu().numpy(), want, f"{name} {pname} alpha={alpha} beta={beta}")
            same_bits(dz.cpu().numpy(), z, "z is read only")
            inplace = dz.clone()                                    # out is z
            cmi.spmv_csr_axpby(rows, cols, dAp, dAj, dAx, dx, alpha, beta, inplace, inplace, plan=plan)
            same_bits(inplace.cpu().numpy(), want, f"{name} {pname} in place alpha={alpha} beta={beta}")
    # arrays that are only 4-byte (8-byte) aligned: the scalar-load instance, same bits
    if len(Aj):
        oAj, oAx = dev(np.r_[Aj[:1], Aj], torch)[1:], dev(np.r_[Ax[:1], Ax], torch)[1:]
        assert oAj.data_ptr() % 16 != 0 and oAx.data_ptr() % 16 != 0
        out = torch.full_like(dz, 7.0)
        cmi.spmv_csr_axpby(rows, cols, dAp, oAj, oAx, dx, 1.0 / 3.0, 0.7, dz, out)
        same_bits(out.cpu().numpy(), want_axpby(name, dtype, 1.0 / 3.0, 0.7), f"{name} unaligned")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", SQUARE)
def test_jacobi_form_bit_exact(cmi, torch_cuda, name, dtype):
    torch = torch_cuda
    rows, cols, Ap, Aj, Ax, x, _, diag, b = case(name, dtype)
    dAp, dAj, dAx, dx, dd, db = (dev(a, torch) for a in (Ap, Aj, Ax, x, diag, b))
    for pname, plan in plans_for(cmi, torch, name, dtype, rows, cols, dAp, dAj):
        for omega in OMEGAS:
            want = want_jacobi(name, dtype, omega)
            out = torch.full_like(dx, 7.0)
            cmi.csr_jacobi_sweep(rows, dAp, dAj, dAx, dd, db, dx, omega, out, plan=plan)
            same_bits(out.cpu().numpy(), want, f"{name} {pname} omega={omega}")
            same_bits(dx.cpu().numpy(), x, "x is read only")
    # the unfused pair: any multiply, then the elementwise update in place -- the same bits
    omega = OMEGAS[1]
    y = torch.from_numpy(R.row_sums(Ap, Aj, Ax, x)).cuda()
    xin = dx.clone()
    cmi.relax_jacobi_update(dd, db, y, omega, xin)
    same_bits(xin.cpu().numpy(), want_jacobi(name, dtype, omega), f"{name} elementwise update")
    if len(Aj):
        oAj, oAx = dev(np.r_[Aj[:1], Aj], torch)[1:], dev(np.r_[Ax[:1], Ax], torch)[1:]
        out = torch.full_like(dx, 7.0)
        cmi.csr_jacobi_sweep(rows, dAp, oAj, oAx, dd, db, dx, omega, out)
        same_bits(out.cpu().numpy(), want_jacobi(name, dtype, omega), f"{name} unaligned")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("mname", ["poisson100", "irregular"])
def test_special_value_decks(cmi, torch_cuda, mname, dtype):
    """NaN / inf next to over-fetched columns, signed zeros, subnormals, an overflow that only storage order produces: the decks of
    tests/special_values.py through both forms (the rectangular matrix: the axpby form only)."""
    torch = torch_cuda
    M = sv.matrices(dtype)[mname]
    dAp, dAj = dev(M.Ap, torch), dev(M.Aj, torch)
    for dname, (Ax, x, y0) in sv.decks(M, dtype).items():
        dAx, dx, dz = dev(Ax, torch), dev(x, torch), dev(y0, torch)
        for alpha, beta in SCALARS[::2]:
            out = torch.full_like(dz, 7.0)
            cmi.spmv_csr_axpby(M.rows, M.cols, dAp, dAj, dAx, dx, alpha, beta, dz, out)
            same_bits(out.cpu().numpy(), R.spmv_axpby(M.Ap, M.Aj, Ax, x, alpha, beta, y0), f"{mname} {dname} axpby {alpha} {beta}")
        if M.rows == M.cols:
            diag = R.extract_diagonal(M.Ap, M.Aj, Ax)
            out = torch.full_like(dx, 7.0)
            cmi.csr_jacobi_sweep(M.rows, dAp, dAj, dAx, dev(diag, torch), dz, dx, 2.0 / 3.0, out)
            with np.errstate(all="ignore"):
                same_bits(out.cpu().numpy(), R.jacobi_sweep(M.Ap, M.Aj, Ax, diag, y0, x, 2.0 / 3.0), f"{mname} {dname} jacobi")


def test_zero_rows_and_refused_arguments(cmi, torch_cuda):
    torch = torch_cuda
    e32, e64 = torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.float64, device="cuda")
    Ap0 = torch.zeros(1, dtype=torch.int32, device="cuda")
    cmi.spmv_csr_axpby(0, 0, Ap0, e32, e64, e64, 1.0, 1.0, e64, e64.clone())
    cmi.csr_jacobi_sweep(0, Ap0, e32, e64, e64, e64, e64, 1.0, e64.clone())
    cmi.relax_jacobi_update(e64, e64, e64, 1.0, e64.clone())
    rows, cols, Ap, Aj, Ax, x, z, diag, b = case("rows65", np.float64)
    dAp, dAj, dAx, dx, dz, dd, db = (dev(a, torch) for a in (Ap, Aj, Ax, x, z, diag, b))
    with pytest.raises(cmi.CmiError) as e:   # the output is x
        cmi.spmv_csr_axpby(rows, cols, dAp, dAj, dAx, dx, 1.0, 1.0, dz, dx)
    assert e.value.status == 1 and "overlaps" in str(e.value)
    for bad in (dx, dd, db):                 # the Jacobi output is x, diag or b
        with pytest.raises(cmi.CmiError) as e:
            cmi.csr_jacobi_sweep(rows, dAp, dAj, dAx, dd, db, dx, 1.0, bad)
        assert e.value.status == 1 and "overlaps" in str(e.value)
    # a plan of another value type or another format is refused; nothing was written
    wrong = [cmi.Plan.csr(torch.float32, rows, cols, dAp, dAj),
             cmi.Plan.coo(torch.float64, rows, cols, dev(np.repeat(np.arange(rows, dtype=np.int32), np.diff(Ap)), torch), dAj)]
    for plan in wrong:
        out = torch.full_like(dz, 7.0)
        with pytest.raises(cmi.CmiError) as e:
            cmi.spmv_csr_axpby(rows, cols, dAp, dAj, dAx, dx, 1.0, 1.0, dz, out, plan=plan)
        assert e.value.status == 1 and "plan" in str(e.value)
        with pytest.raises(cmi.CmiError):
            cmi.csr_jacobi_sweep(rows, dAp, dAj, dAx, dd, db, dx, 1.0, out, plan=plan)
        assert bool((out == 7.0).all())


def test_relaxation_cpp_device_layer(cmi, tmp_path):
    """tests/relaxation/test_relax_device.cpp: the reference's cases on all five formats, every format against the host restatement bit
    for bit, x.data() unchanged by a sweep, two successive polynomial calls on one object, views, empty rows."""
    inc = os.path.join(ROOT, "cusp-autotuned_amd", "include")
    libd = os.path.join(ROOT, "cusp-autotuned_amd", "lib")
    exe = tmp_path / "test_relax_device"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fopenmp", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off",
                        f"-I{inc}", f"-I{os.path.join(ROOT, 'tests', 'cpp')}", os.path.join(ROOT, "tests", "relaxation", "test_relax_device.cpp"),
                        "-o", str(exe), f"-L{libd}", "-lcusp_mi355x", f"-Wl,-rpath,{libd}", "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "43 tests, 0 failed" in r.stdout
