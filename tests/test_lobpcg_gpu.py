"""GPU tests (-m gpu) of the LOBPCG kernels of csrc/lobpcg.hip through binding.py and of the header layer on device_memory
(tests/lobpcg/test_lobpcg_device.cpp), in the shape of tests/test_blas_extra_gpu.py.

Bars for every kernel case (references: tests/lobpcg_refs.py, checked on the CPU by tests/test_lobpcg_refs.py):
  * output vectors BIT-EQUAL to the numpy restatement in T (the library is built with -ffp-contract=off); guard elements round every operand
    and every const operand unchanged;
  * every reduction within 1e-12 * sum|terms| of the exact sum of the products of the vectors the kernel RETURNED (check_sums' bound in
    tests/test_blas_extra_gpu.py; math.fsum; at GRID_N a pairwise longdouble sum, whose own error is below 30 * 2^-64 * sum|terms| = 2e-18);
  * the host mirror equals the device scalar bit for bit; the workspace holds NaNs before the first call; a second call on restored inputs
    gives the same bits.
Sizes.  kBlasBlock = 256 lanes, a lane owns one 16-byte piece (2 doubles / 4 floats); the grid rule is multi_sum_grid(n, W, 8) of
csrc/blas1_shared.h: one workgroup per 256 pieces up to multi_sum_cap(8) = kPartialCapacity / 8 = 16384 workgroups, grid-strided past that.
GRID_N[T] = 16384 * 256 * W + 5 is just past one full grid stride: the first lanes make a second trip (a full piece and a ragged one)."""
import functools
import subprocess

import numpy as np
import pytest

import lobpcg_refs as R
import special_values as sv
from test_blas_extra_gpu import Operand, bits, scalar

pytestmark = pytest.mark.gpu

TYPES = {"f32": np.float32, "f64": np.float64}
K_BLAS_BLOCK = 256                      # csrc/blas1_shared.h kBlasBlock
K_LIST_CAP = (1 << 17) // 8             # csrc/blas1_shared.h multi_sum_cap(8) with common.h kPartialCapacity = 2^17
GRID_N = {np.float32: K_LIST_CAP * K_BLAS_BLOCK * 4 + 5, np.float64: K_LIST_CAP * K_BLAS_BLOCK * 2 + 5}
SIZES = (0, 1, 3, 64, 257, 4099)
NAMES = ("residual", "gram", "gram_first", "update", "update_first", "update_no_r")
MIRRORED = ("residual", "update", "update_first")
NAN = float("nan")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def ws(cmi, torch_cuda):
    return cmi.blas_workspace()


@functools.lru_cache(maxsize=None)
def pool(T):
    """One seeded draw per type, shared (read-only) by every case: operand j starts 1009 j elements in."""
    a = np.random.default_rng(2026).standard_normal(GRID_N[T] + 8 * 1009).astype(T)
    a.setflags(write=False)
    return a


def host_inputs(kernel, T, n):
    return {name: pool(T)[j * 1009:j * 1009 + n] for j, name in enumerate(kernel.vecs)}


def call(cmi, torch, name, s, o, ws, mirror):
    """One launch; returns the reduction results as {name: 1-element float64 device tensor view}."""
    if name == "residual":
        lam, rr = scalar(torch, s["lambda"]), scalar(torch, NAN)
        cmi.lobpcg_residual(lam, o["x"], o["ax"], o["r"], rr, ws, mirror=mirror)
        assert float(lam) == s["lambda"]
        return {"rr": rr}
    if name in ("gram", "gram_first"):
        first = name == "gram_first"
        pp = None if first else scalar(torch, s["pp"])
        out = torch.full((8,), NAN, dtype=torch.float64, device="cuda")
        cmi.lobpcg_gram(pp, o["x"], o["w"], o["aw"], None if first else o["p"], None if first else o["ap"], out, ws)
        if first:
            assert bool(torch.isnan(out[3:]).all()), "the first-iteration form writes three sums only"
        else:
            assert float(pp) == s["pp"]
        return {k: out[j:j + 1] for j, k in enumerate(R.GRAM_SUMS[:3 if first else 8])}
    out = torch.full((2,), NAN, dtype=torch.float64, device="cuda")
    with_r = name != "update_no_r"
    cmi.lobpcg_update(s["cx"], s["cr"], s["cp"], name == "update_first", s["lambda_new"], o["w"], o["aw"], o["p"], o["ap"], o["x"], o["ax"],
                      o["r"] if with_r else None, out, ws, mirror=mirror)
    if not with_r:
        assert bool(torch.isnan(out[0])), "r == NULL leaves scalars_dev[0] alone"
        return {"pp": out[1:2]}
    return {"rr": out[0:1], "pp": out[1:2]}


def quick_sum(a, b):
    H = np.longdouble
    prod = a.astype(H) * b.astype(H)
    return float(np.sum(prod)), float(np.sum(np.abs(prod)))


def run_case(cmi, torch, ws, mirror, name, T, n, offs, kind="inexact", vectors=None, exact=True):
    """One call (made twice) of one kernel on views at the given element offsets (a dict per operand, or one int for all)."""
    kernel = R.KERNELS[name]
    what = f"{name} {np.dtype(T).name} n={n} offsets={offs} {kind}"
    if isinstance(offs, int):
        offs = {v: offs for v in kernel.vecs}
    s, v = R.scalars_for(kernel, kind, T), vectors or host_inputs(kernel, T, n)
    ops = {vn: Operand(torch, T, v[vn], offs[vn]) for vn in kernel.vecs}
    views = {vn: op.view for vn, op in ops.items()}
    m = mirror if name in MIRRORED else None
    with np.errstate(all="ignore"):
        want = kernel.restate(T, s, v)
    runs = []
    for trip in range(2):
        if trip:
            for op in ops.values():
                op.restore(torch)
        else:
            ws.fill_(NAN)  # nothing in the workspace may need initialising; the second call finds the first one's leavings
        res = call(cmi, torch, name, s, views, ws, m)
        mirrored = m.wait() if m is not None else None
        after = {vn: op.after() for vn, op in ops.items()}
        for vn in kernel.const:
            assert bits(after[vn]) == bits(ops[vn].before), f"{what}: const operand {vn} changed"
        if m is not None:
            assert bits(np.float64(mirrored)) == bits(res["rr"].cpu().numpy()), f"{what}: host mirror differs from the device scalar"
        runs.append((after, {rn: bits(t.cpu().numpy()) for rn, t in res.items()}))
        if trip == 0:
            got = {out: ops[out].inner(after[out]) for out in kernel.outputs}
            for out in kernel.outputs:
                if exact:
                    assert bits(got[out]) == bits(want[out]), f"{what}: {out} differs from the restatement at {np.nonzero(got[out] != want[out])[0][:5]}"
                else:
                    sv.same_bits(got[out], want[out], f"{what}: {out}")
            if exact:
                named = kernel.sums(T, got, v)
                assert sorted(named) == sorted(res)
                for rname, (a, b) in named.items():
                    total, absolute = quick_sum(a, b) if n > 1 << 20 else R.exact_sum(a, b)
                    dev = float(res[rname])
                    print(f"{what}: {rname} = {dev!r}, exact {total!r}, |error| / sum|terms| = {abs(dev - total) / absolute if absolute else 0.0:.3g}")
                    assert abs(dev - total) <= 1e-12 * absolute, f"{what}: {rname} = {dev!r}, exact {total!r}"
                    if n == 0:
                        assert bits(np.float64(dev)) == bits(np.float64(0.0)), f"{what}: n == 0 stores zeros"
    if exact:
        assert all(bits(runs[0][0][vn]) == bits(runs[1][0][vn]) for vn in kernel.vecs) and runs[0][1] == runs[1][1], f"{what}: the second call gave other bits"
    else:
        for vn in kernel.vecs:
            sv.same_bits(runs[0][0][vn], runs[1][0][vn], f"{what}: second call, {vn}")


@pytest.mark.parametrize("tname", list(TYPES))
@pytest.mark.parametrize("name", NAMES)
def test_kernel_against_restatement(cmi, torch_cuda, ws, name, tname):
    """Every size, all operands aligned (the 16-byte path) and each operand in turn one element off it (the element path)."""
    T = TYPES[tname]
    kernel = R.KERNELS[name]
    mirror = cmi.HostScalar()
    try:
        for n in SIZES:
            run_case(cmi, torch_cuda, ws, mirror, name, T, n, 0)
            for odd in (kernel.vecs if n else ()):
                run_case(cmi, torch_cuda, ws, mirror, name, T, n, {vn: int(vn == odd) for vn in kernel.vecs})
        run_case(cmi, torch_cuda, ws, mirror, name, T, 4099, 0, kind="exact")   # representable scalars: s = 1 / 2 exactly, and so on
        run_case(cmi, torch_cuda, ws, mirror, name, T, 4099, 1)                  # every operand off the grid by the same element
    finally:
        mirror.close()


@pytest.mark.parametrize("tname", list(TYPES))
@pytest.mark.parametrize("name", ["residual", "gram", "update"])
def test_kernel_past_one_grid_stride(cmi, torch_cuda, ws, name, tname):
    """n = GRID_N: multi_sum_cap(8) = 16384 workgroups of 256 lanes cover the first GRID_N - 5 elements in one trip; the first two lanes of the
    grid make a second one."""
    T = TYPES[tname]
    assert GRID_N[T] == 16384 * 256 * (16 // np.dtype(T).itemsize) + 5
    mirror = cmi.HostScalar()
    try:
        run_case(cmi, torch_cuda, ws, mirror, name, T, GRID_N[T], 0)
    finally:
        mirror.close()


@pytest.mark.parametrize("tname", list(TYPES))
def test_special_values_go_through_bit_for_bit(cmi, torch_cuda, ws, tname):
    """The decks of tests/special_values.py (NaN and infinity near misses, signed zeros, subnormals, overflow) on its 100 x 100 stencil (n = 10000): the three
    arrays of a deck, cycled and reversed, are the operands; the element-wise outputs are the restatement's bits (NaN against NaN at the same
    position, whatever the payload).  The sums of such operands are not looked at."""
    T = TYPES[tname]
    M = sv.matrices(T)["poisson100"]
    n = M.rows
    assert M.cols == n and M.nnz >= 2 * n
    mirror = cmi.HostScalar()
    try:
        for dname, (Ax, x, y0) in sv.decks(M, T).items():
            source = (x, y0, Ax[:n], x[::-1], y0[::-1], Ax[n:2 * n], (x + y0).astype(T))
            for name in ("residual", "gram", "update", "update_first"):
                kernel = R.KERNELS[name]
                with np.errstate(all="ignore"):
                    vectors = {vn: np.ascontiguousarray(source[j]) for j, vn in enumerate(kernel.vecs)}
                for off in (0, 1):
                    run_case(cmi, torch_cuda, ws, mirror, name, T, n, off, vectors=vectors, exact=False)
    finally:
        mirror.close()


# ---- the header layer ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_program(cmi, tmp_path_factory):
    import test_lobpcg_host as H
    return H.build(tmp_path_factory.mktemp("lobpcg_device"), "test_lobpcg_device.cpp", "test_lobpcg_device")


def test_lobpcg_cpp_device_layer(device_program):
    """tests/lobpcg/test_lobpcg_device.cpp: the host program's unit tests in device_memory -- all five formats, a linear_operator, array2d X,
    the cap, the breakdown rule, the shape exceptions."""
    import test_lobpcg_host as H
    r = subprocess.run([str(device_program)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert H.HOST_TESTS in r.stdout


def test_device_solver_cases_fused_and_unfused(device_program):
    """Every case of the host table on device_memory: the fused path and the $CMI_LOBPCG_FUSED=0 path each meet the host's bars, their
    eigenvalues agree within 2 x tolerance, and the fused path run twice returns the same bits."""
    import test_lobpcg_host as H
    r = subprocess.run([str(device_program), "cases"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = H.parse_cases(r.stdout)
    assert len(rows) == 3 * len(R.CASES)
    for k, case in enumerate(R.CASES):
        first, second, plain = rows[3 * k:3 * k + 3]
        assert first["case"] == second["case"] == plain["case"] == case
        assert (first["run"], second["run"], plain["run"]) == ("fused", "fused", "unfused")
        for row in (first, second, plain):
            H.check_case(row)
        assert abs(first["lambda"] - plain["lambda"]) <= 2 * case[5], (first, plain)
        assert first == second, "the fused path run twice: the same iterations and the same bits"
