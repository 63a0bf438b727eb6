"""GPU tests (-m gpu) of csrc/blas1_extra.hip at kernel level: the rest of BLAS-1 (scal, xmy, axpbypcz, asum, amax), the fused
steps of Jacobi-cg, BiCGstab, cr and GMRES, and the CSR diagonal -- every one of the 34 entry points on real data.

Bars (references and the values of k: blas_extra_refs.py, checked on the CPU by test_blas_extra_refs.py):
  * output vectors: (a) BIT-EQUAL to the numpy restatement in type T (the library is built with -ffp-contract=off), and
    (b) within k * u * sum|terms| of the header's formula evaluated in longdouble (f64) / float64 (f32);
  * reduction results: within 1e-12 * sum|terms| of math.fsum over the products of the vectors the kernel returned
    (+ 2^-24 |exact| for cmi_blas_asum_f32, which rounds its result to float once); a host mirror equals the device scalar bit
    for bit; amax returns the exact value and the exact (first) position;
  * guard elements around every operand and every const operand are unchanged; the workspace holds NaNs before every call;
    the same call made twice gives the same bits.
Sizes: kBlock = 256, grid_for = 1024 elements per workgroup, capped at kMaxGrid = 1024 workgroups (reductions) or 4 x that
(element-wise kernels); the 16-byte `wide` forms need n a multiple of 2 (f64) / 4 (f32) and every pointer aligned."""
import functools
import math

import numpy as np
import pytest

import blas_extra_refs as R

pytestmark = pytest.mark.gpu

TYPES = {"f32": np.float32, "f64": np.float64}
PAD = 4            # guard elements on each side of a view: 16 (f32) / 32 (f64) bytes, so offset 0 stays 16-byte aligned
GUARD = -777.25
STEP = 1009        # operand j of a case is the shared pool from j * STEP on
BIG = 4_200_004
SMALL = (0, 1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 1028)
STRIDE = (262143, 262144, 262149)   # the first grid-stride trip of a scalar-path reduction (262144 = 1024 workgroups x 256 lanes)
CAP = (1_048_580,)                  # past the reduction cap on the wide f32 path, past the element-wise cap (4096 x 256) on the scalar path
LARGE = (4_200_003, BIG)            # aligned only; 4_200_004 / 4 > 4096 x 256: the grid-stride trip of the widened element-wise kernels
GROUPS = {"small": SMALL, "stride": STRIDE, "cap": CAP, "large": LARGE}
EXACT_AT = (5, 1028)                # the sizes that also run the exactly representable quotients

RESULTS = {"pcg_update": ("rz_new", "rr"), "bicg_s": ("ss",), "bicg_xr": ("rho_new", "rr"), "cr_xr": ("rr",), "cr_py": ("yy_new",), "axpy_dot": ("out",)}
MIRRORED = {"pcg_update": "rr", "bicg_s": "ss", "bicg_xr": "rr", "cr_xr": "rr"}


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
    """One seeded draw per type, shared (read-only) by every test."""
    a = np.random.default_rng(2024).standard_normal(BIG + 8 * STEP).astype(T)
    a.setflags(write=False)
    return a


def offsets(T, n):
    """All operands aligned, all offset by one element, for f32 also by two; the two largest sizes aligned only."""
    if n in LARGE:
        return (0,)
    return (0, 1, 2) if T is np.float32 else (0, 1)


class Operand:
    """A view of n elements into a larger device buffer, `off` elements past the 16-byte aligned position, guards on both sides."""

    def __init__(self, torch, T, values, off):
        self.n, self.lo = len(values), PAD + off
        self.before = np.full(self.lo + self.n + PAD, GUARD, T)
        self.before[self.lo:self.lo + self.n] = values
        self.buf = torch.from_numpy(self.before).cuda()
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[self.lo:self.lo + self.n]
        if self.n:
            assert (self.view.data_ptr() % 16 == 0) == (off * self.before.itemsize % 16 == 0)

    def restore(self, torch):
        self.buf.copy_(torch.from_numpy(self.before))

    def after(self):
        """The whole buffer as the kernel left it; the guards must be untouched."""
        a = self.buf.cpu().numpy()
        assert np.array_equal(a[:self.lo], self.before[:self.lo]) and np.array_equal(a[self.lo + self.n:], self.before[self.lo + self.n:]), "guard overwritten"
        return a

    def inner(self, a):
        return a[self.lo:self.lo + self.n]


def scalar(torch, value):
    return torch.tensor([value], dtype=torch.float64, device="cuda")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


# one adapter per entry-point family: (cmi, scalars (floats or device doubles), operand views, result tensors, workspace, mirror)
CALLS = {
    "scal": lambda cmi, s, o, res, ws, m: cmi.blas_scal(s["a"], o["x"]),                                              # cmi_blas_scal_f32 / _f64
    "xmy": lambda cmi, s, o, res, ws, m: cmi.blas_xmy(o["x"], o["y"], o["z"]),                                        # cmi_blas_xmy_f32 / _f64
    "axpbypcz": lambda cmi, s, o, res, ws, m: cmi.blas_axpbypcz(s["a"], o["x"], s["b"], o["y"], s["c"], o["z"], o["out"]),  # cmi_blas_axpbypcz_f32 / _f64
    "pcg_update": lambda cmi, s, o, res, ws, m: cmi.pcg_update_jacobi(s["rz"], s["yp"], o["y"], o["r"], o["dinv"], res["rz_new"], res["rr"], ws, mirror=m),  # cmi_pcg_update_jacobi_f32 / _f64
    "pcg_direction": lambda cmi, s, o, res, ws, m: cmi.pcg_direction_x_jacobi(s["rz_new"], s["rz_old"], s["yp"], o["r"], o["dinv"], o["p"], o["x"]),  # cmi_pcg_direction_x_jacobi_f32 / _f64
    "bicg_s": lambda cmi, s, o, res, ws, m: cmi.bicgstab_s(s["rho"], s["d1"], o["r"], o["AMp"], o["s"], res["ss"], ws, mirror=m),  # cmi_bicgstab_s_f32 / _f64
    "bicg_xr": lambda cmi, s, o, res, ws, m: cmi.bicgstab_xr(s["rho"], s["d1"], s["d2"], s["d3"], o["p"], o["s"], o["AMs"], o["r_star"], o["x"], o["r"],
                                                             res["rho_new"], res["rr"], ws, mirror=m),                  # cmi_bicgstab_xr_f32 / _f64
    "bicg_p": lambda cmi, s, o, res, ws, m: cmi.bicgstab_p(s["rho_new"], s["rho"], s["d1"], s["d2"], s["d3"], o["r"], o["AMp"], o["p"]),  # cmi_bicgstab_p_f32 / _f64
    "cr_xr": lambda cmi, s, o, res, ws, m: cmi.cr_xr(s["rz"], s["yy"], o["p"], o["y"], o["x"], o["r"], res["rr"], ws, mirror=m),  # cmi_cr_xr_f32 / _f64
    "cr_py": lambda cmi, s, o, res, ws, m: cmi.cr_py(s["rz_new"], s["rz"], o["r"], o["Ar"], o["p"], o["y"], res["yy_new"], ws),  # cmi_cr_py_f32 / _f64
    "axpy_dot": lambda cmi, s, o, res, ws, m: cmi.blas_axpy_dot(s["h"], o["v"], o["w"], o["u"], res["out"], ws),         # cmi_blas_axpy_dot_f32 / _f64
    "axpy_ratio": lambda cmi, s, o, res, ws, m: cmi.blas_axpy_ratio(s["num"], s["den"], o["x"], o["y"]),               # cmi_blas_axpy_ratio_f32 / _f64
}


def host_inputs(kernel, T, n):
    return {name: pool(T)[j * STEP:j * STEP + n] for j, name in enumerate(kernel.vecs)}


@functools.lru_cache(maxsize=2)
def references(name, T, n, kind):
    """(restatement in T, formula in the higher precision) of one case, computed once and shared by its alignment cases."""
    kernel = R.KERNELS[name]
    s, v = R.scalars_for(kernel, kind, T), host_inputs(kernel, T, n)
    want = kernel.restate(T, s, v)
    high = kernel.formula(*R.higher(T, s, v))
    for a in list(want.values()) + [x for pair in high.values() for x in pair]:
        a.setflags(write=False)
    return want, high


def check_vectors(kernel, T, got, want, high, what):
    for out in kernel.outputs:
        # (a) the kernel's own sequence of IEEE operations
        assert got[out].dtype == want[out].dtype and bits(got[out]) == bits(want[out]), \
            f"{what}: {out} differs from the restatement at {np.nonzero(got[out] != want[out])[0][:5]}"
        # (b) the header's formula in higher precision: k = kernel.k[out] roundings (table KERNELS in blas_extra_refs.py)
        value, terms = high[out]
        k = kernel.k[out]
        err = np.abs(got[out].astype(value.dtype) - value)
        assert np.all(err <= k * R.U[T] * terms), f"{what}: {out} outside {k} u sum|terms|, worst ratio {np.max(err / (R.U[T] * terms))}"


def check_sums(kernel, T, got, v, res, what):
    for rname, (a, b) in kernel.sums(T, got, v).items():
        exact, absolute = R.exact_sum(a, b)
        dev = float(res[rname])
        print(f"{what}: {rname} = {dev!r}, exact {exact!r}, |error| / sum|terms| = {abs(dev - exact) / absolute if absolute else 0.0:.3g}")
        assert abs(dev - exact) <= 1e-12 * absolute, f"{what}: {rname} = {dev!r}, exact {exact!r}"


def run_case(cmi, torch, ws, mirror, name, T, n, offs, kind="inexact"):
    """One call (made twice) of one kernel on views at the given element offsets (a dict per operand, or one int for all)."""
    kernel = R.KERNELS[name]
    what = f"{name} {np.dtype(T).name} n={n} offsets={offs} {kind}"
    if isinstance(offs, int):
        offs = {v: offs for v in kernel.vecs}
    s, v = R.scalars_for(kernel, kind, T), host_inputs(kernel, T, n)
    ops = {vn: Operand(torch, T, v[vn], offs[vn]) for vn in kernel.vecs}
    views = {vn: op.view for vn, op in ops.items()}
    sdev = s if kernel.by_value else {sn: scalar(torch, val) for sn, val in s.items()}
    m = mirror if name in MIRRORED else None
    runs = []
    for trip in range(2):
        if trip:
            for op in ops.values():
                op.restore(torch)
        else:
            ws.fill_(float("nan"))  # nothing in the workspace may need initialising; the second call finds the first one's leavings
        res = {rn: scalar(torch, float("nan")) for rn in RESULTS.get(name, ())}
        CALLS[name](cmi, sdev, views, res, ws, m)
        mirrored = m.wait() if m is not None else None
        after = {vn: op.after() for vn, op in ops.items()}
        for vn in kernel.const:
            assert bits(after[vn]) == bits(ops[vn].before), f"{what}: const operand {vn} changed"
        if m is not None:
            assert bits(np.float64(mirrored)) == bits(res[MIRRORED[name]].cpu().numpy()), f"{what}: host mirror differs from the device scalar"
        if not kernel.by_value:
            for sn, t in sdev.items():
                assert float(t) == s[sn], f"{what}: input scalar {sn} changed"
        runs.append((after, {rn: bits(t.cpu().numpy()) for rn, t in res.items()}))
        if trip == 0:
            got = {out: ops[out].inner(after[out]) for out in kernel.outputs}
            want, high = references(name, T, n, kind)
            check_vectors(kernel, T, got, want, high, what)
            check_sums(kernel, T, got, v, res, what)
    assert all(bits(runs[0][0][vn]) == bits(runs[1][0][vn]) for vn in kernel.vecs) and runs[0][1] == runs[1][1], f"{what}: the second call gave other bits"


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("tname", list(TYPES))
@pytest.mark.parametrize("name", list(CALLS))
def test_kernel_against_restatement_and_formula(cmi, torch_cuda, ws, name, tname, group):
    T = TYPES[tname]
    mirror = cmi.HostScalar()
    try:
        for n in GROUPS[group]:
            for off in offsets(T, n):
                run_case(cmi, torch_cuda, ws, mirror, name, T, n, off)
                if n in EXACT_AT:  # quotients that are representable: a failure of the inexact case alone is about the device's division
                    run_case(cmi, torch_cuda, ws, mirror, name, T, n, off, kind="exact")
    finally:
        mirror.close()


@pytest.mark.parametrize("tname", list(TYPES))
@pytest.mark.parametrize("name", list(CALLS))
def test_one_misaligned_operand_takes_the_scalar_path(cmi, torch_cuda, ws, name, tname):
    """n = 1028 (a multiple of both vector widths) with exactly one operand off the 16-byte grid, each operand in turn: a pointer
    missing from a can_widen list would send the 16-byte kernel over it."""
    T = TYPES[tname]
    kernel = R.KERNELS[name]
    mirror = cmi.HostScalar()
    try:
        for odd in kernel.vecs:
            run_case(cmi, torch_cuda, ws, mirror, name, T, 1028, {vn: int(vn == odd) for vn in kernel.vecs})
    finally:
        mirror.close()


@pytest.mark.parametrize("tname", list(TYPES))
def test_cr_xr_without_the_residual_update(cmi, torch_cuda, ws, tname):
    """cmi_cr_xr_* with update_r = 0: only x moves; r and *rr_dev are untouched."""
    T, torch = TYPES[tname], torch_cuda
    kernel = R.KERNELS["cr_xr"]
    for n in (0, 1, 5, 1025, 1028, 262149):
        for off in offsets(T, n):
            s, v = R.scalars_for(kernel, "inexact", T), host_inputs(kernel, T, n)
            ops = {vn: Operand(torch, T, v[vn], off) for vn in kernel.vecs}
            rr = scalar(torch, 12345.0)
            ws.fill_(float("nan"))
            cmi.cr_xr(scalar(torch, s["rz"]), scalar(torch, s["yy"]), ops["p"].view, ops["y"].view, ops["x"].view, ops["r"].view, rr, ws, update_r=False)
            after = {vn: op.after() for vn, op in ops.items()}
            for vn in ("p", "y", "r"):
                assert bits(after[vn]) == bits(ops[vn].before), (vn, n, off)
            assert float(rr) == 12345.0
            want, high = references("cr_xr", T, n, "inexact")
            got = ops["x"].inner(after["x"])
            assert bits(got) == bits(want["x"])
            assert np.all(np.abs(got.astype(high["x"][0].dtype) - high["x"][0]) <= 3 * R.U[T] * high["x"][1])  # k = 3: alpha -> T, alpha p, the add


@pytest.mark.parametrize("tname", list(TYPES))
def test_axpy_dot_forms(cmi, torch_cuda, ws, tname):
    """cmi_blas_axpy_dot_*: h_dev = NULL (the dot alone, w untouched, v unused), u == w (the norm's square of the updated w),
    and a vector length that leaves a tail behind the 16-byte part (run_case covers u != w)."""
    T, torch = TYPES[tname], torch_cuda
    kernel = R.KERNELS["axpy_dot"]
    for n in (0, 1, 3, 5, 1023, 1028, 262149, 1_048_580):
        for off in offsets(T, n):
            what = f"axpy_dot {tname} n={n} off={off}"
            s, v = R.scalars_for(kernel, "inexact", T), host_inputs(kernel, T, n)
            want, high = references("axpy_dot", T, n, "inexact")
            # the dot alone
            ops = {vn: Operand(torch, T, v[vn], off) for vn in ("w", "u")}
            out = scalar(torch, float("nan"))
            ws.fill_(float("nan"))
            cmi.blas_axpy_dot(None, None, ops["w"].view, ops["u"].view, out, ws)
            for vn, op in ops.items():
                assert bits(op.after()) == bits(op.before), f"{what}: {vn} changed by the dot alone"
            exact, absolute = R.exact_sum(v["w"], v["u"])
            assert abs(float(out) - exact) <= 1e-12 * absolute, what
            # u == w: the norm's square behind the axpy
            ops = {vn: Operand(torch, T, v[vn], off) for vn in ("v", "w")}
            ws.fill_(float("nan"))
            out.fill_(float("nan"))
            cmi.blas_axpy_dot(scalar(torch, s["h"]), ops["v"].view, ops["w"].view, ops["w"].view, out, ws)
            assert bits(ops["v"].after()) == bits(ops["v"].before)
            got = ops["w"].inner(ops["w"].after())
            assert bits(got) == bits(want["w"]), what
            assert np.all(np.abs(got.astype(high["w"][0].dtype) - high["w"][0]) <= 3 * R.U[T] * high["w"][1])  # k = 3: h -> T, h v, the subtraction
            exact, absolute = R.exact_sum(got, got)
            assert abs(float(out) - exact) <= 1e-12 * absolute, what
            # u == w without the axpy
            out.fill_(float("nan"))
            w = Operand(torch, T, v["w"], off)
            cmi.blas_axpy_dot(None, None, w.view, w.view, out, ws)
            assert bits(w.after()) == bits(w.before)
            exact, absolute = R.exact_sum(v["w"], v["w"])
            assert abs(float(out) - exact) <= 1e-12 * absolute, what


@pytest.mark.parametrize("tname", list(TYPES))
def test_xmy_in_place(cmi, torch_cuda, tname):
    """z aliasing x, and z aliasing y."""
    T, torch = TYPES[tname], torch_cuda
    for n in (1, 5, 1025, 262149, 1_048_580):
        for off in offsets(T, n):
            v = host_inputs(R.KERNELS["xmy"], T, n)
            want = v["x"] * v["y"]
            for alias in ("x", "y"):
                ops = {vn: Operand(torch, T, v[vn], off) for vn in ("x", "y")}
                cmi.blas_xmy(ops["x"].view, ops["y"].view, ops[alias].view)
                other = "y" if alias == "x" else "x"
                assert bits(ops[other].after()) == bits(ops[other].before)
                assert bits(ops[alias].inner(ops[alias].after())) == bits(want), (n, off, alias)


# ---- asum / amax ------------------------------------------------------------------------------------------------------------------
def asum_once(cmi, torch, ws, T, x, off):
    op = Operand(torch, T, x, off)
    res = torch.full((1,), float("nan"), dtype=op.buf.dtype, device="cuda")
    ws.fill_(float("nan"))
    cmi.blas_asum(op.view, res, ws)  # cmi_blas_asum_f32 / cmi_blas_asum_f64
    first = res.cpu().numpy().copy()
    res.fill_(float("nan"))
    cmi.blas_asum(op.view, res, ws)
    assert bits(first) == bits(res.cpu().numpy()) and bits(op.after()) == bits(op.before)
    return float(first[0])


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("tname", list(TYPES))
def test_asum(cmi, torch_cuda, ws, tname, group):
    T = TYPES[tname]
    for n in GROUPS[group]:
        x = pool(T)[:n]
        exact = math.fsum(np.abs(x.astype(np.float64)).tolist())  # every term is its own absolute value: sum|terms| = exact
        for off in offsets(T, n):
            got = asum_once(cmi, torch_cuda, ws, T, x, off)
            tol = 1e-12 * exact + (2.0 ** -24 * exact if T is np.float32 else 0.0)  # cmi_blas_asum_f32 rounds its double sum to float once
            print(f"asum {tname} n={n} off={off}: {got!r}, exact {exact!r}")
            assert abs(got - exact) <= tol and (n > 0 or got == 0.0), (n, off, got, exact)


def amax_once(cmi, torch, ws, T, x, off=0, want_value=True, want_index=True):
    op = Operand(torch, T, x, off)
    value = torch.full((1,), float("nan"), dtype=op.buf.dtype, device="cuda") if want_value else None
    index = torch.full((1,), -1, dtype=torch.int64, device="cuda") if want_index else None
    out = []
    for _ in range(2):
        ws.fill_(float("nan"))
        cmi.blas_amax(op.view, value, index, ws)  # cmi_blas_amax_f32 / cmi_blas_amax_f64
        out.append((None if value is None else float(value), None if index is None else int(index)))
    assert bits(op.after()) == bits(op.before)
    assert out[0] == out[1] and (out[0][0] is None or math.copysign(1.0, out[0][0]) == 1.0), out
    return out[0]


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("tname", list(TYPES))
def test_amax_random(cmi, torch_cuda, ws, tname, group):
    T = TYPES[tname]
    for n in GROUPS[group]:
        x = pool(T)[:n]
        want = R.amax_ref_fast(x)
        for off in offsets(T, n):
            assert amax_once(cmi, torch_cuda, ws, T, x, off) == want, (n, off)


@pytest.mark.parametrize("tname", list(TYPES))
def test_amax_edges(cmi, torch_cuda, ws, tname):
    T, torch = TYPES[tname], torch_cuda
    nan, inf = float("nan"), float("inf")
    # n = 0: value 0 and index 0, with either output pointer NULL in turn
    empty = np.zeros(0, T)
    assert amax_once(cmi, torch, ws, T, empty) == (0.0, 0)
    assert amax_once(cmi, torch, ws, T, empty, want_index=False) == (0.0, None)
    assert amax_once(cmi, torch, ws, T, empty, want_value=False) == (None, 0)

    def vec(n, places):
        x = (pool(T)[:n] * T(0.125)).astype(T)  # |x| < 1 nearly everywhere; the planted values are >= 8
        for at, val in places.items():
            x[at] = val
        return x
    cases = [
        (vec(256, {10: 9.0, 20: -9.0}), (9.0, 10)),                     # a tie inside one workgroup
        (vec(256, {10: -9.0, 20: 9.0}), (9.0, 10)),                     # ... whichever sign comes first
        (vec(2048, {300: 9.0, 10: 9.0}), (9.0, 10)),                    # a tie across two workgroups (2: lanes 0-255 and 512-767 / the rest)
        (vec(2048, {1500: -9.0, 700: 9.0}), (9.0, 700)),
        # 262150 elements run on 257 workgroups (stride 65792): position 65797 belongs to workgroup 0, position 300 to workgroup 1
        (vec(262150, {300: 9.0, 65797: 9.0}), (9.0, 300)),              # the later position in the LOWER-numbered workgroup
        (vec(262150, {300: -9.0, 262149: 9.0}), (9.0, 300)),
        (vec(262150, {262149: 9.0}), (9.0, 262149)),                    # the last element
        # 1_048_580 elements: the grid is capped at 1024 workgroups (stride 262144): 300 -> workgroup 1, 262149 -> workgroup 0
        (vec(1_048_580, {300: 9.0, 262149: -9.0, 1_048_579: 9.0}), (9.0, 300)),
        (vec(1025, {77: -8.5}), (8.5, 77)),                             # a negative value of largest magnitude
        (np.full(1025, -0.0, T), (0.0, 0)),                             # -0.0: the value is |x| = +0.0
        (vec(1025, {3: inf}), (inf, 3)),
        (vec(1025, {900: -inf, 1000: inf}), (inf, 900)),
        (vec(1025, {0: nan, 5: nan, 77: 8.5, 1024: nan}), (8.5, 77)),   # NaNs are skipped
        (vec(5, {0: nan, 1: nan, 2: nan, 3: nan, 4: 8.0}), (8.0, 4)),
        (np.full(1025, nan, T), (0.0, 0)),                              # all NaN: (0, 0), as the kernel's comment says
        (np.full(3, nan, T), (0.0, 0)),
    ]
    for x, want in cases:
        assert R.amax_ref_fast(x) == want
        for off in (0, 1):
            assert amax_once(cmi, torch, ws, T, x, off) == want, (len(x), want, off)
        assert amax_once(cmi, torch, ws, T, x, want_index=False) == (want[0], None)
        assert amax_once(cmi, torch, ws, T, x, want_value=False) == (None, want[1])


def test_reductions_of_nothing_write_zero(cmi, torch_cuda, ws):
    """n = 0: every reduction result (and its mirror) is 0, whatever it held before; covered per kernel by run_case at n = 0, and here for asum."""
    for T in TYPES.values():
        assert asum_once(cmi, torch_cuda, ws, T, np.zeros(0, T), 0) == 0.0


# ---- the CSR diagonal ---------------------------------------------------------------------------------------------------------------
def diagonal_once(cmi, torch, T, rows, Ap, Aj, Ax, reciprocal):
    dAp, dAj, dAx = (torch.from_numpy(np.array(a)).cuda() for a in (Ap, Aj, Ax))
    diag = Operand(torch, T, np.full(rows, 55.0, T), 0)
    cmi.csr_diagonal(rows, dAp, dAj, dAx, diag.view, reciprocal=reciprocal)  # cmi_csr_diagonal_f32 / cmi_csr_diagonal_f64
    assert np.array_equal(dAp.cpu().numpy(), Ap) and np.array_equal(dAj.cpu().numpy(), Aj) and bits(dAx.cpu().numpy()) == bits(Ax)
    return diag.inner(diag.after())


@pytest.mark.parametrize("reciprocal", [0, 1])
@pytest.mark.parametrize("tname", list(TYPES))
def test_csr_diagonal(cmi, torch_cuda, tname, reciprocal):
    """Against the numpy loop: empty rows, rows without a diagonal entry (0, or inf for the reciprocal), the entry stored twice (summed
    in storage order), first / in the middle / last in its row, unsorted columns, rows > columns and rows < columns."""
    T, torch = TYPES[tname], torch_cuda
    rows, Ap, Aj, Ax = R.hand_made_matrix(T)  # 6 x 4
    cases = [(rows, Ap, Aj, Ax), (3, Ap[:4], Aj, Ax)]  # ... and its first 3 rows: 3 x 4
    rng = np.random.default_rng(9)
    for nrows, ncols in ((700, 90), (90, 700), (1500, 1500)):
        lens = rng.integers(0, 7, nrows)
        rAp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        rAj = rng.integers(0, ncols, int(rAp[-1])).astype(np.int32)  # unsorted, repeated columns
        near = rng.random(len(rAj)) < 0.4                             # pull entries onto the diagonal where the row has a column of its own
        row = np.repeat(np.arange(nrows), lens)
        rAj[near & (row < ncols)] = row[near & (row < ncols)]
        cases.append((nrows, rAp, rAj, rng.standard_normal(len(rAj)).astype(T)))
    for nrows, cAp, cAj, cAx in cases:
        want = R.csr_diagonal_ref(T, nrows, cAp, cAj, cAx, reciprocal)
        assert bits(diagonal_once(cmi, torch, T, nrows, cAp, cAj, cAx, reciprocal)) == bits(want), nrows
    if not reciprocal:
        assert want.tolist().count(0.0) > 10  # the random matrices do have rows without a diagonal entry


@pytest.mark.parametrize("rows", [1, 1025, 1_048_577])
@pytest.mark.parametrize("tname", list(TYPES))
def test_csr_diagonal_one_entry_per_row(cmi, torch_cuda, tname, rows):
    """One entry per row, every 7th one beside the diagonal; 1_048_577 rows: past the element-wise cap of 4096 workgroups."""
    T = TYPES[tname]
    Ap = np.arange(rows + 1, dtype=np.int32)
    i = np.arange(rows, dtype=np.int64)
    Aj = np.where((i % 7 == 3) & (rows > 1), (i + 1) % rows, i).astype(np.int32)
    Ax = pool(T)[:rows]
    for reciprocal in (0, 1):
        want = R.csr_diagonal_ref_fast(T, rows, Ap, Aj, Ax, reciprocal)
        if rows <= 1025:
            assert bits(want) == bits(R.csr_diagonal_ref(T, rows, Ap, Aj, Ax, reciprocal))
        assert bits(diagonal_once(cmi, torch_cuda, T, rows, Ap, Aj, Ax, reciprocal)) == bits(want)
