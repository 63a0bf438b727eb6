"""GPU tests (-m gpu) of the multi-shift kernels of csrc/krylov_m.hip through binding.py, of cmi.krylov.cg_m, and of the header layer on
device_memory (tests/multishift/test_multishift_device.cpp), in the manner of tests/test_blas_extra_gpu.py.

Bars for every kernel test: the outputs are BIT-EQUAL to the numpy restatements of tests/multishift_refs.py (the library is built with
-ffp-contract=off, its float division is correctly rounded; the restatements are checked on the CPU by tests/test_multishift_refs.py);
guard elements round every operand and every const operand are unchanged; write-only outputs hold NaNs before the call; the same call
made twice on the same inputs gives the same bits.  For the shifted vectors "bit-equal" covers the whole buffer: the ld - n elements
between two shifts stay as they were.

Sizes.  kBlasBlock = 256 lanes, a lane owns one 16-byte piece (2 doubles / 4 floats), kShiftUnroll = 4 shifts are in flight together (so
num_shifts = 1, 3 run the remainder loop only and 8 the unrolled one; the C++ cases with 4 shifts cover one full trip), the grid is
fused_grid: one-shot up to kFusedMaxGrid = 65536 workgroups.  GRID_CAP_N is the first float size past that cap."""
import os
import subprocess

import numpy as np
import pytest

import multishift_refs as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

TYPES = {"f32": np.float32, "f64": np.float64}
PAD = 4            # guard elements on each side of a view: 16 (f32) / 32 (f64) bytes, so offset 0 stays 16-byte aligned
GUARD = -777.25
K_BLAS_BLOCK = 256          # csrc/blas1_shared.h kBlasBlock
K_FUSED_MAX_GRID = 1 << 16  # csrc/blas1_shared.h kFusedMaxGrid
GRID_CAP_N = K_FUSED_MAX_GRID * K_BLAS_BLOCK * 4 + 5   # float: 4 elements per lane; + 5: a second trip for the first lanes and a ragged last piece
XP_N = (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 1028)
XS_N = (1, 5, 256, 257, 1028)
SHIFT_COUNTS = (1, 2, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch


class Operand:
    """A view of n elements into a larger device buffer, `off` elements past the 16-byte aligned position, guards on both sides."""

    def __init__(self, torch, T, values, off=0):
        self.n, self.lo = len(values), PAD + off
        self.before = np.full(self.lo + self.n + PAD, GUARD, T)
        self.before[self.lo:self.lo + self.n] = values
        self.buf = torch.from_numpy(self.before).cuda()
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[self.lo:self.lo + self.n]

    def restore(self, torch):
        self.buf.copy_(torch.from_numpy(self.before))

    def after(self):
        """The inner elements as the kernel left them; the guards must be untouched."""
        a = self.buf.cpu().numpy()
        assert bits(a[:self.lo]) == bits(self.before[:self.lo]) and bits(a[self.lo + self.n:]) == bits(self.before[self.lo + self.n:]), "guard overwritten"
        return a[self.lo:self.lo + self.n]

    def unchanged(self):
        return bits(self.after()) == bits(self.before[self.lo:self.lo + self.n])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def scalar(torch, value):
    return torch.tensor([value], dtype=torch.float64, device="cuda")


def run_twice(torch, call, operands, outputs, wants):
    """Run, compare every output with its reference bit for bit, check the const operands; restore everything and run again: same bits."""
    got = []
    for rep in range(2):
        for o in operands.values():
            o.restore(torch)
        call()
        torch.cuda.synchronize()
        got.append({k: bits(operands[k].after()) for k in outputs})
        for k, o in operands.items():
            if k not in outputs:
                assert o.unchanged(), f"const operand {k} changed"
    for k in outputs:
        assert got[0][k] == bits(wants[k]), f"{k} differs from the restatement"
        assert got[0][k] == got[1][k], f"{k}: two identical calls differ"


# ---- cmi_cg_m_coefficients_* --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", list(TYPES))
@pytest.mark.parametrize("ns", SHIFT_COUNTS)
def test_cg_m_coefficients(cmi, torch_cuda, tname, ns):
    """The first-iteration call (state (1, 0), every zeta 1) and a second call on what the first one left: state and rotation."""
    torch, T = torch_cuda, TYPES[tname]
    rng = np.random.default_rng(100 + ns)
    sigma = rng.uniform(0.05, 5.0, ns).astype(T)
    state, zm1, z0 = np.array([1, 0], T), np.ones(ns, T), np.ones(ns, T)
    nan = np.full(ns, np.nan, T)
    for rsq_old, pAp, rsq_new in ((100.0, 371.5, 31.25), (31.25, 80.75, 7.0625)):
        op = {"state": Operand(torch, T, state), "sigma": Operand(torch, T, sigma), "zeta_m1": Operand(torch, T, zm1), "zeta_0": Operand(torch, T, z0),
              "beta_s": Operand(torch, T, nan), "alpha_s": Operand(torch, T, nan)}
        d = [scalar(torch, v) for v in (rsq_old, pAp, rsq_new)]
        state, zm1, z0, beta_s, alpha_s = R.cg_m_coefficients(T, rsq_old, pAp, rsq_new, state, sigma, zm1, z0)
        wants = {"state": state, "zeta_m1": zm1, "zeta_0": z0, "beta_s": beta_s, "alpha_s": alpha_s}
        run_twice(torch, lambda: cmi.cg_m_coefficients(d[0], d[1], d[2], *(op[k].view for k in ("state", "sigma", "zeta_m1", "zeta_0", "beta_s", "alpha_s"))),
                  op, tuple(wants), wants)
        assert [float(v.item()) for v in d] == [rsq_old, pAp, rsq_new]
        assert np.isfinite(alpha_s).all() and np.isfinite(beta_s).all()


@pytest.mark.parametrize("tname", list(TYPES))
def test_cg_m_coefficients_clamp_and_no_shift(cmi, torch_cuda, tname):
    """A zeta that falls below 1e-30 is set to 1e-18 behind beta_s; num_shifts = 0 only stores the state."""
    torch, T = torch_cuda, TYPES[tname]
    sigma, zm1, z0 = np.array([0, 0.5], T), np.ones(2, T), np.array([2.0 ** -110, 1], T)
    state = np.array([1, 0], T)
    op = {"state": Operand(torch, T, state), "sigma": Operand(torch, T, sigma), "zeta_m1": Operand(torch, T, zm1), "zeta_0": Operand(torch, T, z0),
          "beta_s": Operand(torch, T, np.full(2, np.nan, T)), "alpha_s": Operand(torch, T, np.full(2, np.nan, T))}
    d = [scalar(torch, v) for v in (1.0, 1.0, 0.5)]
    w = R.cg_m_coefficients(T, 1.0, 1.0, 0.5, state, sigma, zm1, z0)
    wants = dict(zip(("state", "zeta_m1", "zeta_0", "beta_s", "alpha_s"), w))
    assert wants["zeta_0"][0] == T(1e-18) and wants["beta_s"][0] == T(-1)
    run_twice(torch, lambda: cmi.cg_m_coefficients(d[0], d[1], d[2], *(op[k].view for k in ("state", "sigma", "zeta_m1", "zeta_0", "beta_s", "alpha_s"))),
              op, tuple(wants), wants)
    st = Operand(torch, T, state)
    empty = torch.empty(0, dtype=st.view.dtype, device="cuda")
    cmi.cg_m_coefficients(d[0], d[1], d[2], st.view, empty, empty, empty, empty, empty)
    torch.cuda.synchronize()
    assert bits(st.after()) == bits(np.array([-1, 0.5], T))


# ---- cmi_cg_m_update_xp_* ------------------------------------------------------------------------------------------------
def xp_case(cmi, torch, T, n, ns, ld, off, with_p0, rng):
    size = (ns - 1) * ld + n
    state = rng.standard_normal(2).astype(T)
    coef = {k: rng.standard_normal(ns).astype(T) for k in ("beta_s", "alpha_s", "zeta_0")}
    r, p0 = rng.standard_normal(n).astype(T), rng.standard_normal(n).astype(T)
    x, ps = rng.standard_normal(size).astype(T), rng.standard_normal(size).astype(T)
    op = {"state": Operand(torch, T, state), **{k: Operand(torch, T, v) for k, v in coef.items()}, "r": Operand(torch, T, r, off), "x": Operand(torch, T, x, off),
          "p_s": Operand(torch, T, ps, off)}
    if with_p0:
        op["p0"] = Operand(torch, T, p0, off)
    wp0, wx, wps = R.cg_m_update_xp(T, n, ns, ld, state, coef["beta_s"], coef["alpha_s"], coef["zeta_0"], r, p0 if with_p0 else None, x, ps)
    wants = {"x": wx, "p_s": wps, **({"p0": wp0} if with_p0 else {})}
    run_twice(torch, lambda: cmi.cg_m_update_xp(n, ld, op["state"].view, op["beta_s"].view, op["alpha_s"].view, op["zeta_0"].view, op["r"].view,
                                                op["p0"].view if with_p0 else None, op["x"].view, op["p_s"].view), op, tuple(wants), wants)


@pytest.mark.parametrize("tname", list(TYPES))
@pytest.mark.parametrize("ns", [1, 3, 8])
def test_cg_m_update_xp(cmi, torch_cuda, tname, ns):
    """Every n x ld x alignment: whole buffers bit-equal, the gaps between the shifts included.  ld = n + 1 and n + 5 break the 16-byte
    alignment from one shift to the next (f64: every other shift; f32: three of four)."""
    torch, T = torch_cuda, TYPES[tname]
    rng = np.random.default_rng(7 * ns)
    for n in XP_N:
        for ld in (n, n + 1, n + 5):
            for off in (0, 1):
                xp_case(cmi, torch, T, n, ns, ld, off, True, rng)


@pytest.mark.parametrize("tname", list(TYPES))
def test_cg_m_update_xp_without_p0_and_without_shifts(cmi, torch_cuda, tname):
    torch, T = torch_cuda, TYPES[tname]
    rng = np.random.default_rng(5)
    for n, ns, ld, off in ((5, 3, 6, 1), (257, 8, 257, 0), (1028, 3, 1033, 1)):
        xp_case(cmi, torch, T, n, ns, ld, off, False, rng)
    # num_shifts = 0: only p0 <- r + alpha_0 p0
    n = 1025
    state, r, p0 = rng.standard_normal(2).astype(T), rng.standard_normal(n).astype(T), rng.standard_normal(n).astype(T)
    op = {"state": Operand(torch, T, state), "r": Operand(torch, T, r, 1), "p0": Operand(torch, T, p0)}
    empty = torch.empty(0, dtype=op["r"].view.dtype, device="cuda")
    want = (r + state[1] * p0).astype(T)
    run_twice(torch, lambda: cmi.cg_m_update_xp(n, n, op["state"].view, empty, empty, empty, op["r"].view, op["p0"].view, empty, empty), op, ("p0",), {"p0": want})


def test_cg_m_update_xp_past_the_grid_cap(cmi, torch_cuda):
    """n = GRID_CAP_N floats: kFusedMaxGrid workgroups of kBlasBlock lanes cover the first GRID_CAP_N - 5 elements in one trip, the first two
    lanes of the grid make a second one (a full piece and a ragged one).  num_shifts = 2, ld = n + 2 (shift 1 unaligned).  The reference is
    formed on the device by torch, one rounding per operation (a product and a sum or difference are separate kernels): the same bits."""
    torch = torch_cuda
    n, ns = GRID_CAP_N, 2
    ld = n + 2
    assert n > K_FUSED_MAX_GRID * K_BLAS_BLOCK * 4 and ld % 4 != 0
    g = torch.Generator(device="cuda").manual_seed(11)
    size = (ns - 1) * ld + n
    buf = {k: torch.full((2 * PAD + m,), GUARD, dtype=torch.float32, device="cuda") for k, m in (("r", n), ("p0", n), ("x", size), ("p_s", size))}
    v = {k: b[PAD:b.numel() - PAD] for k, b in buf.items()}
    for t in v.values():
        t.copy_(torch.randn(t.numel(), generator=g, device="cuda", dtype=torch.float32))
    state = torch.tensor([0.75, -0.375], dtype=torch.float32, device="cuda")
    beta_s, alpha_s, zeta = (torch.tensor(c, dtype=torch.float32, device="cuda") for c in ([0.3, -1.7], [0.9, 0.11], [1.3, -0.6]))
    want_p0 = v["r"] + state[1] * v["p0"]
    want_x, want_ps = v["x"].clone(), v["p_s"].clone()
    for s in range(ns):
        sl = slice(s * ld, s * ld + n)
        old = v["p_s"][sl]
        want_x[sl] = v["x"][sl] - beta_s[s] * old
        want_ps[sl] = zeta[s] * v["r"] + alpha_s[s] * old
    r_before = v["r"].clone()
    cmi.cg_m_update_xp(n, ld, state, beta_s, alpha_s, zeta, v["r"], v["p0"], v["x"], v["p_s"])
    torch.cuda.synchronize()
    as_int = lambda t: t.view(torch.int32)
    assert torch.equal(as_int(v["p0"]), as_int(want_p0)) and torch.equal(as_int(v["x"]), as_int(want_x)) and torch.equal(as_int(v["p_s"]), as_int(want_ps))
    assert torch.equal(as_int(v["r"]), as_int(r_before))
    for b in buf.values():
        assert bool((b[:PAD] == GUARD).all()) and bool((b[-PAD:] == GUARD).all())


# ---- cmi_bicgstab_m_* ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", list(TYPES))
def test_bicgstab_m_s(cmi, torch_cuda, tname):
    torch, T = torch_cuda, TYPES[tname]
    rng = np.random.default_rng(21)
    for n in XS_N:
        for off in (0, 1):
            alpha_1, chi_0 = T(rng.standard_normal()), T(rng.standard_normal())
            v = {k: rng.standard_normal(n).astype(T) for k in ("r_1", "As", "s_0")}
            op = {k: Operand(torch, T, a, off) for k, a in v.items()}
            want = R.bicgstab_m_s(T, alpha_1, chi_0, v["r_1"], v["As"], v["s_0"])
            run_twice(torch, lambda: cmi.bicgstab_m_s(float(alpha_1), float(chi_0), op["r_1"].view, op["As"].view, op["s_0"].view), op, ("s_0",), {"s_0": want})


@pytest.mark.parametrize("tname", list(TYPES))
@pytest.mark.parametrize("ns", [1, 3, 257])
def test_bicgstab_m_coefficients(cmi, torch_cuda, tname, ns):
    torch, T = torch_cuda, TYPES[tname]
    rng = np.random.default_rng(31 + ns)
    sigma = rng.uniform(0.05, 5.0, ns).astype(T)
    zm1, z0, rho0 = rng.uniform(0.5, 1.0, ns).astype(T), rng.uniform(0.1, 0.5, ns).astype(T), rng.uniform(0.1, 1.0, ns).astype(T)
    if ns > 1:
        zm1[1], z0[1], sigma[1] = 1, 2.0 ** -110, 0     # trips the clamp (beta_m1 zeta_m1 / (beta_m1 zeta_m1) = 1, alpha_old = 0 below would too)
    sc = [T(v) for v in (-0.4375, -0.28125, 0.0 if ns == 3 else 0.6875, 0.53125, 0.71875)]
    names = ("sigma", "zeta_m1", "zeta_0", "rho_0", "zeta_1", "beta_s", "chi_s", "rho_1", "alpha_s")
    op = {"sigma": Operand(torch, T, sigma), "zeta_m1": Operand(torch, T, zm1), "zeta_0": Operand(torch, T, z0), "rho_0": Operand(torch, T, rho0),
          **{k: Operand(torch, T, np.full(ns, np.nan, T)) for k in names[4:]}}
    wants = dict(zip(names[4:], R.bicgstab_m_coefficients(T, *sc, sigma, zm1, z0, rho0)))
    if ns == 3:
        assert wants["zeta_1"][1] == T(1e-18)
    run_twice(torch, lambda: cmi.bicgstab_m_coefficients(*(float(v) for v in sc), *(op[k].view for k in names)), op, names[4:], wants)


@pytest.mark.parametrize("tname", list(TYPES))
@pytest.mark.parametrize("ns", [1, 3])
def test_bicgstab_m_update_xs(cmi, torch_cuda, tname, ns):
    """x_s and s_s bit-equal over the whole buffers (gaps included), and the rotation of zeta and rho behind the update."""
    torch, T = torch_cuda, TYPES[tname]
    rng = np.random.default_rng(41 + ns)
    coef_names = ("beta_s", "chi_s", "rho_0", "zeta_m1", "zeta_0", "alpha_s", "rho_1", "zeta_1")
    for n in XS_N:
        for ld in (n, n + 1):
            for off in (0, 1):
                size = (ns - 1) * ld + n
                c = {k: rng.uniform(0.25, 1.5, ns).astype(T) * T(rng.choice([-1, 1])) for k in coef_names}
                v = {k: rng.standard_normal(n).astype(T) for k in ("r_0", "r_1", "w_1")}
                x, ss = rng.standard_normal(size).astype(T), rng.standard_normal(size).astype(T)
                op = {**{k: Operand(torch, T, a) for k, a in c.items()}, **{k: Operand(torch, T, a, off) for k, a in v.items()}, "x": Operand(torch, T, x, off),
                      "s_s": Operand(torch, T, ss, off)}
                wx, wss, wzm1, wz0, wrho0 = R.bicgstab_m_update_xs(T, n, ns, ld, c["beta_s"], c["chi_s"], c["rho_0"], c["zeta_m1"], c["zeta_0"], c["alpha_s"],
                                                                   c["rho_1"], c["zeta_1"], v["r_0"], v["r_1"], v["w_1"], x, ss)
                wants = {"x": wx, "s_s": wss, "zeta_m1": wzm1, "zeta_0": wz0, "rho_0": wrho0}
                run_twice(torch, lambda: cmi.bicgstab_m_update_xs(n, ld, *(op[k].view for k in coef_names), op["r_0"].view, op["r_1"].view, op["w_1"].view,
                                                                  op["x"].view, op["s_s"].view), op, tuple(wants), wants)


# ---- cmi.krylov.cg_m --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", ["fused", "CMI_CG_M_FUSED=0"])
@pytest.mark.parametrize("fmt", ["csr", "ell"])
@pytest.mark.parametrize("tname,nx,ny", [("f32", 10, 10), ("f32", 7, 5), ("f64", 10, 10), ("f64", 7, 5), ("f64", 33, 31)])
def test_python_cg_m(cmi, torch_cuda, monkeypatch, tname, nx, ny, fmt, fused):
    """The multi_mass.cu case through cmi.krylov.cg_m: every shift's true residual below 100 x the monitor's tolerance x ||b||, the monitor
    converged; the fused iteration and the operation-by-operation one ($CMI_CG_M_FUSED=0).  CSR multiplies through its plan."""
    torch, T = torch_cuda, TYPES[tname]
    tol = 1e-6 if T is np.float32 else 1e-10
    monkeypatch.setenv("CMI_CG_M_FUSED", "0" if fused != "fused" else "1")
    dt = torch.float32 if T is np.float32 else torch.float64
    A = cmi.poisson5pt(nx, ny, fmt, dtype=dt)
    if fmt == "csr":
        assert A.plan() is not None
    n = nx * ny
    sigma = np.array([0.1, 0.5, 1.0, 5.0], T)
    b = torch.ones(n, dtype=dt, device="cuda")
    x = torch.full((n * 4,), 3.0, dtype=dt, device="cuda")   # zero-filled by the solver
    out, mon = cmi.krylov.cg_m(A, b, torch.from_numpy(sigma).cuda(), x=x, iteration_limit=100, relative_tolerance=tol)
    assert mon.converged() and 0 < mon.iteration_count < 100
    assert out.data_ptr() == x.data_ptr() and tuple(out.shape) == (4, n)
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    rel = R.relative_residuals(R.poisson5pt(nx, ny, T), got, np.ones(n, T), sigma)
    print(tname, nx, ny, fmt, fused, mon.iteration_count, rel)
    assert max(rel) < 100 * tol


# ---- the header layer -----------------------------------------------------------------------------------------------------
def test_multishift_cpp_device_layer(cmi, tmp_path):
    """tests/multishift/test_multishift_device.cpp: the host program's solver cases in device_memory, all five formats, both solvers."""
    import test_eigen_host as H
    import test_multishift_host as M
    exe = tmp_path / "test_multishift_device"
    r = subprocess.run(["g++", *H.CXXFLAGS, os.path.join(ROOT, "tests", "multishift", "test_multishift_device.cpp"), "-o", str(exe), *H.LDFLAGS],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert M.HOST_TESTS in r.stdout
