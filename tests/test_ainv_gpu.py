"""GPU tests (-m gpu) of the row scale a one-launch HYB plan carries (cmi_plan_set_row_scale) and of the AINV preconditioners on device_memory.

Through the binding: cmi_spmv_hyb_plan_* and cmi_spmv_hyb_dot_plan_* through a scaled plan against the numpy restatement below -- per row the
chain from +0 over the ELL slots in slot order and the row's COO entries in entry order, then ONE multiply by d[row], every operation rounded on its
own -- bit for bit; the refusals; the stream and capture contract with the checks of tests/test_stream_contract_gpu.py.
tests/ainv/test_ainv_device.cpp, built and run once: the classes on device_memory against host_memory and the reference's tests."""
import os
import subprocess

import numpy as np
import pytest

import stream_contract as SC
from test_stream_contract_gpu import check_a, check_b, ctx, filler, side, stop_after_a_device_fault, torch_cuda  # noqa: F401  (fixtures and the two checks)

pytestmark = pytest.mark.gpu

NOT_SUPPORTED, INVALID = 3, 1
TILE = 256


def hyb_problem(T, n, width, coo, seed=0, special=False):
    """A HYB matrix as the conversions lay it out: ELL arrays column-major with pitch (padding: column -1, value 0, at the rows' ends), COO part
    sorted by row.  coo: "empty" | "light" (some rows hold 1..3 entries, one holds 20) | "heavy" (one 256-row tile holds 600: three LDS chunks of
    256, the others few).  special: IEEE special values among the matrix values and x."""
    rng = np.random.default_rng([n, width, seed, len(coo)])
    pitch = (n + 31) // 32 * 32
    eAj = np.full((max(width, 1), pitch), -1, np.int32)
    eAx = np.zeros((max(width, 1), pitch), T)
    lens = rng.integers(0, width + 1, n) if width else np.zeros(n, np.int64)
    lens[rng.integers(0, n, max(1, n // 2))] = width  # most rows full
    for k in range(width):
        rows = np.flatnonzero(lens > k)
        eAj[k, rows] = rng.integers(0, n, len(rows))
        eAx[k, rows] = rng.standard_normal(len(rows)).astype(T)
    per_row = np.zeros(n, np.int64)
    if coo == "light":
        some = rng.choice(n, max(1, n // 5), replace=False)
        per_row[some] = rng.integers(1, 4, len(some))
        per_row[rng.integers(0, n)] = min(20, n * 3 - int(per_row.sum()) if n > 1 else 3)
    elif coo == "heavy":
        tile = (n - 1) // TILE // 2  # a middle tile (the only one for n <= 256)
        rows = np.arange(tile * TILE, min(n, tile * TILE + TILE))
        per_row[rows] = 600 // len(rows)
        per_row[rows[: 600 - int(per_row[rows].sum())]] += 1
        per_row[rng.choice(n, max(1, n // 50), replace=False)] += 1
    assert per_row.sum() <= 3 * n, "the COO part must stay light enough for one launch"
    cAi = np.repeat(np.arange(n), per_row).astype(np.int32)
    cAj = rng.integers(0, n, len(cAi)).astype(np.int32)
    cAx = rng.standard_normal(len(cAi)).astype(T)
    x = rng.standard_normal(n).astype(T)
    d = rng.uniform(0.5, 2.0, n).astype(T) * rng.choice([-1, 1], n).astype(T)
    if special:
        deck = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, np.finfo(T).tiny / 4, -np.finfo(T).tiny / 8, np.finfo(T).max, 1.0, -3.0], T)
        for a in (eAx.reshape(-1), cAx, x, d):
            if len(a):
                where = rng.choice(len(a), max(1, len(a) // 12), replace=False)
                a[where] = deck[rng.integers(0, len(deck), len(where))]
        eAx[eAj == -1] = 0
    if width == 0:
        eAj, eAx = eAj[:0], eAx[:0]
    return dict(n=n, width=width, pitch=pitch, eAj=eAj.reshape(-1), eAx=eAx.reshape(-1), cAi=cAi, cAj=cAj, cAx=cAx, x=x, d=d, per_row=per_row)


def chain(P, x, eAx=None, cAx=None):
    """the unscaled row sums: from +0, the ELL slots in slot order, then the row's COO entries in entry order; one rounding per operation"""
    T = x.dtype.type
    n, width, pitch = P["n"], P["width"], P["pitch"]
    eAx = P["eAx"] if eAx is None else eAx
    cAx = P["cAx"] if cAx is None else cAx
    acc = np.zeros(n, T)
    with np.errstate(all="ignore"):
        for k in range(width):
            col = P["eAj"][k * pitch:k * pitch + n]
            val = eAx[k * pitch:k * pitch + n]
            live = col != -1
            acc[live] = acc[live] + val[live] * x[np.where(live, col, 0)[live]]
        first = np.r_[0, np.cumsum(P["per_row"])]
        for r in range(int(P["per_row"].max()) if n else 0):
            rows = np.flatnonzero(P["per_row"] > r)
            e = first[rows] + r
            acc[rows] = acc[rows] + cAx[e] * x[P["cAj"][e]]
    return acc


def scaled(P, x=None, d=None, **kw):
    x = P["x"] if x is None else x
    with np.errstate(all="ignore"):
        return chain(P, x, **kw) * (P["d"] if d is None else d)


def same_bits_or_nan(got, want, what):
    """NaN positions equal (the payload of a NaN differs between numpy and the device), everything else by its bits, as special_values.same_bits"""
    from special_values import same_bits
    same_bits(got, want, what)


class Device:
    def __init__(self, cmi, torch, P):
        dev = torch.device("cuda")
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.P, self.cmi, self.torch = P, cmi, torch
        self.eAj, self.eAx, self.cAi, self.cAj, self.cAx = t(P["eAj"]), t(P["eAx"]), t(P["cAi"]), t(P["cAj"]), t(P["cAx"])
        self.x, self.d = t(P["x"]), t(P["d"])
        self.tdt = self.x.dtype
        self.plan = cmi.Plan.hyb(self.tdt, P["n"], P["n"], P["width"], self.cAi)
        self.y = torch.full((P["n"],), SC.SENTINEL, dtype=self.tdt, device=dev)

    def multiply(self, accumulate=False, x=None, stream=None):
        P = self.P
        self.cmi.spmv_hyb_plan(self.plan, P["pitch"], self.eAj, self.eAx, self.cAi, self.cAj, self.cAx, self.x if x is None else x, self.y, accumulate=accumulate, stream=stream)
        return self.y.cpu().numpy()


SHAPES = [(1, 0, "light"), (1, 3, "empty"), (255, 1, "light"), (256, 3, "heavy"), (256, 9, "empty"), (257, 9, "light"), (257, 0, "heavy"), (257, 0, "empty"),
          (5063, 9, "heavy"), (5063, 3, "light"), (5063, 1, "empty"), (5063, 0, "light")]


@pytest.mark.parametrize("T", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,width,coo", SHAPES)
def test_scaled_plan_multiply_equals_the_restatement_bit_for_bit(cmi, torch_cuda, T, n, width, coo):
    P = hyb_problem(T, n, width, coo)
    D = Device(cmi, torch_cuda, P)
    assert D.plan.hyb_launches() == 1
    plain = D.multiply()
    SC.same_bits(plain, chain(P, P["x"]), "the plain planned multiply")
    cmi.plan_set_row_scale(D.plan, D.d)
    got = D.multiply()
    SC.same_bits(got, scaled(P), "the scaled planned multiply")
    # ... which is the multiply followed by blas_xmy
    z = torch_cuda.empty_like(D.y)
    cmi.blas_xmy(torch_cuda.from_numpy(plain).cuda(), D.d, z)
    SC.same_bits(got, z.cpu().numpy(), "the scaled multiply against multiply + xmy")
    # d changed in place: the next multiply sees it, no new plan
    d2 = (P["d"] * T(-0.75) + T(0.125)).astype(T)
    D.d.copy_(torch_cuda.from_numpy(d2))
    SC.same_bits(D.multiply(), scaled(P, d=d2), "after changing d in place")
    # NULL clears the scale
    cmi.plan_set_row_scale(D.plan, None)
    SC.same_bits(D.multiply(), plain, "after clearing the scale")


@pytest.mark.parametrize("T", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,width,coo", [(257, 9, "light"), (5063, 3, "heavy"), (256, 0, "light"), (5063, 1, "empty")])
def test_scaled_plan_multiply_on_special_values(cmi, torch_cuda, T, n, width, coo):
    P = hyb_problem(T, n, width, coo, seed=5, special=True)
    want = scaled(P)
    assert np.isnan(want).any() and not np.isnan(want).all()
    D = Device(cmi, torch_cuda, P)
    cmi.plan_set_row_scale(D.plan, D.d)
    same_bits_or_nan(D.multiply(), want, "the scaled planned multiply on the special-value deck")


@pytest.mark.parametrize("T", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,width,coo", [(1, 3, "empty"), (257, 9, "light"), (5063, 3, "heavy"), (5063, 0, "light"), (5063, 9, "empty")])
def test_scaled_plan_multiply_with_the_fused_dot(cmi, torch_cuda, T, n, width, coo):
    torch = torch_cuda
    P = hyb_problem(T, n, width, coo, seed=2)
    D = Device(cmi, torch, P)
    cmi.plan_set_row_scale(D.plan, D.d)
    w_host = np.random.default_rng(n).standard_normal(n).astype(T)
    w, res, ws = torch.from_numpy(w_host).cuda(), torch.full((1,), SC.SENTINEL, dtype=torch.float64, device="cuda"), cmi.blas_workspace()
    args = cmi.binding.hyb_plan_args(D.plan, P["pitch"], D.eAj, D.eAx, D.cAi, D.cAj, D.cAx)
    cmi.binding.spmv_hyb_dot_plan_args(args, D.x, D.y, w, res, ws)
    y = D.y.cpu().numpy()
    SC.same_bits(y, scaled(P), "y of the scaled multiply with the fused dot")
    SC.sum_close(res[0], y, w_host, "<y, w> of the scaled y")


def test_refusals(cmi, torch_cuda):
    torch = torch_cuda
    T = np.float64
    P = hyb_problem(T, 257, 3, "light")
    D = Device(cmi, torch, P)
    cmi.plan_set_row_scale(D.plan, D.d)
    D.y.fill_(SC.SENTINEL)
    with pytest.raises(cmi.CmiError) as e:   # accumulate through a scaled plan: refused before any launch
        D.multiply(accumulate=True)
    assert e.value.status == INVALID
    torch.cuda.synchronize()
    assert bool((D.y == SC.SENTINEL).all())
    # a CSR plan
    Ap = torch.arange(0, 258, dtype=torch.int32, device="cuda")
    Aj = torch.arange(0, 257, dtype=torch.int32, device="cuda")
    csr = cmi.Plan.csr(torch.float64, 257, 257, Ap, Aj)
    with pytest.raises(cmi.CmiError) as e:
        cmi.plan_set_row_scale(csr, D.d)
    assert e.value.status == NOT_SUPPORTED
    coo = cmi.Plan(cmi.FORMAT_COO, torch.float64, 257, 257, int(D.cAi.numel()), D.cAi)
    with pytest.raises(cmi.CmiError) as e:
        cmi.plan_set_row_scale(coo, D.d)
    assert e.value.status == NOT_SUPPORTED
    # a HYB plan that runs two launches (the COO part in descending row order): refused, still usable, still unscaled
    o = slice(None, None, -1)
    rev = dict(P, cAi=P["cAi"][o].copy(), cAj=P["cAj"][o].copy(), cAx=P["cAx"][o].copy())
    R = Device(cmi, torch, rev)
    assert R.plan.hyb_launches() == 2
    with pytest.raises(cmi.CmiError) as e:
        cmi.plan_set_row_scale(R.plan, R.d)
    assert e.value.status == NOT_SUPPORTED
    import rounding_refs as RR
    got = R.multiply()
    Ap_, Aj_, Ax_ = as_csr(P)
    bad = RR.within_rounding_bound(got, *RR.exact_rows(Ap_, Aj_, Ax_, P["x"]), got.dtype)
    assert not bad, "the refused plan's multiply is not the plain product: " + RR.describe(bad)
    # a wrapper-level refusal: a scale of the wrong type
    with pytest.raises(ValueError):
        cmi.plan_set_row_scale(D.plan, D.d.float())


def as_csr(P):
    """the HYB matrix as CSR (any entry order inside a row), for the rounding-bound comparison of the two-launch multiply"""
    n, width, pitch = P["n"], P["width"], P["pitch"]
    rows, cols, vals = [], [], []
    for k in range(width):
        col = P["eAj"][k * pitch:k * pitch + n]
        live = np.flatnonzero(col != -1)
        rows.append(live); cols.append(col[live]); vals.append(P["eAx"][k * pitch:k * pitch + n][live])
    rows.append(P["cAi"]); cols.append(P["cAj"]); vals.append(P["cAx"])
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.argsort(rows, kind="stable")
    Ap = np.r_[0, np.cumsum(np.bincount(rows, minlength=n))].astype(np.int32)
    return Ap, cols[order].astype(np.int32), vals[order]


def scaled_case(ctx, T, dot):
    """One SC.Case of the scaled planned multiply: the structure stays in place (the plan was made from it), the values, x, d (and w) have two sets."""
    P0 = hyb_problem(T, 5063, 3, "light")
    c = SC.Case(ctx, "scaled plan" + (" with the dot" if dot else ""))
    # the second value set keeps the first's structure: new values, x and d only
    rng = np.random.default_rng(99)
    vals1 = [rng.standard_normal(len(P0[k])).astype(T) for k in ("eAx", "cAx", "x", "d")]
    vals1[0][P0["eAj"] == -1] = 0
    eAj, cAi, cAj = c.fixed(P0["eAj"]), c.fixed(P0["cAi"]), c.fixed(P0["cAj"])
    eAx, cAx, x, d = c.inp(P0["eAx"], vals1[0]), c.inp(P0["cAx"], vals1[1]), c.inp(P0["x"], vals1[2]), c.inp(P0["d"], vals1[3])
    plan = ctx.cmi.Plan.hyb(x.dtype, P0["n"], P0["n"], P0["width"], cAi)
    assert plan.hyb_launches() == 1
    ctx.cmi.plan_set_row_scale(plan, d)
    c.keep.append(plan)
    y = c.out(P0["n"], T)
    want = [scaled(P0), scaled(P0, x=vals1[2], d=vals1[3], eAx=vals1[0], cAx=vals1[1])]
    if not dot:
        c.call = lambda s: ctx.cmi.spmv_hyb_plan(plan, P0["pitch"], eAj, eAx, cAi, cAj, cAx, x, y, stream=s)
        c.check = lambda k, ret: SC.same_bits(y, want[k], f"scaled planned multiply (value set {k})")
        return c
    w_sets = ctx.vecs(T, P0["n"], "w")
    w, res = c.inp(*w_sets), c.out(1, np.float64)
    args = ctx.cmi.binding.hyb_plan_args(plan, P0["pitch"], eAj, eAx, cAi, cAj, cAx)
    c.call = lambda s: ctx.cmi.binding.spmv_hyb_dot_plan_args(args, x, y, w, res, ctx.ws, stream=s)

    def check(k, ret):
        SC.same_bits(y, want[k], f"scaled planned multiply with the dot (value set {k})")
        SC.sum_close(res[0], want[k], w_sets[k], f"<y, w> (value set {k})")
    c.check = check
    return c


@pytest.mark.parametrize("dot", [False, True], ids=["multiply", "multiply+dot"])
def test_scaled_multiply_is_ordered_on_a_side_stream_behind_filler_work(ctx, torch_cuda, side, filler, dot):
    c = scaled_case(ctx, np.float64, dot)
    try:
        check_a(c, SC.ASYNC, torch_cuda, side, filler, c.label)
    finally:
        c.close()


@pytest.mark.parametrize("dot", [False, True], ids=["multiply", "multiply+dot"])
def test_scaled_multiply_records_into_a_capture_and_replays_on_new_values(ctx, torch_cuda, side, dot):
    c = scaled_case(ctx, np.float32, dot)
    try:
        check_b(c, torch_cuda, side, c.label)
    finally:
        c.close()


def test_ainv_device_layer_program(cmi, torch_cuda, tmp_path):
    """tests/ainv/test_ainv_device.cpp, once, in a child process under its own time limit: the reference's three tests on device_memory in float and
    double, the factors and the apply (both routes) against host_memory bit for bit, cusp::multiply(M.w) untouched by the second plan, cg through the
    fused branch and with CMI_CG_FUSED_AINV=0, the four solves of the reference's example."""
    from conftest import ROOT
    inc, libd = os.path.join(ROOT, "cusp-autotuned_amd", "include"), os.path.join(ROOT, "cusp-autotuned_amd", "lib")
    exe = tmp_path / "test_ainv_device"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fopenmp", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off",
                        f"-I{inc}", f"-I{os.path.join(ROOT, 'tests', 'cpp')}", os.path.join(ROOT, "tests", "ainv", "test_ainv_device.cpp"),
                        "-o", str(exe), f"-L{libd}", "-lcusp_mi355x", f"-Wl,-rpath,{libd}", "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run(["timeout", "-k", "10", "300", str(exe)], capture_output=True, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "tests, 0 failed" in r.stdout
