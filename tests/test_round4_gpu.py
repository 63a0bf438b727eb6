"""Round-4 additions on an MI355X, through the C-ABI: the run-compressed column copy (CMI_CSR_STREAM_WAVER), its packed twin
(CMI_CSR_STREAM_PACKED), the unaligned fall-back of AUTO wave-tile plans, the plan-less wave-tile multiply."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch


def dev(a, torch):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_csr(rng, rows, cols, lens, run_mean):
    """CSR whose rows are made of runs of consecutive columns (geometric lengths of mean `run_mean`; run_mean <= 1: single columns),
    columns ascending inside a row, no duplicates; the last row ends in the LAST column (a piece of one entry there is the kernel's
    clamped x load)."""
    Ap = np.r_[0, np.cumsum(lens)].astype(np.int32)
    Aj = np.empty(int(Ap[-1]), np.int32)
    for r in range(rows):
        n = int(lens[r])
        if n == 0:
            continue
        out = []
        c = int(rng.integers(0, max(1, cols - 3 * n - 8)))
        while len(out) < n:
            L = 1 if run_mean <= 1 else int(min(rng.geometric(1.0 / run_mean), n - len(out)))
            L = max(1, min(L, n - len(out)))
            if c + L > cols:
                break
            out.extend(range(c, c + L))
            c += L + int(rng.integers(1, 6))  # a gap: the next run is a new piece
        while len(out) < n:                   # ran out of columns: fill from the row's front (still ascending, no duplicates)
            have = set(out)
            k = 0
            while k in have:
                k += 1
            out.append(k)
            out.sort()
        Aj[Ap[r]:Ap[r + 1]] = np.array(sorted(out), np.int32)
    if lens[-1] > 0:
        row = Aj[Ap[-2]:Ap[-1]]
        if cols - 1 not in row:
            row[-1] = cols - 1
    Ax = rng.standard_normal(len(Aj))
    return Ap, Aj, Ax


def pieces_of(Ap, Aj, cap=4):
    n = 0
    for r in range(len(Ap) - 1):
        ln, prev = 0, None
        for c in Aj[Ap[r]:Ap[r + 1]]:
            if ln == 0 or c != prev + 1 or ln == cap:
                n += 1
                ln = 0
            ln += 1
            prev = c
    return n


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("vectors", [0, 1, 2, 4])
def test_waver_kernel_bit_exact(cmi, torch_cuda, orc, vectors, packed, tag):
    """reference arithmetic: cusp/system/detail/sequential/multiply/csr_spmv.h:42-74.  Every row of every matrix must have the host
    loop's bits: FEM-like runs (3, 6, 9 ...), single columns only (every piece one entry: more pieces than the unrolled pass holds),
    empty rows and a stretch of 300 of them, the longest row the tile admits, an odd entry count (the arrays' last pair), a piece of
    one entry in the last column, accumulate, the fused <y, w>."""
    torch = torch_cuda
    dtype, tdt = (np.float64, torch.float64) if tag == "f64" else (np.float32, torch.float32)
    cases = [(1, 6000, 20, 72, 3.0), (2, 3000, 1, 100, 1.0), (3, 20000, 5, 28, 2.0), (4, 4099, 0, 40, 6.0), (5, 900, 60, 125, 4.0), (6, 5000, 1, 9, 1.5)]
    for seed, rows, lo, hi, run_mean in cases:
        rng = np.random.default_rng(1000 * seed + vectors)
        lens = rng.integers(lo, hi + 1, size=rows)
        lens[rows // 3:rows // 3 + 300] = 0
        lens[-1] = hi
        if int(lens.sum()) % 2 == 0:
            lens[0] += 1
        cols = rows + 700
        Ap, Aj, Ax = run_csr(rng, rows, cols, lens, run_mean)
        Ax = Ax.astype(dtype)
        nnz, longest = int(Ap[-1]), int(lens.max())
        v_rule = vectors if vectors else 4
        x = rng.standard_normal(cols).astype(dtype)
        y0 = rng.standard_normal(rows).astype(dtype)
        dAp, dAj, dAx, dx = dev(Ap, torch), dev(Aj, torch), dev(Ax, torch), dev(x, torch)
        kern = cmi.CSR_STREAM_PACKED if packed else cmi.CSR_STREAM_WAVER
        cfg = cmi.Config(kernel=kern, items_per_thread=vectors)
        make = (lambda: cmi.Plan.csr_values(rows, cols, dAp, dAj, dAx, cfg)) if packed else (lambda: cmi.Plan.csr(tdt, rows, cols, dAp, dAj, cfg))
        if 2 * (longest + 3) > 256 * v_rule:  # the longest row takes more than half a tile: refused, by name
            with pytest.raises(cmi.CmiError):
                make()
            continue
        plan = make()
        c = plan.config()
        assert (c.kernel, c.items_per_thread) == (kern, v_rule), (seed, c)
        assert plan.info()["storage_order_sums"] is True
        npieces = pieces_of(Ap, Aj)
        want_bytes = 4 * (npieces + 64) + 16 * (nnz // (256 * v_rule - longest - 3) + 2)
        assert plan.device_bytes() >= want_bytes, (plan.device_bytes(), want_bytes)  # (+ the packed tiles)
        want, want_acc = orc.spmv_csr(Ap, Aj, Ax, x), orc.spmv_csr(Ap, Aj, Ax, x, y0)
        y = torch.full((rows,), 9.0, dtype=tdt, device="cuda")
        cmi.spmv_csr_plan(plan, dAp, dAj, dAx, dx, y)
        assert np.array_equal(y.cpu().numpy(), want), (seed, vectors, packed, tag)
        y = dev(y0, torch)
        cmi.spmv_csr_plan(plan, dAp, dAj, dAx, dx, y, accumulate=True)
        assert np.array_equal(y.cpu().numpy(), want_acc), (seed, vectors, packed, tag, "accumulate")
        w = rng.standard_normal(rows).astype(dtype)
        res = torch.zeros(1, dtype=torch.float64, device="cuda")
        y = torch.zeros(rows, dtype=tdt, device="cuda")
        cmi.spmv_csr_dot(rows, cols, dAp, dAj, dAx, dx, y, dev(w, torch), res, cmi.blas_workspace(), plan=plan)
        assert np.array_equal(y.cpu().numpy(), want), (seed, vectors, packed, tag, "dot")
        ref64 = float(np.dot(want.astype(np.float64), w.astype(np.float64)))
        assert abs(res.item() - ref64) <= 1e-9 * float(np.dot(np.abs(want).astype(np.float64), np.abs(w).astype(np.float64))) + 1e-300
        # the plan's contract: the column indices must not change in place -- and cmi_plan_validate tells when they have
        assert plan.validate(dAp, dAj) is True
        if packed:
            assert plan.validate_values(dAx) is True
            dAx2 = dAx.clone()
            dAx2[nnz // 2] += 1.0
            assert plan.validate_values(dAx2) is False
        else:  # the VALUES are the caller's: refreshed in place they are seen by the next multiply
            dAx.mul_(2.0)
            cmi.spmv_csr_plan(plan, dAp, dAj, dAx, dx, y)
            assert np.array_equal(y.cpu().numpy(), orc.spmv_csr(Ap, Aj, (2.0 * Ax).astype(dtype), x)), (seed, "values refreshed in place")
            assert plan.validate_values(dAx) is True  # (nothing of them is kept)
        dAj2 = dAj.clone()
        dAj2[nnz // 2] = (int(Aj[nnz // 2]) + 1) % cols
        assert plan.validate(dAp, dAj2) is False


def test_waver_refusals(cmi, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(5)
    rows = cols = 5000
    Ap, Aj, Ax = run_csr(rng, rows, cols, np.full(rows, 12), 3.0)
    dAp, dAj, dAx = dev(Ap, torch), dev(Aj, torch), dev(Ax, torch)
    with pytest.raises(cmi.CmiError):   # without the columns
        cmi.Plan(cmi.FORMAT_CSR, torch.float64, rows, cols, len(Aj), dAp, cmi.Config(kernel=cmi.CSR_STREAM_WAVER))
    with pytest.raises(cmi.CmiError):   # packed without the values
        cmi.Plan.csr(torch.float64, rows, cols, dAp, dAj, cmi.Config(kernel=cmi.CSR_STREAM_PACKED))
    # (f32 is served since session 9 of round 4: one 16-byte x load per piece; AUTO: the same size / piece-length rule as f64 -- this matrix is too small)
    assert cmi.Plan.csr(torch.float32, rows, cols, dAp, dAj, cmi.Config(kernel=cmi.CSR_STREAM_WAVER)).config().kernel == cmi.CSR_STREAM_WAVER
    assert cmi.Plan.csr(torch.float32, rows, cols, dAp, dAj).config().kernel != cmi.CSR_STREAM_WAVER
    with pytest.raises(cmi.CmiError):   # plan-less
        y = torch.zeros(rows, dtype=torch.float64, device="cuda")
        cmi.spmv_csr(rows, cols, dAp, dAj, dAx, y.clone(), y, cfg=cmi.Config(kernel=cmi.CSR_STREAM_WAVER))
    plan = cmi.Plan.csr(torch.float64, rows, cols, dAp, dAj, cmi.Config(kernel=cmi.CSR_STREAM_WAVER))
    x = torch.zeros(cols + 1, dtype=torch.float64, device="cuda")
    y = torch.zeros(rows, dtype=torch.float64, device="cuda")
    pad = torch.zeros(len(Aj) + 1, dtype=torch.float64, device="cuda")
    pad[1:] = dAx
    with pytest.raises(cmi.CmiError):   # an ASKED-FOR kernel keeps its alignment requirement as a hard error
        cmi.spmv_csr_plan(plan, dAp, dAj, pad[1:], x[:cols], y)


def test_auto_plans_fall_back_on_unaligned_arrays(cmi, torch_cuda, orc):
    """an AUTO plan that chose a wave-tile kernel with 16-byte loads never saw Aj / Ax / x; offset views then run the table's
    row-tile kernel (any alignment) instead of failing -- as they did before those kernels existed.  Two matrices beyond the size rule of
    those kernels: FEM blocks (-> the run-compressed copy) and columns anywhere inside a band (-> wave tiles, with or without the x window)."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import suitesparse_like as ssl
    torch = torch_cuda
    rng = np.random.default_rng(11)
    mats = []
    Ap, Aj, Ax = ssl.ldoor_like(0.45)
    mats.append(("fem blocks", Ap, Aj, Ax, (cmi.CSR_STREAM_WAVER,)))
    rows = 800000
    lens = rng.integers(16, 33, size=rows)
    Ap = np.r_[0, np.cumsum(lens)].astype(np.int32)
    ri = np.repeat(np.arange(rows, dtype=np.int64), lens)
    Aj = np.clip(ri + rng.integers(-3000, 3001, size=len(ri)), 0, rows - 1).astype(np.int32)
    mats.append(("band", Ap, Aj, rng.standard_normal(len(Aj)), (cmi.CSR_STREAM_WAVEV, cmi.CSR_STREAM_WAVEX)))
    for label, Ap, Aj, Ax, kernels in mats:
        rows = cols = len(Ap) - 1
        nnz = len(Aj)
        x = rng.standard_normal(cols)
        want = orc.spmv_csr(Ap, Aj, Ax, x, omp=True)
        dAp = dev(Ap, torch)
        jpad = torch.zeros(nnz + 1, dtype=torch.int32, device="cuda"); jpad[1:] = dev(Aj, torch)
        vpad = torch.zeros(nnz + 1, dtype=torch.float64, device="cuda"); vpad[1:] = dev(Ax, torch)
        xpad = torch.zeros(cols + 1, dtype=torch.float64, device="cuda"); xpad[1:] = dev(x, torch)
        plan = cmi.Plan.csr(torch.float64, rows, cols, dAp, jpad[1:])
        assert plan.config().kernel in kernels, (label, plan.config())
        y = torch.full((rows,), 3.0, dtype=torch.float64, device="cuda")
        cmi.spmv_csr_plan(plan, dAp, jpad[1:], vpad[1:], xpad[1:], y)   # 4 / 8 bytes off a 16-byte boundary
        assert np.array_equal(y.cpu().numpy(), want), label
        y.fill_(3.0)
        cmi.spmv_csr_plan(plan, dAp, dev(Aj, torch), dev(Ax, torch), dev(x, torch), y)  # aligned: the plan's own kernel
        assert np.array_equal(y.cpu().numpy(), want), label


@pytest.mark.parametrize("name", ["ldoor", "nlpkkt120", "thermal2"])
def test_configs3_full_size_run_compressed(cmi, torch_cuda, orc, name):
    """BASELINE.json configs[3] at full size through the run-compressed copy and its packed twin: asked for
    explicitly, and what an AUTO plan made with the columns selects (WAVER where the pieces average 2.5+ entries: ldoor, nlpkkt120)."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import suitesparse_like as ssl
    torch = torch_cuda
    Ap, Aj, Ax, source = ssl.load(name, 1.0)
    rows = cols = len(Ap) - 1
    nnz = len(Aj)
    x = orc.fill_x(cols)
    want = orc.spmv_csr(Ap, Aj, Ax, x, omp=True)
    dAp, dAj, dAx, dx = dev(Ap, torch), dev(Aj, torch), dev(Ax, torch), dev(x, torch)
    y = torch.empty(rows, dtype=torch.float64, device="cuda")
    for v in (0, 2, 4) if name != "thermal2" else (0, 1, 2):
        for packed in (False, True):
            cfg = cmi.Config(kernel=cmi.CSR_STREAM_PACKED if packed else cmi.CSR_STREAM_WAVER, items_per_thread=v)
            plan = cmi.Plan.csr_values(rows, cols, dAp, dAj, dAx, cfg) if packed else cmi.Plan.csr(torch.float64, rows, cols, dAp, dAj, cfg)
            y.fill_(10.0)
            cmi.spmv_csr_plan(plan, dAp, dAj, dAx, dx, y)
            assert np.array_equal(y.cpu().numpy(), want), f"{name} ({source}) V={v} packed={packed}: not bit-identical to the host loop"
            print(f"{name}: V={v} packed={packed}: plan owns {plan.device_bytes() / 1e6:.1f} MB for {12 * nnz / 1e6:.1f} MB of index + value streams")
    auto = cmi.Plan.csr(torch.float64, rows, cols, dAp, dAj)
    k = auto.config().kernel
    print(f"{name}: AUTO plan made with the columns -> kernel {k}")
    if name in ("ldoor", "nlpkkt120") and source.startswith("seeded"):
        assert k == cmi.CSR_STREAM_WAVER, k
    elif source.startswith("seeded"):  # thermal2-like: f64 rows of ~7 entries whose columns share x lines -> wave tiles with V = 1 (round 4 rule)
        assert (k, auto.config().items_per_thread) == (cmi.CSR_STREAM_WAVEV, 1), auto.config()
    else:
        assert k != cmi.CSR_STREAM_PACKED
    y.fill_(10.0)
    cmi.spmv_csr_plan(auto, dAp, dAj, dAx, dx, y)
    assert np.array_equal(y.cpu().numpy(), want)
    A = cmi.CsrMatrix(rows, cols, nnz, dAp, dAj, dAx)   # the containers' own path: plan made (with the columns) at the first multiply
    y.fill_(10.0)
    cmi.multiply(A, dx, y)
    assert np.array_equal(y.cpu().numpy(), want)
    # the same matrix held in COO (row-sorted, what every conversion produces): the container's plan is made from BOTH index arrays
    # (cmi_plan_create_coo) and its CSR sub-plan takes the run-compressed copy too
    import ctypes
    dAi = torch.empty(nnz, dtype=torch.int32, device="cuda")
    cmi.check(cmi.lib().cmi_csr_row_indices(rows, ctypes.c_void_p(dAp.data_ptr()), ctypes.c_void_p(dAi.data_ptr()), None))
    C = cmi.CooMatrix(rows, cols, nnz, dAi, dAj, dAx)
    y.fill_(10.0)
    cmi.multiply(C, dx, y)
    assert np.array_equal(y.cpu().numpy(), want), (name, "coo", C.plan().config())
    if name in ("ldoor", "nlpkkt120") and source.startswith("seeded"):
        assert C.plan().config().kernel == cmi.CSR_STREAM_WAVER, C.plan().config()
        assert C.plan().validate(dAi, dAj) is True
        with pytest.raises(cmi.CmiError):   # the plan owns a copy derived from the columns: validating it needs them
            C.plan().validate(dAi)
    plain = cmi.Plan(cmi.FORMAT_COO, torch.float64, rows, cols, nnz, dAi)   # (row indices only: the CSR kernels on row offsets, as in round 3)
    assert plain.config().kernel != cmi.CSR_STREAM_WAVER
    y.fill_(10.0)
    cmi.spmv_coo_plan(plain, dAi, dAj, dAx, dx, y)
    assert np.array_equal(y.cpu().numpy(), want), (name, "coo without the columns")
    del C, dAi
    # f32 values of the same matrix: the AUTO plan takes the run-compressed copy too (ldoor, nlpkkt120), the host loop's f32 bits
    Ax32, x32 = Ax.astype(np.float32), x.astype(np.float32)
    want32 = orc.spmv_csr(Ap, Aj, Ax32, x32, omp=True)
    dAx32, dx32 = dev(Ax32, torch), dev(x32, torch)
    auto32 = cmi.Plan.csr(torch.float32, rows, cols, dAp, dAj)
    if name in ("ldoor", "nlpkkt120") and source.startswith("seeded"):
        assert auto32.config().kernel == cmi.CSR_STREAM_WAVER, auto32.config()
    y32 = torch.full((rows,), 10.0, dtype=torch.float32, device="cuda")
    cmi.spmv_csr_plan(auto32, dAp, dAj, dAx32, dx32, y32)
    assert np.array_equal(y32.cpu().numpy(), want32), (name, "f32", auto32.config())


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_packed_wave_tiles_on_stencils(cmi, torch_cuda, orc, tag):
    """CMI_CSR_STREAM_PACKED on stencil-like rows: per wave tile of 64 rows ONE contiguous span [head | row starts |
    16-bit column offsets | values]; the multiply reads neither Ap nor Aj nor Ax.  Bit-exact against the host loop
    (sequential/multiply/csr_spmv.h:42-74) on 5-point Poisson grids (row counts that are and are not multiples of 64 / 256), accumulate,
    fused <y, w>; the plan owns a copy of the values: refreshed values are NOT seen and cmi_plan_validate_values says so."""
    torch = torch_cuda
    dtype, tdt = (np.float64, torch.float64) if tag == "f64" else (np.float32, torch.float32)
    for m, n in ((64, 48), (100, 100), (333, 77), (512, 512)):
        Ap, Aj, Ax = orc.poisson5pt_csr(m, n)
        Ax = (Ax * np.linspace(0.5, 1.5, len(Ax))).astype(dtype)  # (values that differ entry by entry)
        rows = cols = m * n
        x = orc.fill_x(cols).astype(dtype)
        y0 = np.linspace(-1.0, 1.0, rows).astype(dtype)
        dAp, dAj, dAx, dx = dev(Ap, torch), dev(Aj, torch), dev(Ax, torch), dev(x, torch)
        plan = cmi.Plan.csr_values(rows, cols, dAp, dAj, dAx, cmi.Config(kernel=cmi.CSR_STREAM_PACKED))
        c = plan.config()
        assert (c.kernel, c.items_per_thread, c.rows_per_block) == (cmi.CSR_STREAM_PACKED, 5, 64), c
        vb = 8 if tag == "f64" else 4
        assert plan.device_bytes() == -(-rows // 64) * (256 + 64 * 5 * (2 + vb)), plan.device_bytes()
        assert plan.info()["storage_order_sums"] is True
        want, want_acc = orc.spmv_csr(Ap, Aj, Ax, x), orc.spmv_csr(Ap, Aj, Ax, x, y0)
        y = torch.full((rows,), 9.0, dtype=tdt, device="cuda")
        cmi.spmv_csr_plan(plan, dAp, dAj, dAx, dx, y)
        assert np.array_equal(y.cpu().numpy(), want), (m, n)
        y = dev(y0, torch)
        cmi.spmv_csr_plan(plan, dAp, dAj, dAx, dx, y, accumulate=True)
        assert np.array_equal(y.cpu().numpy(), want_acc), (m, n, "accumulate")
        w = np.cos(np.arange(rows)).astype(dtype)
        res = torch.zeros(1, dtype=torch.float64, device="cuda")
        y = torch.zeros(rows, dtype=tdt, device="cuda")
        cmi.spmv_csr_dot(rows, cols, dAp, dAj, dAx, dx, y, dev(w, torch), res, cmi.blas_workspace(), plan=plan)
        assert np.array_equal(y.cpu().numpy(), want), (m, n, "dot")
        ref = float(np.dot(want.astype(np.float64), w.astype(np.float64)))
        assert abs(res.item() - ref) <= 1e-9 * float(np.dot(np.abs(want).astype(np.float64), np.abs(w).astype(np.float64))) + 1e-300
        assert plan.validate(dAp, dAj) and plan.validate_values(dAx)
        keep = dAx.clone()
        dAx.mul_(2.0)                                   # refreshed in place: the plan's copy is stale, and says so
        assert plan.validate_values(dAx) is False
        cmi.spmv_csr_plan(plan, dAp, dAj, dAx, dx, y)   # (still the OLD values: the documented contract of this opt-in)
        assert np.array_equal(y.cpu().numpy(), want)
        dAx.copy_(keep)


# ------------------------------------------------------------------------------------------------------------------------------------
# The REAL-FILE branch of configs[3] without the real files: a symmetric `coordinate real` MatrixMarket file of
# 10^6+ stored entries, named thermal2.mtx, dropped where CMI_SUITESPARSE_DIR points.  Both readers run: the C++ layer's
# (cusp/io/matrix_market.h, replacing /root/reference's cusp/io/detail/matrix_market.inl:160-300 -- symmetric expansion, sort by row and
# column) through tools/bin/spmv_bench, and the test path's (tools/suitesparse_like.py::load) through the every-CSR-variant body.
# ------------------------------------------------------------------------------------------------------------------------------------
def test_configs3_real_file_branch_on_a_written_mtx(cmi, torch_cuda, orc, tmp_path, monkeypatch):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import suitesparse_like as ssl
    import test_round3_gpu as r3
    from conftest import coo_to_csr
    Ap, Aj, Ax = ssl.thermal2_like(0.33)                       # symmetric PATTERN (every edge both ways + the diagonal)
    rows = len(Ap) - 1
    ri = np.repeat(np.arange(rows, dtype=np.int64), np.diff(Ap))
    low = ri >= Aj                                             # the stored half: lower triangle incl. the diagonal
    I, J, V = ri[low], Aj[low].astype(np.int64), Ax[low]
    assert len(I) >= 10 ** 6, len(I)
    path = tmp_path / "thermal2.mtx"
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real symmetric\n% written by tests/test_round4_gpu.py: the real-file branch of configs[3]\n")
        f.write(f"{rows} {rows} {len(I)}\n")
        np.savetxt(f, np.column_stack([I + 1, J + 1, V]), fmt="%d %d %.17g")
    off = I != J                                               # what the file MEANS: both triangles, sorted by row and column
    eAp, eAj, eAx = coo_to_csr(rows, np.concatenate([I, J[off]]), np.concatenate([J, I[off]]), np.concatenate([V, V[off]]))
    monkeypatch.setenv("CMI_SUITESPARSE_DIR", str(tmp_path))
    gAp, gAj, gAx, source = ssl.load("thermal2", 1.0)
    assert source.startswith("file "), source
    assert np.array_equal(gAp, eAp) and np.array_equal(gAj, eAj) and np.array_equal(gAx, eAx)   # %.17g: the values round-trip exactly
    r3.test_configs3_full_size_every_csr_variant(cmi, torch_cuda, orc, "thermal2")            # its load() now takes the file
    # the product's own reader: header-only C++ layer -> device containers -> every format's multiply against the host multiply
    exe = os.path.join(root, "tools", "bin", "spmv_bench")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(root, "tests", "cpp"), exe], check=True, capture_output=True)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stderr[-500:]
    assert f"with shape ({rows},{rows}) and {len(eAj)} entries" in r.stdout, r.stdout[:600]
    assert "RESULT MISMATCH" not in r.stdout
    assert sum(1 for k in ("coo ", "csr ", "ell ", "hyb ") if f"\t{k}:" in r.stdout and "GFLOP/s" in r.stdout) == 4, r.stdout


def test_bench_under_torchrun_n1_agrees_with_the_plain_run(torch_cuda):
    """the driver's SCALE run starts `bench.py --gpus 1` under torch.distributed.run; its N = 1 value must be the
    plain run's.  The launcher is started as a CHILD (nothing of it touches the GPU before its own child does); both runs use the driver's
    flags but 200 timed steps (a 24 ms region: the 20-step region of 2.4 ms wanders by +-1.5 % by itself).  3 % band."""
    import json
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    flags = ["--full", "--gpus", "1", "--steps", "200", "--warmup", "5", "--no-cpu-baseline", "--cg-iterations", "0"]
    env = dict(os.environ, CMI_BENCH_COLD="0")

    def line_of(cmd):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=root)
        assert r.returncode == 0, (r.stdout[-800:], r.stderr[-1500:])
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    plain = line_of([sys.executable, os.path.join(root, "bench.py")] + flags)
    launched = line_of([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(root, "bench.py")] + flags)
    for d in (plain, launched):
        assert d["n_gpus"] == 1 and d["metric"] == "spmv_gflops_fp64_poisson5pt" and d["roofline"]["frac"] > 0.6, d
    a, b = plain["roofline"]["kernel_avg_ms"], launched["roofline"]["kernel_avg_ms"]
    assert abs(a - b) <= 0.03 * a, (a, b)
    assert abs(plain["value"] - launched["value"]) <= 0.03 * plain["value"], (plain["value"], launched["value"])
    print(f"plain {plain['value']:.1f} GFLOP/s kernel {a * 1e3:.2f} us | under torch.distributed.run {launched['value']:.1f} GFLOP/s kernel {b * 1e3:.2f} us")


@pytest.mark.parametrize("fmt", ["ell", "dia", "coo", "hyb"])
def test_sharded_operator_in_the_other_formats_one_rank_through_rccl(cmi, torch_cuda, orc, fmt):
    """VERDICT r3 missing 6: row-block sharding for every container the hot path serves.  ShardedCsr(local_format=...) keeps the CSR
    block's partition and exchange and converts the block once; the multiply is exchange + the format's single-GPU multiply on the
    rectangular block.  Here with one rank through the C-ABI communicator (RCCL), against the oracle's host loops, and inside krylov.cg
    against the CSR operator's solve.  (World 2-3: tests/cpp/test_distributed.cpp run_formats, host_memory and ranks sharing the GPU.)"""
    torch = torch_cuda
    comm = cmi.binding.Comm(0, 1)
    m, n = 97, 83
    N = m * n
    A = cmi.poisson5pt(m, n, "csr")
    sh = cmi.distributed.ShardedCsr(A, N, 0, 1, mode="allgather", comm=comm, local_format=fmt)
    assert sh.local_format == fmt and type(sh.A).__name__.lower().startswith(fmt)
    x = cmi.fill_x(N).cuda()
    sh.x_local.copy_(x)
    y = torch.full((N,), 7.0, dtype=torch.float64, device="cuda")
    sh.multiply(y)
    Ap, Aj, Ax = orc.poisson5pt_csr(m, n)
    want = orc.spmv_csr(Ap, Aj, Ax, orc.fill_x(N))
    assert np.array_equal(y.cpu().numpy(), want), fmt   # one chain per row in each of these formats' default paths: the host loop's bits
    b = torch.ones(N, dtype=torch.float64, device="cuda")
    x1, x2 = torch.zeros_like(b), torch.zeros_like(b)
    mon1 = cmi.krylov.cg(sh, x1, b, iteration_limit=400, relative_tolerance=1e-8)
    mon2 = cmi.krylov.cg(A, x2, b, iteration_limit=400, relative_tolerance=1e-8)
    assert mon1.converged() and abs(mon1.iteration_count - mon2.iteration_count) <= 1
    assert torch.allclose(x1, x2, rtol=0, atol=1e-9)
    sh.vec.close()
    comm.close()


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_wave_tiles_that_overflow_take_further_passes(cmi, torch_cuda, orc, tag):
    """csr_wave with K entries per lane on rows LONGER than K (round 4: an explicit config on an irregular matrix, or the plan-less rule on a
    matrix that only looks like a stencil): a tile whose entries do not fit its 64 K slots runs the same body in passes of 64 K entries, every
    lane carrying its row's running sum across them -- the host loop's order (sequential/multiply/csr_spmv.h:56-73), so its bits.  Rows of
    2000 entries among rows of 1..9, empty rows, accumulate, the fused <y, w>; then the plan-less NULL-config call on a matrix whose sizes
    satisfy the stencil rule (mean 4.99) although its rows are 1..9 long."""
    torch = torch_cuda
    dtype, tdt = (np.float64, torch.float64) if tag == "f64" else (np.float32, torch.float32)
    rng = np.random.default_rng(77)
    rows = 20011
    lens = rng.integers(0, 10, size=rows)
    lens[[5, 4000, 4001, rows - 1]] = 2000
    lens[100:400] = 0
    cols = rows
    Ap = np.r_[0, np.cumsum(lens)].astype(np.int32)
    Aj = rng.integers(0, cols, size=int(Ap[-1])).astype(np.int32)
    Ax = rng.standard_normal(len(Aj)).astype(dtype)
    x = rng.standard_normal(cols).astype(dtype)
    y0 = rng.standard_normal(rows).astype(dtype)
    want, want_acc = orc.spmv_csr(Ap, Aj, Ax, x), orc.spmv_csr(Ap, Aj, Ax, x, y0)
    dAp, dAj, dAx, dx = dev(Ap, torch), dev(Aj, torch), dev(Ax, torch), dev(x, torch)
    for k in (2, 5, 10):
        cfg = cmi.Config(kernel=cmi.CSR_STREAM_WAVE, block_size=256, rows_per_block=256, items_per_thread=k, nontemporal=3)
        y = torch.full((rows,), 9.0, dtype=tdt, device="cuda")
        cmi.spmv_csr(rows, cols, dAp, dAj, dAx, dx, y, cfg=cfg)
        assert np.array_equal(y.cpu().numpy(), want), (tag, k)
        y = dev(y0, torch)
        cmi.spmv_csr(rows, cols, dAp, dAj, dAx, dx, y, accumulate=True, cfg=cfg)
        assert np.array_equal(y.cpu().numpy(), want_acc), (tag, k, "accumulate")
        w = rng.standard_normal(rows).astype(dtype)
        res = torch.zeros(1, dtype=torch.float64, device="cuda")
        y = torch.zeros(rows, dtype=tdt, device="cuda")
        cmi.spmv_csr_dot(rows, cols, dAp, dAj, dAx, dx, y, dev(w, torch), res, cmi.blas_workspace(), cfg=cfg)
        assert np.array_equal(y.cpu().numpy(), want), (tag, k, "dot")
        ref = float(np.dot(want.astype(np.float64), w.astype(np.float64)))
        assert abs(res.item() - ref) <= 1e-9 * float(np.dot(np.abs(want).astype(np.float64), np.abs(w).astype(np.float64))) + 1e-300
    # the plan-less rule: sizes say "stencil of 5" (mean within 0.5 % below 5), rows say otherwise
    rows2 = 200000
    lens2 = rng.integers(1, 10, size=rows2)
    target = int(4.99 * rows2)
    while lens2.sum() > target:
        i = rng.integers(0, rows2)
        if lens2[i] > 1:
            lens2[i] -= 1
    while lens2.sum() < target:
        i = rng.integers(0, rows2)
        if lens2[i] < 9:
            lens2[i] += 1
    Ap2 = np.r_[0, np.cumsum(lens2)].astype(np.int32)
    Aj2 = rng.integers(0, rows2, size=int(Ap2[-1])).astype(np.int32)
    Ax2 = rng.standard_normal(len(Aj2)).astype(dtype)
    x2 = rng.standard_normal(rows2).astype(dtype)
    y = torch.full((rows2,), 9.0, dtype=tdt, device="cuda")
    cmi.spmv_csr(rows2, rows2, dev(Ap2, torch), dev(Aj2, torch), dev(Ax2, torch), dev(x2, torch), y)   # NULL config, no plan
    assert np.array_equal(y.cpu().numpy(), orc.spmv_csr(Ap2, Aj2, Ax2, x2)), tag


def test_the_tables_waver_rule_steers_the_auto_plan(cmi, torch_cuda, orc):
    """The run-compressed copy's shape and size gate come from the tuning table ("waver_rule", tools/autotune_waver.py): a rule layered on
    top changes what an AUTO plan made with the columns runs -- and never the bits (every shape is the storage-order sum)."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import suitesparse_like as ssl
    torch = torch_cuda
    Ap, Aj, Ax = ssl.ldoor_like(0.3)       # ~14 M entries in blocks of 3 columns: over the shipped f64 gate
    rows = len(Ap) - 1
    x = np.random.default_rng(3).standard_normal(rows)
    want = orc.spmv_csr(Ap, Aj, Ax, x)
    dAp, dAj, dAx, dx = dev(Ap, torch), dev(Aj, torch), dev(Ax, torch), dev(x, torch)
    shipped = cmi.tuning_waver_rule(cmi.F64).as_dict()
    try:
        seen = []
        for rule in (shipped, dict(shipped, items_per_thread=2, cap=4, xcd_swizzle=0), dict(shipped, min_entries=int(Ap[-1]) + 1), dict(shipped, min_piece=3.5)):
            cmi.tuning_set_waver_rule(cmi.F64, **rule)
            plan = cmi.Plan.csr(torch.float64, rows, rows, dAp, dAj)
            c = plan.config()
            seen.append((c.kernel, c.items_per_thread, c.xcd_swizzle))
            y = torch.full((rows,), 7.0, dtype=torch.float64, device="cuda")
            cmi.spmv_csr_plan(plan, dAp, dAj, dAx, dx, y)
            assert np.array_equal(y.cpu().numpy(), want), rule
        assert seen[0] == (cmi.CSR_STREAM_WAVER, shipped["items_per_thread"], shipped["xcd_swizzle"])
        assert seen[1] == (cmi.CSR_STREAM_WAVER, 2, 0)
        assert seen[2][0] != cmi.CSR_STREAM_WAVER      # under the size gate
        assert seen[3][0] != cmi.CSR_STREAM_WAVER      # pieces of 3 are shorter than the rule asks for
    finally:
        cmi.tuning_set_waver_rule(cmi.F64, **shipped)


def test_stencil_rows_by_the_regret_runs_rules(cmi, torch_cuda, orc):
    """What tools/auto_regret.py found and tools/stencil_tiles_probe.py confirmed (profiles/r04_auto_regret.txt, r04_stencil_tiles_ab.txt):
    f64 stencil rows of 5..8 entries beyond the Infinity Cache run wave tiles of 256 entries with the 16-byte-vector body (csr_wavev,
    V = 1; f32: V = 2) instead of csr_wave; small matrices keep csr_wave; stencil rows of 8+ entries whose columns come in runs (9-point) take
    the run-compressed copy when the plan is made with the columns.  All bit-exact, plain, accumulating and through the fused dot."""
    torch = torch_cuda
    rng = np.random.default_rng(21)
    # the headline matrix
    m = 3162
    A = cmi.poisson5pt(m, m, "csr")
    N = A.num_rows
    for plan in (cmi.Plan.csr(torch.float64, N, N, A.row_offsets, A.column_indices), cmi.Plan(cmi.FORMAT_CSR, torch.float64, N, N, A.num_entries, A.row_offsets)):
        c = plan.config()
        assert (c.kernel, c.items_per_thread, c.nontemporal & 3) == (cmi.CSR_STREAM_WAVEV, 1, 3), c    # (with or without the columns: the partition needs the offsets only)
        assert plan.info()["storage_order_sums"] is True
    Ap, Aj, Ax = (t.cpu().numpy() for t in (A.row_offsets, A.column_indices, A.values))
    Ax = Ax * rng.standard_normal(len(Ax))
    x, y0 = rng.standard_normal(N), rng.standard_normal(N)
    want, want_acc = orc.spmv_csr(Ap, Aj, Ax, x), orc.spmv_csr(Ap, Aj, Ax, x, y0)
    dAx, dx = dev(Ax, torch), dev(x, torch)
    y = torch.full((N,), 3.0, dtype=torch.float64, device="cuda")
    cmi.spmv_csr_plan(plan, A.row_offsets, A.column_indices, dAx, dx, y)
    assert np.array_equal(y.cpu().numpy(), want)
    y = dev(y0, torch)
    cmi.spmv_csr_plan(plan, A.row_offsets, A.column_indices, dAx, dx, y, accumulate=True)
    assert np.array_equal(y.cpu().numpy(), want_acc)
    res = torch.zeros(1, dtype=torch.float64, device="cuda")
    y = torch.zeros(N, dtype=torch.float64, device="cuda")
    cmi.spmv_csr_dot(N, N, A.row_offsets, A.column_indices, dAx, dx, y, dx, res, cmi.blas_workspace(), plan=plan)
    assert np.array_equal(y.cpu().numpy(), want)
    assert abs(float(res) - float(np.dot(want, x))) <= 1e-12 * float(np.abs(want * x).sum())
    # f32: tiles of 512 entries (V = 2); a matrix inside the cache: csr_wave as before
    c32 = cmi.Plan.csr(torch.float32, N, N, A.row_offsets, A.column_indices).config()
    assert (c32.kernel, c32.items_per_thread) == (cmi.CSR_STREAM_WAVEV, 2), c32
    S = cmi.poisson5pt(1000, 1000, "csr")
    assert cmi.Plan.csr(torch.float64, S.num_rows, S.num_rows, S.row_offsets, S.column_indices).config().kernel == cmi.CSR_STREAM_WAVE
    del A, S, dAx, dx, y
    torch.cuda.empty_cache()
    # 9-point: three runs of 3 columns per row
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import autotune as at
    for tag, tdt, ndt in (("f64", torch.float64, np.float64), ("f32", torch.float32, np.float32)):
        Ap, Aj, Ax = at.stencil_csr(1200, 1200, 1, at.stencil_points(9), np.float64)      # 12.9 M entries: over both size gates
        Ax = (Ax * rng.standard_normal(len(Ax))).astype(ndt)
        N = len(Ap) - 1
        x = rng.standard_normal(N).astype(ndt)
        want = orc.spmv_csr(Ap, Aj, Ax, x)
        dAp, dAj, dAx, dx = dev(Ap, torch), dev(Aj, torch), dev(Ax, torch), dev(x, torch)
        plan = cmi.Plan.csr(tdt, N, N, dAp, dAj)
        assert plan.config().kernel == cmi.CSR_STREAM_WAVER, (tag, plan.config())
        assert cmi.Plan(cmi.FORMAT_CSR, tdt, N, N, len(Aj), dAp).config().kernel == cmi.CSR_STREAM_WAVE     # without the columns: as before
        y = torch.full((N,), 3.0, dtype=tdt, device="cuda")
        cmi.spmv_csr_plan(plan, dAp, dAj, dAx, dx, y)
        assert np.array_equal(y.cpu().numpy(), want), tag


def test_equal_row_lengths_are_a_stencil_only_if_the_columns_say_so(cmi, torch_cuda, orc):
    """6 entries in every row, columns drawn anywhere inside +-2000 of the diagonal: by its LENGTHS a stencil, by its columns a gather-bound
    band matrix.  A plan made with the columns sees that (97 % of the entries jump 16+ columns from their predecessor; a 7-point stencil:
    57 %) and takes the general rule's wave tiles (V = 4, with the x window) instead of a stencil kernel; a plan made from the row offsets
    alone cannot know and keeps the lengths' verdict.  Same bits either way (profiles/r04_auto_regret_equal_lengths.txt: 1.28-1.35 x faster)."""
    torch = torch_cuda
    rng = np.random.default_rng(33)
    rows, k = 6_000_000, 6
    Ap = (np.arange(rows + 1, dtype=np.int64) * k).astype(np.int32)
    base = np.repeat(np.arange(rows, dtype=np.int64), k)
    Aj = np.sort(np.clip(base + rng.integers(-2000, 2001, size=rows * k), 0, rows - 1).reshape(rows, k), axis=1).reshape(-1).astype(np.int32)
    Ax = rng.standard_normal(rows * k)
    x = rng.standard_normal(rows)
    want = orc.spmv_csr(Ap, Aj, Ax, x)
    dAp, dAj, dAx, dx = dev(Ap, torch), dev(Aj, torch), dev(Ax, torch), dev(x, torch)
    with_columns = cmi.Plan.csr(torch.float64, rows, rows, dAp, dAj)
    offsets_only = cmi.Plan(cmi.FORMAT_CSR, torch.float64, rows, rows, rows * k, dAp)
    cw, co = with_columns.config(), offsets_only.config()
    assert cw.kernel in (cmi.CSR_STREAM_WAVEX, cmi.CSR_STREAM_WAVEV) and cw.items_per_thread == 4, cw
    assert (co.kernel, co.items_per_thread) == (cmi.CSR_STREAM_WAVEV, 1), co
    for plan in (with_columns, offsets_only):
        y = torch.full((rows,), 4.0, dtype=torch.float64, device="cuda")
        cmi.spmv_csr_plan(plan, dAp, dAj, dAx, dx, y)
        assert np.array_equal(y.cpu().numpy(), want)


def test_auto_rules_from_the_later_regret_sets(cmi, torch_cuda, orc):
    """The rules that the regret table's sets 2-4 led to, pinned by what the AUTO plan selects -- and by the oracle's bits /
    bounds: rows that are ALL long keep the row-tile kernel (the merge-path kernel is for a TAIL of long rows); rows of 1..4 take wave
    tiles (mean >= 2); a gather-bound band matrix INSIDE the cache takes the plain wave tiles (f64 V = 2, f32 V = 4); the run-compressed
    copy from 2.2 / 1.9 entries per piece (5-point x 2 dof: exactly 2.5 but for the boundary rows), with V = 2 on short f64 rows."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import autotune as at
    torch = torch_cuda
    rng = np.random.default_rng(41)

    def stride_csr(lens, spread):
        lens = np.asarray(lens, np.int64)
        rows = len(lens)
        Ap = np.zeros(rows + 1, np.int64)
        Ap[1:] = np.cumsum(lens)
        row = np.repeat(np.arange(rows, dtype=np.int64), lens)
        j = np.arange(int(Ap[-1]), dtype=np.int64) - Ap[:-1][row]
        col = np.clip(row + (j - lens[row] // 2) * spread, 0, rows - 1)
        return Ap.astype(np.int32), col.astype(np.int32), rng.standard_normal(int(Ap[-1]))

    def run(name, Ap, Aj, Ax, tdt, expect, exact=True):
        ndt = np.float64 if tdt == torch.float64 else np.float32
        rows = len(Ap) - 1
        Ax = Ax.astype(ndt)
        x = rng.standard_normal(rows).astype(ndt)
        dAp, dAj, dAx, dx = dev(Ap, torch), dev(Aj, torch), dev(Ax, torch), dev(x, torch)
        plan = cmi.Plan.csr(tdt, rows, rows, dAp, dAj)
        c = plan.config()
        assert expect(c), (name, c)
        y = torch.full((rows,), 6.0, dtype=tdt, device="cuda")
        cmi.spmv_csr_plan(plan, dAp, dAj, dAx, dx, y)
        want = orc.spmv_csr(Ap, Aj, Ax, x)
        if exact:
            assert plan.info()["storage_order_sums"] is True and np.array_equal(y.cpu().numpy(), want), name
        else:   # lane groups add a long row: the 1e-6 class (|dy| <= 1e-6 sum |a_ij x_j|)
            bound = orc.spmv_csr(Ap, Aj, np.abs(Ax), np.abs(x))
            assert np.all(np.abs(y.cpu().numpy().astype(np.float64) - want) <= (1e-6 if ndt == np.float64 else 1e-4) * bound + 1e-300), name

    Ap, Aj, Ax = stride_csr(rng.integers(400, 1201, size=20_000), 1)
    run("all rows 400..1200 long", Ap, Aj, Ax, torch.float64, lambda c: c.kernel == cmi.CSR_STREAM and c.threads_per_row > 1, exact=False)
    Ap, Aj, Ax = stride_csr(rng.integers(1, 5, size=12_000_000), 3)
    assert Ap[-1] / 12_000_000 < 2.55
    run("rows of 1..4", Ap, Aj, Ax, torch.float64, lambda c: (c.kernel, c.items_per_thread) == (cmi.CSR_STREAM_WAVEV, 1))   # (f64 rows of < 8, none longer than 16: V = 1)
    del Ap, Aj, Ax
    Ap, Aj, Ax = at.synthetic_csr(1_000_000, 1_000_000, 16, 23, np.float64)        # 16 M entries: inside the cache in both value types
    run("band matrix inside the cache, f64", Ap, Aj, Ax, torch.float64, lambda c: (c.kernel, c.items_per_thread) == (cmi.CSR_STREAM_WAVEV, 2))
    run("band matrix inside the cache, f32", Ap, Aj, Ax, torch.float32, lambda c: (c.kernel, c.items_per_thread) == (cmi.CSR_STREAM_WAVEV, 4))
    Ap, Aj, Ax = at.block_expand(*at.stencil_csr(1200, 1200, 1, [(0, -1, 0, -1.0), (-1, 0, 0, -1.0), (0, 0, 0, 4.0), (1, 0, 0, -1.0), (0, 1, 0, -1.0)], np.float64), 2, np.float64)
    run("5-point x 2 dof, f64", Ap, Aj, Ax, torch.float64, lambda c: (c.kernel, c.items_per_thread) == (cmi.CSR_STREAM_WAVER, 2))
    run("5-point x 2 dof, f32", Ap, Aj, Ax, torch.float32, lambda c: (c.kernel, c.items_per_thread) == (cmi.CSR_STREAM_WAVER, 4))
