"""The 32-bit edges of the index types, on the device: matrices at the CSR entry ceiling (INT32_MAX - 65536 entries), the
5-point stencil at that ceiling, and a matrix whose columns reach INT32_MAX - 1.

Exact references by construction: every matrix is built on the device with small-integer values (A in {+-1, +-2, +-3},
x in {-4..4}, w in {-1, 0, 1}) and rows of at most 1.3e5 entries, so every product and partial row sum is an integer below
2^24 -- exact in f32 and f64 in any order of summation -- and every dot is an integer below 2^53.  The reference is a float64
index_add_ of the products over entry chunks, computed with torch (independent of this library), and every kernel is checked
with torch.equal: a dropped, duplicated or misplaced entry always shows, the atomic / order-free kernels included.  The
stencil is checked against bench.stencil_expected (bit-exact for the storage-order kernels).

Device memory: torch's measured peak per test (the library's own plan buffers come on top; need() asks for this much free):
E CSR 30 GiB (f64) / 21 GiB (f32); E SpMM + COO + HYB 60 / 43 GiB; stencil 42 GiB; columns 16 GiB; S 31 / 22 GiB; rows ~40 GiB;
wide ELL/DIA/HYB ~25 GiB; past 2^31 56 GiB.  The whole module runs in about 6 minutes on an MI355X."""
import pytest

pytestmark = pytest.mark.gpu

CEILING = 2**31 - 1 - 65536  # the most entries a CSR multiply takes ("int32 index ceiling")
CHUNK = 1 << 26              # entries per generation / reference chunk
GiB = 2**30


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch


def need(torch, gib):
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < gib * GiB:
        pytest.skip(f"needs about {gib} GiB of free device memory, {free / GiB:.1f} GiB free")


def mix(torch, v):
    """a 32-bit multiplicative hash of int64 positions (products stay below 2^63)"""
    return (v * 2654435761) & 0xFFFFFFFF


def small_vector(torch, n, dtype, salt, lo, hi):
    """x[i] in {lo..hi}, generated in chunks (no int64 temporary of the whole length)"""
    out = torch.empty(n, dtype=dtype, device="cuda")
    for s in range(0, n, 1 << 28):
        e = min(n, s + (1 << 28))
        i = torch.arange(s, e, dtype=torch.int64, device="cuda")
        out[s:e] = ((mix(torch, i + salt) >> 5) % (hi - lo + 1) + lo).to(dtype)
    return out


VALS = (-3.0, -2.0, -1.0, 1.0, 2.0, 3.0)


def nonzeros(torch, t):
    """count_nonzero over chunks (no temporary of the whole array)"""
    f = t.reshape(-1)
    return sum(int(torch.count_nonzero(f[s:s + (1 << 28)])) for s in range(0, f.numel(), 1 << 28))


def fill_entries(torch, Ap, num_cols, dtype, columns):
    """Aj / Ax for the row offsets Ap: columns(rows, h, k) -> int64 columns (k: the entry's place in its row); values from VALS
    by a hash of the position"""
    nnz = int(Ap[-1])
    Ap64 = Ap.to(torch.int64)
    Aj = torch.empty(nnz, dtype=torch.int32, device="cuda")
    Ax = torch.empty(nnz, dtype=dtype, device="cuda")
    vals = torch.tensor(VALS, dtype=dtype, device="cuda")
    for s in range(0, nnz, CHUNK):
        e = min(nnz, s + CHUNK)
        pos = torch.arange(s, e, dtype=torch.int64, device="cuda")
        rows = torch.searchsorted(Ap64, pos, right=True) - 1
        h = mix(torch, pos)
        Aj[s:e] = columns(rows, h, pos - Ap64[rows]).to(torch.int32)
        Ax[s:e] = vals[(h >> 11) % 6]
    del Ap64
    return Aj, Ax


def reference(torch, Ap, Aj, Ax, X):
    """Y = A X in float64 (X: a vector or a cols x k block), index_add_ over entry chunks: exact for these integer values"""
    if X.dim() == 2:  # one column at a time (a 2-D gather of 2^26 rows is one more temporary per column)
        return torch.stack([reference(torch, Ap, Aj, Ax, X[:, j].contiguous()) for j in range(X.shape[1])], 1)
    nnz = Aj.numel()
    rows = Ap.numel() - 1
    Ap64 = Ap.to(torch.int64)
    Y = torch.zeros(rows, dtype=torch.float64, device="cuda")
    for s in range(0, nnz, CHUNK):
        e = min(nnz, s + CHUNK)
        pos = torch.arange(s, e, dtype=torch.int64, device="cuda")
        r = torch.searchsorted(Ap64, pos, right=True) - 1
        Y.index_add_(0, r, X[Aj[s:e].to(torch.int64)].to(torch.float64) * Ax[s:e].to(torch.float64))
    del Ap64
    return Y


def entry_ceiling_matrix(torch, dtype):
    """E: exactly CEILING entries.  Rows in repeating units of 40 short rows (0..40 entries), 64 stencil-like rows of 5, one
    row of 512..4096 and 50 empty rows; row 0 has 70 000 entries; the last ~400 000 entries are a hand-made tail: a row of
    120 000, 2 000 rows of 5, short and empty rows, three rows of ~90 000 (more than 65536 each) and 777 empty rows at the
    very end."""
    unit = 155
    mean = 40 * 20 + 64 * 5 + 2304
    n_units = (CEILING - 400_000) // mean + 64
    u = torch.arange(n_units * unit, dtype=torch.int64, device="cuda")
    h = mix(torch, u)
    k = u % unit
    L = torch.zeros_like(u)
    L = torch.where(k < 40, h % 41, L)
    L = torch.where((k >= 40) & (k < 104), torch.full_like(u, 5), L)
    L = torch.where(k == 104, 512 + h % 3585, L)
    del u, h, k
    L[0] = 70_000
    cum = torch.cumsum(L, 0)
    keep = int(torch.searchsorted(cum, torch.tensor([CEILING - 400_000], device="cuda"), right=True))
    base = int(cum[keep - 1])
    del cum
    short = [0, 17, 3, 40, 1, 0, 0, 9] * 25
    fixed = 120_000 + 5 * 2000 + 3 * sum(short)
    rest = CEILING - base - fixed
    f1 = rest // 3
    f2 = (rest - f1) // 2
    f3 = rest - f1 - f2
    assert 65536 < f1 <= f3 < 130_000
    tail = [120_000] + [5] * 2000 + short + [f1] + short + [f2, f3] + short + [0] * 777
    L = torch.cat([L[:keep], torch.tensor(tail, dtype=torch.int64, device="cuda")])
    Ap = torch.zeros(L.numel() + 1, dtype=torch.int32, device="cuda")
    Ap[1:] = torch.cumsum(L, 0).to(torch.int32)
    del L
    assert int(Ap[-1]) == CEILING and int(Ap[-1 - 777]) == CEILING
    N = Ap.numel() - 1
    # a band of +-1024 columns around the row (wrapped): x gathers stay local, every column index is in range
    Aj, Ax = fill_entries(torch, Ap, N, dtype, lambda rows, h, k: torch.remainder(rows + (h % 2049) - 1024, N))
    return N, Ap, Aj, Ax


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_csr_at_the_entry_ceiling(cmi, torch_cuda, tag):
    """CSR kernels at nnz = INT32_MAX - 65536 (and at row prefixes of the same arrays: other residues of the entry count, a
    matrix ending in empty rows), every plan-less family, the planned paths and the fused dot -- exact against the reference."""
    torch = torch_cuda
    dtype = torch.float64 if tag == "f64" else torch.float32
    need(torch, 40 if tag == "f64" else 30)
    N, Ap, Aj, Ax = entry_ceiling_matrix(torch, dtype)
    x = small_vector(torch, N, dtype, 7, -4, 4)
    want = reference(torch, Ap, Aj, Ax, x)
    assert float(want.abs().max()) < 2**24
    y = torch.empty(N, dtype=dtype, device="cuda")

    def check(what, run, rows=N):
        y.fill_(1e30)
        run()
        assert torch.equal(y[:rows].to(torch.float64), want[:rows]), what

    C = cmi.Config
    planless = [None, C(kernel=cmi.CSR_SCALAR)]
    planless += [C(kernel=cmi.CSR_VECTOR, threads_per_row=t) for t in (2, 4, 8, 16, 32, 64)]
    planless += [C(kernel=cmi.CSR_STREAM, items_per_thread=i, block_size=b, threads_per_row=t)
                 for i, b, t in ((1, 256, 0), (2, 512, 1), (4, 1024, 0), (2, 1024, 4))]
    planless += [C(kernel=cmi.CSR_STREAM_PIPE), C(kernel=cmi.CSR_STREAM_WAVE, items_per_thread=5),
                 C(kernel=cmi.CSR_STREAM_WAVE, items_per_thread=10), C(kernel=cmi.CSR_BALANCED)]
    for cfg in planless:
        check(f"plan-less {None if cfg is None else cfg.as_dict()}",
              lambda: cmi.spmv_csr(N, N, Ap, Aj, Ax, x, y[:N], cfg=cfg))
    # row prefixes of the same arrays: the entry count ends on other residues mod 4 / 16, or the matrix ends in empty rows
    for r in (N - 1, N - 777, N - 800, N - 1000, N - 2000):
        nz = int(Ap[r])
        for cfg in (None, C(kernel=cmi.CSR_STREAM, items_per_thread=4, block_size=1024), C(kernel=cmi.CSR_BALANCED)):
            check(f"prefix of {r} rows ({nz} entries, {nz % 16} mod 16) {None if cfg is None else cfg.as_dict()}",
                  lambda: cmi.spmv_csr(r, N, Ap[:r + 1], Aj[:nz], Ax[:nz], x, y[:r], cfg=cfg), rows=r)
    # planned: the AUTO plan (profile: long rows), csr_stream's cooperative long-row instance, the wave-tile kernel in passes
    for cfg in (None, C(kernel=cmi.CSR_STREAM), C(kernel=cmi.CSR_STREAM, items_per_thread=4, block_size=1024, threads_per_row=4),
                C(kernel=cmi.CSR_STREAM_WAVE, items_per_thread=5), C(kernel=cmi.CSR_BALANCED)):
        plan = cmi.Plan.csr(dtype, N, N, Ap, Aj, cfg=cfg)
        check(f"plan {None if cfg is None else cfg.as_dict()} -> {plan.config().as_dict()}",
              lambda: cmi.spmv_csr_plan(plan, Ap, Aj, Ax, x, y))
        del plan
    # the fused <A x, w> with and without a plan: y exact, the dot exact (an integer below 2^53 summed in double)
    w = small_vector(torch, N, dtype, 11, -1, 1)
    want_dot = float((want * w.to(torch.float64)).sum())
    res = torch.zeros(1, dtype=torch.float64, device="cuda")
    ws = cmi.blas_workspace("cuda")
    for plan in (None, cmi.Plan.csr(dtype, N, N, Ap, Aj)):
        res.fill_(1e300)
        check("fused dot" + (" (plan)" if plan else ""),
              lambda: cmi.spmv_csr_dot(N, N, Ap, Aj, Ax, x, y, w, res, ws, plan=plan))
        assert float(res.item()) == want_dot, ("fused dot", plan is not None)
        del plan


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_spmm_coo_and_hyb_at_the_entry_ceiling(cmi, torch_cuda, tag):
    """SpMM (k = 2, 5; row- and column-major X / Y), COO (plan, tile, lane4, segmented) and HYB at nnz = INT32_MAX - 65536."""
    torch = torch_cuda
    dtype = torch.float64 if tag == "f64" else torch.float32
    need(torch, 64 if tag == "f64" else 44)
    N, Ap, Aj, Ax = entry_ceiling_matrix(torch, dtype)
    for k in (2, 5):
        X = torch.stack([small_vector(torch, N, dtype, 100 + j, -4, 4) for j in range(k)], 1)
        want = reference(torch, Ap, Aj, Ax, X)
        for xcm, ycm in ((False, False), (True, True), (True, False)):
            Xl = X.t().contiguous().t() if xcm else X
            Y = torch.full((k, N), 1e30, dtype=dtype, device="cuda").t() if ycm else torch.full((N, k), 1e30, dtype=dtype, device="cuda")
            cmi.spmm_csr(N, N, Ap, Aj, Ax, Xl, Y)
            assert torch.equal(Y.to(torch.float64), want), (k, xcm, ycm)
            del Xl, Y
        del X, want
    x = small_vector(torch, N, dtype, 7, -4, 4)
    want = reference(torch, Ap, Aj, Ax, x)
    y = torch.empty(N, dtype=dtype, device="cuda")
    Ai = torch.empty(CEILING, dtype=torch.int32, device="cuda")
    cmi.csr_row_indices(N, Ap, Ai)
    assert int(Ai[-1]) == N - 778 and int(Ai[0]) == 0
    plan = cmi.Plan.coo(dtype, N, N, Ai, Aj)
    y.fill_(1e30)
    cmi.spmv_coo_plan(plan, Ai, Aj, Ax, x, y)
    assert torch.equal(y.to(torch.float64), want), "coo plan"
    del plan
    for kern in (cmi.COO_TILE, cmi.COO_LANE4, cmi.COO_SEGMENTED):
        y.fill_(1e30)
        cmi.spmv_coo(N, N, Ai, Aj, Ax, x, y, cfg=cmi.Config(kernel=kern))
        assert torch.equal(y.to(torch.float64), want), f"coo kernel {kern}"
    del Ai
    torch.cuda.empty_cache()
    # HYB through its plan: ELL part of 4 per row, the rest (the long rows' tails) in the row-sorted COO part
    A = cmi.CsrMatrix(num_rows=N, num_cols=N, num_entries=CEILING, row_offsets=Ap, column_indices=Aj, values=Ax)
    H = cmi.convert(A, "hyb", num_entries_per_row=4)
    del A, Ap, Aj, Ax
    torch.cuda.empty_cache()
    y.fill_(1e30)
    cmi.multiply(H, x, y)
    assert torch.equal(y.to(torch.float64), want), "hyb plan"


def test_stencil_at_the_entry_ceiling(cmi, torch_cuda):
    """poisson5pt(20724, 20724): 2 147 337 984 entries, the largest square grid under the ceiling, f64, against the stencil's
    closed form -- the stencil paths (wave tiles, run-compressed, packed, 16-bit columns) at the top of the entry range."""
    import bench
    torch = torch_cuda
    need(torch, 60)
    m = n = 20724
    N = m * n
    want = bench.stencil_expected(torch, cmi, m, n, 0, N, "cuda")  # (first: its temporaries are gone before the matrix exists)
    torch.cuda.empty_cache()
    A = cmi.poisson5pt(m, n, "csr")
    assert A.num_entries == 2147337984 and int(A.row_offsets[-1]) == 2147337984
    x = cmi.fill_x(N).to("cuda")
    y = torch.empty(N, dtype=torch.float64, device="cuda")
    Ap, Aj, Ax = A.row_offsets, A.column_indices, A.values

    def check(what, run, exact=True):
        y.fill_(1e30)
        run()
        if exact:
            assert torch.equal(y, want), what
        else:
            assert float((y - want).abs().max()) <= 1e-6 * 8.0 * 0.51, what

    C = cmi.Config
    for cfg in (None, C(kernel=cmi.CSR_SCALAR), C(kernel=cmi.CSR_STREAM, items_per_thread=4, block_size=1024),
                C(kernel=cmi.CSR_STREAM_PIPE), C(kernel=cmi.CSR_STREAM_WAVE, items_per_thread=5)):
        check(f"plan-less {None if cfg is None else cfg.as_dict()}", lambda: cmi.spmv_csr(N, N, Ap, Aj, Ax, x, y, cfg=cfg))
    check("csr_balanced", lambda: cmi.spmv_csr(N, N, Ap, Aj, Ax, x, y, cfg=C(kernel=cmi.CSR_BALANCED)), exact=False)
    plans = [("auto", lambda: cmi.Plan.csr(x.dtype, N, N, Ap, Aj), None),
             ("wavev", lambda: cmi.Plan(cmi.FORMAT_CSR, x.dtype, N, N, A.num_entries, Ap, C(kernel=cmi.CSR_STREAM_WAVEV, items_per_thread=2)), cmi.CSR_STREAM_WAVEV),
             ("waver", lambda: cmi.Plan.csr(x.dtype, N, N, Ap, Aj, cfg=C(kernel=cmi.CSR_STREAM_WAVER, items_per_thread=1)), cmi.CSR_STREAM_WAVER),
             ("c16", lambda: cmi.Plan.csr(x.dtype, N, N, Ap, Aj, cfg=C(kernel=cmi.CSR_STREAM_C16)), cmi.CSR_STREAM_C16),
             ("packed", lambda: cmi.Plan.csr_values(N, N, Ap, Aj, Ax, cfg=C(kernel=cmi.CSR_STREAM_PACKED)), cmi.CSR_STREAM_PACKED)]
    for name, make, kernel in plans:
        plan = make()
        if kernel is not None:
            assert plan.config().kernel == kernel, (name, plan.config().as_dict())
        check(f"plan {name}", lambda: cmi.spmv_csr_plan(plan, Ap, Aj, Ax, x, y))
        del plan
        torch.cuda.empty_cache()


def test_columns_at_the_int32_ceiling(cmi, torch_cuda):
    """num_cols = INT32_MAX, 2^20 rows of 1..7 entries whose columns alternate per 64-row tile between [0, 65000) and
    [INT32_MAX - 1000, INT32_MAX - 1].  The 16-bit column copy on 64-row tiles then sees a tile based at the top of the range
    whose first 16-byte vector starts with entries of the tile before (offsets up to 65000 against THAT tile's base): their
    column, base + offset, must not wrap past INT32_MAX.  Every CSR path, exact against the reference, f32."""
    torch = torch_cuda
    need(torch, 20)
    rows, cols = 1 << 20, 2**31 - 1
    r = torch.arange(rows, dtype=torch.int64, device="cuda")
    L = 1 + mix(torch, r) % 7
    Ap = torch.zeros(rows + 1, dtype=torch.int32, device="cuda")
    Ap[1:] = torch.cumsum(L, 0).to(torch.int32)
    del r, L

    def columns(rr, h, k):
        top = (rr // 64) % 2 == 1
        return torch.where(top, cols - 1 - h % 1000, h % 65000)

    Aj, Ax = fill_entries(torch, Ap, cols, torch.float32, columns)
    assert int(Aj.max()) == cols - 1 or int(Aj.max()) > cols - 1000
    x = small_vector(torch, cols, torch.float32, 3, -4, 4)
    want = reference(torch, Ap, Aj, Ax, x)
    y = torch.empty(rows, dtype=torch.float32, device="cuda")
    nnz = Aj.numel()
    # the tiles whose first vector reaches back into a tile of the other cluster
    starts = Ap[64::64].to(torch.int64)
    assert int((starts % 4 != 0).sum()) > 1000

    def check(what, run):
        y.fill_(1e30)
        run()
        assert torch.equal(y.to(torch.float64), want), what

    C = cmi.Config
    for cfg in (None, C(kernel=cmi.CSR_SCALAR), C(kernel=cmi.CSR_VECTOR, threads_per_row=4), C(kernel=cmi.CSR_STREAM, items_per_thread=1),
                C(kernel=cmi.CSR_STREAM, items_per_thread=4, block_size=1024), C(kernel=cmi.CSR_STREAM_PIPE),
                C(kernel=cmi.CSR_STREAM_WAVE, items_per_thread=7), C(kernel=cmi.CSR_BALANCED)):
        check(f"plan-less {None if cfg is None else cfg.as_dict()}", lambda: cmi.spmv_csr(rows, cols, Ap, Aj, Ax, x, y, cfg=cfg))
    # (the run-compressed kernels take f64 and fewer than 2^30 columns: their plans refuse this matrix)
    for cfg in (None, C(kernel=cmi.CSR_STREAM_WAVEV, items_per_thread=2)):
        plan = cmi.Plan.csr(torch.float32, rows, cols, Ap, Aj, cfg=cfg)
        check(f"plan {None if cfg is None else cfg.as_dict()} -> {plan.config().as_dict()}", lambda: cmi.spmv_csr_plan(plan, Ap, Aj, Ax, x, y))
        del plan
    # the 16-bit copy on 64-row tiles, with 16-byte vectors (policy 0) and lane-strided requests (policy bit 4)
    for pol in (0, 4):
        plan = cmi.Plan.csr(torch.float32, rows, cols, Ap, Aj,
                            cfg=C(kernel=cmi.CSR_STREAM_C16, block_size=256, rows_per_block=64, items_per_thread=1, nontemporal=pol))
        got = plan.config()
        assert got.kernel == cmi.CSR_STREAM_C16 and got.rows_per_block == 64, got.as_dict()
        check(f"16-bit columns, policy {pol}", lambda: cmi.spmv_csr_plan(plan, Ap, Aj, Ax, x, y))
        del plan
    # COO through the row-sorted tile kernel and the segmented one
    Ai = torch.empty(nnz, dtype=torch.int32, device="cuda")
    cmi.csr_row_indices(rows, Ap, Ai)
    for kern in (cmi.COO_TILE, cmi.COO_SEGMENTED):
        check(f"coo {kern}", lambda: cmi.spmv_coo(rows, cols, Ai, Aj, Ax, x, y, cfg=C(kernel=kern)))


def short_row_ceiling_matrix(torch, dtype):
    """S: exactly CEILING entries in rows of 0..40 entries (a run of 100 empty rows at the end), each row's columns one run of
    consecutive columns near the diagonal -- the shape the wave-tile, run-compressed, packed and 16-bit plans accept"""
    n = CEILING // 20 + (1 << 22)
    r = torch.arange(n, dtype=torch.int64, device="cuda")
    L = mix(torch, r + 12345) % 41
    del r
    cum = torch.cumsum(L, 0)
    keep = int(torch.searchsorted(cum, torch.tensor([CEILING - 4096], device="cuda"), right=True))
    rest = CEILING - int(cum[keep - 1])
    del cum
    tail = [40] * (rest // 40) + [rest % 40] + [0] * 100
    L = torch.cat([L[:keep], torch.tensor(tail, dtype=torch.int64, device="cuda")])
    Ap = torch.zeros(L.numel() + 1, dtype=torch.int32, device="cuda")
    Ap[1:] = torch.cumsum(L, 0).to(torch.int32)
    del L
    assert int(Ap[-1]) == CEILING
    N = Ap.numel() - 1
    Aj, Ax = fill_entries(torch, Ap, N, dtype,
                          lambda rows, h, k: torch.clamp(rows + mix(torch, rows) % 64 - 32, 0, N - 41) + k)
    return N, Ap, Aj, Ax


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_short_rows_at_the_entry_ceiling(cmi, torch_cuda, orc, tag):
    """S at nnz = INT32_MAX - 65536 through the kernels that refuse E's long rows: the plan-built wave tiles (csr_wave on a
    partition, csr_wavev with V = 1, 2, 4, csr_wavex), the run-compressed and packed tiles (f64), the 16-bit column copy, plus the
    plan-less families and the fused dot.  The rows of the last 2^20 entries hold real values instead: they are checked against
    the CPU oracle (bit-exact for the storage-order kernels, within 1e-6 relative (f32: 1e-5) for csr_vector / csr_balanced),
    every other row exactly against the integer reference."""
    import numpy as np
    torch = torch_cuda
    dtype = torch.float64 if tag == "f64" else torch.float32
    need(torch, 56 if tag == "f64" else 36)
    N, Ap, Aj, Ax = short_row_ceiling_matrix(torch, dtype)
    x = small_vector(torch, N, dtype, 5, -4, 4)
    want = reference(torch, Ap, Aj, Ax, x)
    # the tail: rows whose entries all lie in the last 2^20 get real values
    rt = int(torch.searchsorted(Ap, torch.tensor([CEILING - 2**20], dtype=torch.int32, device="cuda")))
    e0 = int(Ap[rt])
    g = torch.Generator(device="cuda").manual_seed(3)
    Ax[e0:] = (torch.rand(CEILING - e0, generator=g, device="cuda", dtype=torch.float64) * 6 - 3).to(dtype)
    c0, c1 = int(Aj[e0:].min()), int(Aj[e0:].max())
    tAp = (Ap[rt:] - e0).cpu().numpy()
    tAj = (Aj[e0:] - c0).cpu().numpy()
    tAx = Ax[e0:].cpu().numpy()
    tx = x[c0:c1 + 1].cpu().numpy()
    want_tail = orc.spmv_csr(tAp, tAj, tAx, tx)
    bound_tail = float(np.max(orc.spmv_csr(tAp, tAj, np.abs(tAx), np.abs(tx))))
    rel = 1e-6 if tag == "f64" else 1e-5
    y = torch.empty(N, dtype=dtype, device="cuda")

    def check(what, run, exact=True):
        y.fill_(1e30)
        run()
        assert torch.equal(y[:rt].to(torch.float64), want[:rt]), what
        got = y[rt:].cpu().numpy()
        if exact:
            assert np.array_equal(got, want_tail), what + " (real-valued tail)"
        else:
            assert float(np.max(np.abs(got.astype(np.float64) - want_tail))) <= rel * bound_tail, what + " (real-valued tail)"

    C = cmi.Config
    for cfg, exact in ((None, True), (C(kernel=cmi.CSR_SCALAR), True), (C(kernel=cmi.CSR_VECTOR, threads_per_row=8), False),
                       (C(kernel=cmi.CSR_STREAM, items_per_thread=2, block_size=512), True), (C(kernel=cmi.CSR_STREAM_PIPE), True),
                       (C(kernel=cmi.CSR_STREAM_WAVE, items_per_thread=10), True), (C(kernel=cmi.CSR_BALANCED), False)):
        check(f"plan-less {None if cfg is None else cfg.as_dict()}", lambda: cmi.spmv_csr(N, N, Ap, Aj, Ax, x, y, cfg=cfg), exact)
    asked = [(C(kernel=cmi.CSR_STREAM_WAVE, items_per_thread=10), None),
             (C(kernel=cmi.CSR_STREAM_WAVEV, items_per_thread=1), cmi.CSR_STREAM_WAVEV),
             (C(kernel=cmi.CSR_STREAM_WAVEV, items_per_thread=2), cmi.CSR_STREAM_WAVEV),
             (C(kernel=cmi.CSR_STREAM_WAVEV, items_per_thread=4), cmi.CSR_STREAM_WAVEV),
             (C(kernel=cmi.CSR_STREAM_WAVEX, items_per_thread=2), cmi.CSR_STREAM_WAVEX),
             (C(kernel=cmi.CSR_STREAM_C16, block_size=1024, rows_per_block=64, items_per_thread=1), cmi.CSR_STREAM_C16)]
    if tag == "f64":
        asked.append((C(kernel=cmi.CSR_STREAM_WAVER, items_per_thread=4), cmi.CSR_STREAM_WAVER))
    for cfg, kernel in asked + [(None, None)]:
        plan = cmi.Plan.csr(dtype, N, N, Ap, Aj, cfg=cfg)
        got = plan.config()
        if kernel is not None:
            assert got.kernel == kernel, (cfg.as_dict(), got.as_dict())
        check(f"plan {None if cfg is None else cfg.as_dict()} -> {got.as_dict()}", lambda: cmi.spmv_csr_plan(plan, Ap, Aj, Ax, x, y),
              exact=plan.info()["storage_order_sums"])
        del plan
        torch.cuda.empty_cache()
    if tag == "f64":
        plan = cmi.Plan.csr_values(N, N, Ap, Aj, Ax, cfg=C(kernel=cmi.CSR_STREAM_PACKED))
        assert plan.config().kernel == cmi.CSR_STREAM_PACKED
        check("packed", lambda: cmi.spmv_csr_plan(plan, Ap, Aj, Ax, x, y))
        del plan
        torch.cuda.empty_cache()
    # the fused dot through the AUTO plan (the integer rows' part of <y, w> is exact; the tail's by the oracle's bound)
    w = small_vector(torch, N, dtype, 11, -1, 1)
    res = torch.zeros(1, dtype=torch.float64, device="cuda")
    plan = cmi.Plan.csr(dtype, N, N, Ap, Aj)
    check("fused dot (plan)", lambda: cmi.spmv_csr_dot(N, N, Ap, Aj, Ax, x, y, w, res, cmi.blas_workspace("cuda"), plan=plan),
          exact=plan.info()["storage_order_sums"])
    want_dot = float((want[:rt] * w[:rt].to(torch.float64)).sum()) + float(np.dot(want_tail.astype(np.float64), w[rt:].cpu().numpy()))
    assert abs(float(res.item()) - want_dot) <= 4 * rel * bound_tail * 2**20 + 1e-9 * abs(want_dot)


def test_rows_at_the_int32_ceiling(cmi, torch_cuda):
    """R: num_rows = INT32_MAX - 8, almost all empty: 4096 non-empty rows spread over the range and 512 clustered just before the
    last 88 rows, 1..16 entries each, f32.  CSR plan-less and planned, the fused dot (more tiles than its partial list: the plain
    dot follows), SpMM k = 2 and COO -- every non-empty row exact, every empty row exactly zero."""
    torch = torch_cuda
    need(torch, 40)
    rows, cols = 2**31 - 1 - 8, 1 << 20
    idx = torch.cat([torch.arange(4096, dtype=torch.int64, device="cuda") * (rows // 4096),
                     torch.arange(rows - 600, rows - 88, dtype=torch.int64, device="cuda")])
    lens = 1 + mix(torch, idx) % 16
    prefix = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(lens, 0)])
    nnz = int(prefix[-1])
    Ap = torch.empty(rows + 1, dtype=torch.int32, device="cuda")
    for s in range(0, rows + 1, 1 << 28):
        e = min(rows + 1, s + (1 << 28))
        Ap[s:e] = prefix[torch.searchsorted(idx, torch.arange(s, e, dtype=torch.int64, device="cuda"))].to(torch.int32)
    erow = torch.repeat_interleave(idx, lens)
    pos = torch.arange(nnz, dtype=torch.int64, device="cuda")
    h = mix(torch, pos)
    Aj = (h % cols).to(torch.int32)
    Ax = torch.tensor(VALS, dtype=torch.float32, device="cuda")[(h >> 11) % 6]
    x = small_vector(torch, cols, torch.float32, 9, -4, 4)
    comp = torch.searchsorted(idx, erow)  # the entry's row among the non-empty ones
    want = torch.zeros(idx.numel(), dtype=torch.float64, device="cuda")
    want.index_add_(0, comp, Ax.double() * x[Aj.long()].double())
    y = torch.empty(rows, dtype=torch.float32, device="cuda")

    def check(what, run):
        y.fill_(1e30)
        run()
        assert torch.equal(y[idx].double(), want), what
        assert nonzeros(torch, y) == int(torch.count_nonzero(want)), what + ": an empty row is not zero"

    C = cmi.Config
    for cfg in (None, C(kernel=cmi.CSR_SCALAR), C(kernel=cmi.CSR_VECTOR, threads_per_row=4), C(kernel=cmi.CSR_STREAM, items_per_thread=1),
                C(kernel=cmi.CSR_STREAM_PIPE), C(kernel=cmi.CSR_STREAM_WAVE, items_per_thread=4), C(kernel=cmi.CSR_BALANCED)):
        check(f"plan-less {None if cfg is None else cfg.as_dict()}", lambda: cmi.spmv_csr(rows, cols, Ap, Aj, Ax, x, y, cfg=cfg))
    plan = cmi.Plan.csr(torch.float32, rows, cols, Ap, Aj)
    check(f"plan -> {plan.config().as_dict()}", lambda: cmi.spmv_csr_plan(plan, Ap, Aj, Ax, x, y))
    w = small_vector(torch, rows, torch.float32, 13, -1, 1)
    res = torch.zeros(1, dtype=torch.float64, device="cuda")
    for p in (None, plan):
        check("fused dot", lambda: cmi.spmv_csr_dot(rows, cols, Ap, Aj, Ax, x, y, w, res, cmi.blas_workspace("cuda"), plan=p))
        assert float(res.item()) == float((want * w[idx].double()).sum()), "fused dot"
    del plan, w, y
    torch.cuda.empty_cache()
    X = torch.stack([x, small_vector(torch, cols, torch.float32, 21, -4, 4)], 1)
    Y = torch.full((rows, 2), 1e30, dtype=torch.float32, device="cuda")
    cmi.spmm_csr(rows, cols, Ap, Aj, Ax, X, Y)
    want2 = torch.zeros(idx.numel(), dtype=torch.float64, device="cuda")
    want2.index_add_(0, comp, Ax.double() * X[Aj.long(), 1].double())
    assert torch.equal(Y[idx, 0].double(), want) and torch.equal(Y[idx, 1].double(), want2), "spmm"
    assert nonzeros(torch, Y) == int(torch.count_nonzero(want)) + int(torch.count_nonzero(want2)), "spmm: an empty row is not zero"
    del Y
    torch.cuda.empty_cache()
    y = torch.empty(rows, dtype=torch.float32, device="cuda")
    Ai = erow.to(torch.int32)
    for kern in (None, cmi.COO_TILE, cmi.COO_SEGMENTED):
        check(f"coo {kern}", lambda: cmi.spmv_coo(rows, cols, Ai, Aj, Ax, x, y, cfg=None if kern is None else C(kernel=kern)))


def test_wide_ell_dia_hyb(cmi, torch_cuda):
    """W: 2^26 + 5 rows whose columns are one run starting 16 left of the diagonal; every 8th row has 33 entries, the others
    1..8.  Its ELL form (width 33) and HYB form (ELL width 32), and a DIA matrix of 33 diagonals over the same rows, hold
    width x pitch > 2^31 slots, f32."""
    torch = torch_cuda
    need(torch, 40)
    rows = (1 << 26) + 5
    r = torch.arange(rows, dtype=torch.int64, device="cuda")
    L = torch.where(r % 8 == 0, torch.full_like(r, 33), 1 + mix(torch, r) % 8)
    L = torch.minimum(L, rows + 16 - r)  # columns stay < rows
    del r
    Ap = torch.zeros(rows + 1, dtype=torch.int32, device="cuda")
    Ap[1:] = torch.cumsum(L, 0).to(torch.int32)
    del L
    Aj, Ax = fill_entries(torch, Ap, rows, torch.float32, lambda rr, h, k: torch.clamp(rr - 16, min=0) + k)
    assert int(Aj.max()) < rows
    x = small_vector(torch, rows, torch.float32, 17, -4, 4)
    want = reference(torch, Ap, Aj, Ax, x)
    y = torch.empty(rows, dtype=torch.float32, device="cuda")
    A = cmi.CsrMatrix(num_rows=rows, num_cols=rows, num_entries=Aj.numel(), row_offsets=Ap, column_indices=Aj, values=Ax)

    def check(M, what, cfg=None):
        y.fill_(1e30)
        cmi.multiply(M, x, y, cfg=cfg)
        assert torch.equal(y.double(), want), what

    E = cmi.convert(A, "ell")
    assert E.num_entries_per_row == 33 and 33 * E.pitch > 2**31
    check(E, "ell")
    check(E, "ell 2 rows per lane", cmi.Config(kernel=cmi.ELL_ROW, items_per_thread=2))
    del E
    torch.cuda.empty_cache()
    # DIA: 33 diagonals -16..16 of the same rows, built directly (the converter refuses W's fill-in); zero slots outside the matrix
    pitch = (rows + 31) // 32 * 32
    offsets = torch.arange(-16, 17, dtype=torch.int32, device="cuda")
    vals = small_vector(torch, 33 * pitch, torch.float32, 37, -3, 3)
    want_d = torch.zeros(rows, dtype=torch.float64, device="cuda")
    r = torch.arange(rows, dtype=torch.int64, device="cuda")
    for d in range(33):
        c = r + (d - 16)
        ok = (c >= 0) & (c < rows)
        v = vals[d * pitch:d * pitch + rows]
        v[~ok] = 0
        want_d += v.double() * x[c.clamp(0, rows - 1)].double()
    del r, c, ok
    assert 33 * pitch > 2**31
    for cfg in (None, cmi.Config(kernel=cmi.DIA_ROW, items_per_thread=2)):
        y.fill_(1e30)
        cmi.spmv_dia(rows, rows, 33, pitch, offsets, vals, x, y, cfg=cfg)
        assert torch.equal(y.double(), want_d), f"dia {cfg}"
    del vals, want_d
    torch.cuda.empty_cache()
    H = cmi.convert(A, "hyb", num_entries_per_row=32)
    assert 32 * H.ell.pitch > 2**31
    check(H, "hyb (ELL part past 2^31 slots)")


def test_int64_entry_points_past_2_31_elements(cmi, torch_cuda):
    """Plan-less COO (lane4, segmented, the default; aligned and one-entry-offset arrays) with 2^31 + 4099 entries and BLAS-1 with
    n = 2^31 + 17 (aligned and one-element-offset views), f32: these take int64 lengths and must be exact past 2^31."""
    torch = torch_cuda
    need(torch, 60)
    nnz, cols = 2**31 + 4099, 1 << 20
    rows = (nnz + 127) // 128
    Ai = torch.empty(nnz, dtype=torch.int32, device="cuda")
    Aj = torch.empty(nnz, dtype=torch.int32, device="cuda")
    Ax = torch.empty(nnz, dtype=torch.float32, device="cuda")
    vals = torch.tensor(VALS, dtype=torch.float32, device="cuda")
    x = small_vector(torch, cols, torch.float32, 23, -4, 4)
    want = torch.zeros(rows, dtype=torch.float64, device="cuda")
    for s in range(0, nnz, CHUNK):
        e = min(nnz, s + CHUNK)
        pos = torch.arange(s, e, dtype=torch.int64, device="cuda")
        h = mix(torch, pos)
        Ai[s:e] = (pos // 128).to(torch.int32)
        Aj[s:e] = (h % cols).to(torch.int32)
        Ax[s:e] = vals[(h >> 11) % 6]
        want.index_add_(0, pos // 128, Ax[s:e].double() * x[Aj[s:e].long()].double())
    want_off = want.clone()
    want_off[0] -= float(Ax[0]) * float(x[int(Aj[0])])
    y = torch.empty(rows, dtype=torch.float32, device="cuda")
    for kern in (None, cmi.COO_LANE4, cmi.COO_SEGMENTED):
        cfg = None if kern is None else cmi.Config(kernel=kern)
        for off, ref in ((0, want), (1, want_off)):
            y.fill_(1e30)
            cmi.spmv_coo(rows, cols, Ai[off:], Aj[off:], Ax[off:], x, y, cfg=cfg)
            assert torch.equal(y.double(), ref), (kern, off)
    del Ai, Aj, Ax, y, want, want_off
    torch.cuda.empty_cache()

    n = 2**31 + 17
    xb = small_vector(torch, n + 1, torch.float32, 29, -4, 4)
    yb = small_vector(torch, n + 1, torch.float32, 31, -4, 4)
    zb = torch.empty(n + 1, dtype=torch.float32, device="cuda")
    ws = cmi.blas_workspace("cuda")

    def chunked_dot(a, b):
        return sum(float((a[s:s + (1 << 28)].double() * b[s:s + (1 << 28)].double()).sum()) for s in range(0, n, 1 << 28))

    for off in (0, 1):
        xv, yv, zv = xb[off:off + n], yb[off:off + n], zb[off:off + n]
        exact = chunked_dot(xv, yv)
        rd = torch.zeros(1, dtype=torch.float64, device="cuda")
        cmi.blas_dotd(xv, yv, rd, ws)
        assert float(rd.item()) == exact, ("dotd", off)
        rf = torch.zeros(1, dtype=torch.float32, device="cuda")
        cmi.blas_dot(xv, yv, rf, ws)
        assert float(rf.item()) == float(torch.tensor(exact, dtype=torch.float32)), ("dot", off)
        cmi.blas_nrm2(xv, rf, ws)
        nrm = chunked_dot(xv, xv) ** 0.5
        assert abs(float(rf.item()) - nrm) <= 2**-23 * nrm, ("nrm2", off)
        cmi.blas_axpby(2.0, xv, -3.0, yv, zv)
        for s in range(0, n, 1 << 28):
            assert torch.equal(zv[s:s + (1 << 28)], 2 * xv[s:s + (1 << 28)] - 3 * yv[s:s + (1 << 28)]), ("axpby", off, s)
        cmi.blas_copy(xv, zv)
        assert torch.equal(zv, xv), ("copy", off)
        cmi.blas_axpy(2.0, yv, zv)  # z = x + 2 y
        for s in range(0, n, 1 << 28):
            assert torch.equal(zv[s:s + (1 << 28)], xv[s:s + (1 << 28)] + 2 * yv[s:s + (1 << 28)]), ("axpy", off, s)
        cmi.blas_fill(-7.0, zv)
        assert nonzeros(torch, zv + 7.0) == 0, ("fill", off)
