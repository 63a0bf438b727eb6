"""GPU tests (-m gpu) of cmi_dense_gemm_{f64,f32} (csrc/dense.hip) through cmi.dense_gemm, in the shape of tests/test_lobpcg_gpu.py.

Bars for every case (reference: lanczos_refs.gemm_ref, checked on the CPU by tests/test_lanczos_refs.py):
  * C BIT-EQUAL to the restatement (special_values.same_bits: NaN against NaN at the same position); C holds NaN before the call;
  * guard elements round every operand, the padding between C's columns, and all of A and B unchanged;
  * a second call on restored inputs gives the same bits.
Sizes.  kBlasBlock = 256 lanes, a lane owns W rows (one 16-byte piece: 2 doubles / 4 floats): m runs round one workgroup's W * 256 rows;
k round the unroll factor kUnroll = 4 and the staged chunk of B, kChunk = 64; n round the group of kCols = 8 columns.  The grid is
fused_grid(m, W): capped at kFusedMaxGrid = 65536 workgroups, tile-strided past it -- GRID_M is five rows past the first stride."""
import numpy as np
import pytest

import lanczos_refs as R
import special_values as sv
from test_blas_extra_gpu import Operand, bits

pytestmark = pytest.mark.gpu

TYPES = {"f32": np.float32, "f64": np.float64}
K_BLAS_BLOCK, K_UNROLL, K_CHUNK, K_COLS, K_MAX_GRID = 256, 4, 64, 8, 1 << 16   # csrc/blas1_shared.h, csrc/dense.hip
KS = (0, 1, 2, K_UNROLL - 1, K_UNROLL + 1, K_CHUNK - 1, K_CHUNK, K_CHUNK + 1, 70)
NS = (0, 1, K_COLS - 1, K_COLS, K_COLS + 1, 17)
NAN = float("nan")


def rows(T):
    W = 16 // np.dtype(T).itemsize
    return (0, 1, 3, W * K_BLAS_BLOCK - 1, W * K_BLAS_BLOCK + 1, 4099)


def shapes(T):
    """Every value of each axis with at least two values of each of the others."""
    MS = rows(T)
    out = []
    for i, k in enumerate(KS):
        out += [(MS[(i + 2) % 6], k, NS[(i + 1) % 6]), (MS[(i + 5) % 6], k, NS[(i + 3) % 6])]
    for i, n in enumerate(NS):
        out += [(MS[(i + 1) % 6], KS[(2 * i + 1) % 9], n), (MS[(i + 4) % 6], KS[(2 * i + 6) % 9], n)]
    for i, m in enumerate(MS):
        out += [(m, KS[(3 * i + 2) % 9], NS[(i + 2) % 6]), (m, KS[(3 * i + 7) % 9], NS[(i + 5) % 6])]
    out = list(dict.fromkeys(out))
    for axis, values in ((0, MS), (1, KS), (2, NS)):
        for v in values:
            mine = [s for s in out if s[axis] == v]
            assert all(len({s[o] for s in mine}) >= 2 for o in range(3) if o != axis), (axis, v, mine)
    return out


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch


def leading(kind, rows_):
    return {"tight": rows_, "odd": rows_ + 1 if rows_ % 2 == 0 else rows_ + 2, "pad64": -(-max(rows_, 1) // 64) * 64}[kind]


def run_case(cmi, torch, T, m, k, n, lda, ldb, ldc, offs=(0, 0, 0), A=None, B=None, what=""):
    """One product (made twice) on views at the given element offsets; A (lda x k), B (ldb x n) flat column-major host arrays or None (drawn)."""
    what = f"{what} {np.dtype(T).name} m={m} k={k} n={n} ld=({lda},{ldb},{ldc}) offsets={offs}"
    rng = np.random.default_rng(m * 1000003 + k * 1009 + n)
    A = rng.standard_normal(lda * k).astype(T) if A is None else A
    B = rng.standard_normal(ldb * n).astype(T) if B is None else B
    C0 = np.full(ldc * n, NAN, T)
    with np.errstate(all="ignore"):
        inner = R.gemm_ref(A.reshape(k, lda)[:, :m].T.copy(), B.reshape(n, ldb)[:, :k].T.copy())
    want = C0.copy().reshape(n, ldc)
    want[:, :m] = inner.T
    want = want.reshape(-1)
    ops = [Operand(torch, T, v, off) for v, off in zip((A, B, C0), offs)]
    runs = []
    for trip in range(2):
        if trip:
            for op in ops:
                op.restore(torch)
        cmi.dense_gemm(m, n, k, ops[0].view, lda, ops[1].view, ldb, ops[2].view, ldc)
        after = [op.after() for op in ops]   # (the guards are checked there)
        assert bits(after[0]) == bits(ops[0].before) and bits(after[1]) == bits(ops[1].before), f"{what}: A or B changed"
        sv.same_bits(ops[2].inner(after[2]), want, f"{what}: C (trip {trip})")
        runs.append(after[2])
    sv.same_bits(runs[0], runs[1], f"{what}: the second call")


@pytest.mark.parametrize("tname", list(TYPES))
def test_gemm_against_restatement(cmi, torch_cuda, tname):
    """Every shape; the leading dimensions tight, odd (columns of A off the 16-byte grid: the element path) and padded to 64, ldb > k and
    ldc > m among them; every operand in turn one element off the grid."""
    T = TYPES[tname]
    kinds = ("tight", "odd", "pad64")
    for i, (m, k, n) in enumerate(shapes(T)):
        lda, ldb, ldc = leading(kinds[i % 3], m), k + (i % 4), leading(kinds[(i // 3) % 3], m)
        offs = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)][i % 5]
        run_case(cmi, torch_cuda, T, m, k, n, lda, ldb, ldc, offs)
    m = rows(T)[4]
    for kind in kinds:   # one shape through every leading dimension of A, aligned and not
        for off in (0, 1):
            run_case(cmi, torch_cuda, T, m, 5, 9, leading(kind, m), 7, m + 3, (off, 0, off), what=kind)


@pytest.mark.parametrize("tname", list(TYPES))
def test_special_values_go_through_bit_for_bit(cmi, torch_cuda, tname):
    """-0.0, +-Inf, NaN, subnormals, the largest and the smallest normal number in both operands: products and sums as the host loop forms
    them (one chain starts from +0, so a column of -0 products gives +0)."""
    T = TYPES[tname]
    tiny = np.finfo(T).smallest_subnormal
    special = np.array([-0.0, 0.0, np.inf, -np.inf, np.nan, tiny, -tiny, 1.0, -1.0, np.finfo(T).max, np.finfo(T).tiny, 0.5], T)
    m, n, k = 1031, 9, len(special)
    A = np.concatenate([np.resize(np.roll(special, j), m) for j in range(k)]).astype(T)
    B = np.concatenate([np.roll(special[::-1], 5 * c) for c in range(n)]).astype(T)
    for off in (0, 1):
        run_case(cmi, torch_cuda, T, m, k, n, m, k, m, (off, off, off), A=A, B=B, what="special")
    zeros = np.full(m * 3, -0.0, T)
    run_case(cmi, torch_cuda, T, m, 3, 2, m, 3, m, A=zeros, B=np.ones(6, T), what="minus zero")


@pytest.mark.parametrize("tname", list(TYPES))
def test_gemm_past_one_grid_stride(cmi, torch_cuda, tname):
    """m = 65536 * 256 * W + 5: the first workgroup makes a second trip with a full piece and a ragged one."""
    T = TYPES[tname]
    W = 16 // np.dtype(T).itemsize
    m = K_MAX_GRID * K_BLAS_BLOCK * W + 5
    run_case(cmi, torch_cuda, T, m, 2, 1, m, 2, m, what="grid stride")


def test_gemm_offsets_are_64_bit(cmi, torch_cuda):
    """lda = 2^31 + 3 in float: the second column of A starts past 2^31 elements (and past 2^33 bytes).  The 8.6 GB buffer is not initialised;
    only the ten elements the product reads are written."""
    torch = torch_cuda
    from test_index_ceiling_gpu import need
    need(torch, 10)
    lda, m, k, n = 2 ** 31 + 3, 5, 2, 1
    buf = torch.empty(lda + m + 1, dtype=torch.float32, device="cuda")
    a0, a1 = np.arange(1, 6, dtype=np.float32) / 3, np.arange(7, 12, dtype=np.float32) / 7
    for off in (0, 1):
        A = buf[off:]
        A[:m] = torch.from_numpy(a0).cuda()
        A[lda:lda + m] = torch.from_numpy(a1).cuda()
        B = torch.tensor([0.3, -1.7], dtype=torch.float32, device="cuda")
        C = torch.full((m,), NAN, dtype=torch.float32, device="cuda")
        cmi.dense_gemm(m, n, k, A, lda, B, k, C, m)
        want = R.gemm_ref(np.stack([a0, a1], 1), B.cpu().numpy().reshape(2, 1))[:, 0]
        sv.same_bits(C.cpu().numpy(), want, f"lda = 2^31 + 3, offset {off}")
    del buf
    torch.cuda.empty_cache()


def test_gemm_refusals_on_the_device(cmi, torch_cuda):
    torch = torch_cuda
    for dt in (torch.float64, torch.float32):
        A, B = torch.ones(40, dtype=dt, device="cuda"), torch.ones(15, dtype=dt, device="cuda")
        C = torch.full((27,), NAN, dtype=dt, device="cuda")
        cmi.dense_gemm(8, 3, 4, A, 10, B, 5, C, 9)
        got = C.cpu().numpy().reshape(3, 9)
        assert np.all(got[:, :8] == 4.0) and np.all(np.isnan(got[:, 8]))
        for args, word in (((-1, 3, 4, A, 10, B, 5, C, 9), "negative"), ((8, 3, 4, A, 7, B, 5, C, 9), "leading dimension"), ((8, 3, 4, A, 10, B, 3, C, 9), "leading dimension"),
                           ((8, 3, 4, A, 10, B, 5, C, 7), "leading dimension"), ((8, 3, 4, A, 10, B, 5, A[8:], 9), "overlaps"), ((8, 3, 4, A, 10, B, 5, B[2:], 9), "overlaps"),
                           ((8, 3, 4, None, 10, B, 5, C, 9), "null")):
            with pytest.raises(cmi.CmiError) as e:
                cmi.dense_gemm(*args)
            assert e.value.status == 1 and word in str(e.value), (args[:3], word, str(e.value))
        cmi.dense_gemm(0, 3, 4, A, 1, B, 5, C, 1)   # nothing to write
        cmi.dense_gemm(8, 0, 4, A, 10, B, 5, C, 9)
        torch.cuda.synchronize()
        assert np.all(C.cpu().numpy().reshape(3, 9)[:, :8] == 4.0)
