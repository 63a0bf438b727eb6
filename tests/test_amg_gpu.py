"""The set-up kernels of smoothed-aggregation multigrid (csrc/amg.hip) on the MI355X, through the C-ABI, against
tests/amg_refs.py: structure exactly, values bit for bit (special_values.same_bits), f64 and f32.  No tolerance anywhere.
"""
import ctypes

import numpy as np
import pytest

import amg_refs as R
import special_values as SV
import spgemm_refs as SR
from special_values import same_bits

pytestmark = pytest.mark.gpu
DT = [np.float64, np.float32]
INVALID = 1
CEILING = 2**31 - 1 - 65536


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch


def dev(a, torch):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(ts):
    return tuple(t.cpu().numpy() for t in ts)


def check_csr(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: row offsets differ"
    assert got[0][-1] == len(got[1]) == len(got[2]), what
    assert np.array_equal(got[1], want[1]), f"{what}: column indices differ"
    same_bits(got[2], want[2], what)


def free_bytes(torch):
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def assert_memory_returns(cmi, torch, call):
    """`call` leaves the device bytes held by the library where they were (its own results are dropped before the reading)."""
    L = cmi.lib()
    call()                                                     # warm-up: code objects and the runtime's pools are in place
    before = free_bytes(torch)
    p = ctypes.c_void_p()
    cmi.check(L.cmi_malloc(ctypes.byref(p), 1))
    held = free_bytes(torch)
    cmi.check(L.cmi_free(p))
    slack = max(before - held, abs(before - free_bytes(torch)))
    base = free_bytes(torch)
    call()
    assert abs(free_bytes(torch) - base) <= slack, "scratch still held after the call"


def random_csr(rng, lens, n_cols, dtype, diag=True):
    """Rows of the given lengths, columns unsorted and possibly repeated, the diagonal stored in most rows."""
    rows = []
    for i, l in enumerate(lens):
        cols = rng.integers(0, n_cols, size=l)
        if diag and l and i % 7 != 3:
            cols[rng.integers(0, l)] = i
        rows.append(cols)
    Ap = np.r_[0, np.cumsum(lens)].astype(np.int32)
    Aj = np.concatenate(rows + [np.zeros(0, np.int64)]).astype(np.int32)
    return Ap, Aj, rng.standard_normal(len(Aj)).astype(dtype)


# ---- (a) strength ---------------------------------------------------------------------------------------------------------
def device_strength(cmi, torch, n, Ap, Aj, Ax, theta):
    return host(cmi.csr_strength_symmetric(n, dev(Ap, torch), dev(Aj, torch), dev(Ax, torch), theta))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("theta", [0.0, 0.25, 1.0])
def test_strength_row_lengths_around_the_wave(cmi, torch_cuda, dtype, theta):
    rng = np.random.default_rng(11)
    lens = np.r_[rng.integers(0, 9, size=130), [63, 64, 65, 0, 1000, 0, 0, 64, 65, 129], rng.integers(0, 9, size=70)]
    n = len(lens)
    Ap, Aj, Ax = random_csr(rng, lens, n, dtype)
    Ax[Aj == R.csr_rows(Ap)] *= 3                               # a diagonal that makes theta = 0.25 and 1 cut through the rows
    got = device_strength(cmi, torch_cuda, n, Ap, Aj, Ax, theta)
    want = R.strength(n, Ap, Aj, Ax, theta)
    check_csr(got, want, f"theta {theta}")
    if theta == 0:
        assert len(got[1]) == len(Aj)
    else:
        assert 0 < len(got[1]) < len(Aj)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", [255, 256, 257, 2047, 2048, 2049])
def test_strength_row_counts_around_the_workgroup_and_the_scan_tile(cmi, torch_cuda, dtype, n):
    rng = np.random.default_rng(n)
    Ap, Aj, Ax = random_csr(rng, rng.integers(0, 7, size=n), n, dtype)
    check_csr(device_strength(cmi, torch_cuda, n, Ap, Aj, Ax, 0.5), R.strength(n, Ap, Aj, Ax, 0.5), f"{n} rows")


@pytest.mark.parametrize("dtype", DT)
def test_strength_degenerate_and_diagonal_cases(cmi, torch_cuda, dtype):
    e, ev = np.zeros(0, np.int32), np.zeros(0, dtype)
    got = device_strength(cmi, torch_cuda, 0, np.zeros(1, np.int32), e, ev, 0.25)
    assert got[0].tolist() == [0] and len(got[1]) == 0
    got = device_strength(cmi, torch_cuda, 5, np.zeros(6, np.int32), e, ev, 0.25)
    assert got[0].tolist() == [0] * 6
    # row 0: no diagonal (A_00 = 0: the threshold is 0, everything stays); row 1: the diagonal twice (2 + 2 = 4);
    # row 2: empty; row 3: the diagonal twice, cancelling to 0
    rows = [[(1, 0.5), (2, -0.25)], [(1, 2.0), (0, 0.9), (1, 2.0), (3, 1e-3)], [], [(3, 1.0), (1, 0.1), (3, -1.0)]]
    Ap, Aj, Ax = SR.csr(rows, dtype)
    for theta in (0.0, 0.25, 1.0):
        want = R.strength(4, Ap, Aj, Ax, theta)
        check_csr(device_strength(cmi, torch_cuda, 4, Ap, Aj, Ax, theta), want, f"diagonals, theta {theta}")
    assert R.diagonal(4, Ap, Aj, Ax).tolist() == [0, 4, 0, 0]
    # every entry dropped: theta so large that not even the diagonal passes
    N, Ap, Aj, Ax = SR.poisson5pt(20, 13, dtype)
    got = device_strength(cmi, torch_cuda, N, Ap, Aj, Ax, 1e30)
    assert not got[0].any() and len(got[1]) == 0 and len(R.strength(N, Ap, Aj, Ax, 1e30)[1]) == 0


@pytest.mark.parametrize("dtype", DT)
def test_strength_one_ulp_either_side_of_the_threshold(cmi, torch_cuda, dtype):
    for n, Ap, Aj, Ax, theta, keep in R.threshold_deck(dtype):
        got = device_strength(cmi, torch_cuda, n, Ap, Aj, Ax, theta)
        check_csr(got, R.strength(n, Ap, Aj, Ax, theta), f"A_01 = {Ax[1]!r}, theta {theta}")
        assert ((0, 1) in set(zip(R.csr_rows(got[0]).tolist(), got[1].tolist()))) == keep
    if dtype == np.float32:                                    # the product with theta and the comparison are in double
        n, Ap, Aj, Ax, theta, keep = R.value_type_threshold_case()
        got = device_strength(cmi, torch_cuda, n, Ap, Aj, Ax, theta)
        check_csr(got, R.strength(n, Ap, Aj, Ax, theta), "threshold in double")
        assert not keep and len(got[1]) == 2


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("deck", SV.DECKS)
def test_strength_special_values(cmi, torch_cuda, dtype, deck):
    M = SV.matrices(dtype)["poisson100"]
    Ax, x, _ = SV.decks(M, dtype)[deck]
    with np.errstate(all="ignore"):
        vals = (Ax * x[M.Aj]).astype(dtype)                     # NaN, Inf, signed zeros, subnormals and overflow among the entries
    for theta in (0.0, 0.25):
        check_csr(device_strength(cmi, torch_cuda, M.rows, M.Ap, M.Aj, vals, theta), R.strength(M.rows, M.Ap, M.Aj, vals, theta), f"{deck}, theta {theta}")


# ---- (b) scale_rows, (e) presmooth ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
def test_scale_rows_in_place_and_special_diagonals(cmi, torch_cuda, dtype):
    torch = torch_cuda
    rng = np.random.default_rng(12)
    lens = np.r_[rng.integers(0, 6, size=300), [0, 0, 700, 0], rng.integers(0, 6, size=300)]
    n = len(lens)
    Ap, Aj, Ax = random_csr(rng, lens, n, dtype)
    d = rng.standard_normal(n).astype(dtype)
    d[:8] = [0.0, -0.0, np.inf, np.nan, -np.inf, 1.0, 0.0, -0.0]
    lam = 4.0 / 3.0 / 1.987
    want = R.scale_rows(Ap, Ax, d, lam)
    dAp, dAx, dd = dev(Ap, torch), dev(Ax, torch), dev(d, torch)
    out = cmi.csr_scale_rows(n, dAp, dAx, dd, lam)
    same_bits(out.cpu().numpy(), want, "scale_rows")
    same_bits(dAx.cpu().numpy(), Ax, "the input is untouched")
    assert cmi.csr_scale_rows(n, dAp, dAx, dd, lam, out=dAx) is dAx     # aliased: in place
    same_bits(dAx.cpu().numpy(), want, "scale_rows in place")
    assert np.isnan(want).any() and np.isinf(want).any()
    empty = cmi.csr_scale_rows(0, dev(np.zeros(1, np.int32), torch), dev(np.zeros(0, dtype), torch), dev(np.zeros(0, dtype), torch), lam)
    assert empty.numel() == 0


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", [0, 1, 257])
def test_jacobi_presmooth(cmi, torch_cuda, dtype, n):
    torch = torch_cuda
    rng = np.random.default_rng(13 + n)
    d, b = rng.standard_normal(n).astype(dtype), rng.standard_normal(n).astype(dtype)
    if n > 8:
        d[:8] = [0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -1e30, 3.0]
        b[:3] = [0.0, 1.0, np.inf]
    omega = 4.0 / 3.0 / 1.93
    x = dev(np.full(n, 7.0, dtype), torch)
    cmi.relax_jacobi_presmooth(dev(d, torch), dev(b, torch), omega, x)
    same_bits(x.cpu().numpy(), R.presmooth(d, b, omega), f"presmooth n = {n}")


# ---- (c) fit --------------------------------------------------------------------------------------------------------------
def device_fit(cmi, torch, agg, B, na):
    return host(cmi.aggregates_fit(dev(agg, torch), dev(B, torch), na))


def check_fit(got, want, what):
    check_csr(got[:3], want[:3], what)
    same_bits(got[3], want[3], what + ": R")


@pytest.mark.parametrize("dtype", DT)
def test_fit_shapes_of_aggregates(cmi, torch_cuda, dtype):
    rng = np.random.default_rng(14)
    n = 1500
    B = rng.standard_normal(n).astype(dtype)
    mixed = np.where(rng.random(n) < 0.1, -1, rng.integers(0, 257, size=n)).astype(np.int32)
    mixed[mixed == 100] = 101                                   # id 100 is unused
    cases = {
        "every row unaggregated": (np.full(n, -1, np.int32), 3),
        "one aggregate holding every row": (np.zeros(n, np.int32), 1),
        "aggregates of one row": (rng.permutation(n).astype(np.int32), n),
        "257 aggregates, some rows outside, id 100 unused": (mixed, 257),
        "n = 1": (np.zeros(1, np.int32), 1),
        "n = 1 outside": (np.full(1, -1, np.int32), 0),
    }
    got = {}
    for what, (agg, na) in cases.items():
        b = B[:len(agg)]
        got[what] = device_fit(cmi, torch_cuda, agg, b, na)
        check_fit(got[what], R.fit(agg, b, na), what)
    assert got["n = 1 outside"][0].tolist() == [0, 0] and got["every row unaggregated"][3].tolist() == [0, 0, 0]
    Rr = got["257 aggregates, some rows outside, id 100 unused"][3]
    assert Rr[100] == 0 and np.array_equal(Rr == 0, np.bincount(mixed[mixed >= 0], minlength=257) == 0)   # R = 0 exactly where no row uses the id
    empty = device_fit(cmi, torch_cuda, np.zeros(0, np.int32), np.zeros(0, dtype), 4)
    assert empty[0].tolist() == [0] and empty[3].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("dtype", DT)
def test_fit_sums_in_ascending_row_order(cmi, torch_cuda, dtype):
    agg, B = R.binade_deck(dtype)
    want = R.fit(agg, B, 1)
    check_fit(device_fit(cmi, torch_cuda, agg, B, 1), want, "binade deck")
    assert want[3][0] != R.fit(agg, B, 1, mutant="rows_descending")[3][0]
    # the same values dealt to three aggregates and to no aggregate, interleaved
    ids = (np.arange(len(B)) % 4 - 1).astype(np.int32)
    check_fit(device_fit(cmi, torch_cuda, ids, B, 3), R.fit(ids, B, 3), "binade deck, interleaved")


def test_fit_refuses_ids_out_of_range(cmi, torch_cuda):
    torch = torch_cuda
    B = np.ones(300)
    for bad in (5, -2, 2**31 - 1):
        agg = (np.arange(300) % 5).astype(np.int32)
        agg[211] = bad
        with pytest.raises(cmi.CmiError) as err:
            cmi.aggregates_fit(dev(agg, torch), dev(B, torch), 5)
        assert err.value.status == INVALID and "aggregate id" in str(err.value)
    # nothing is written by a refused call
    L = cmi.lib()
    Tp = torch.full((301,), -7, dtype=torch.int32, device="cuda")
    Tj = torch.full((300,), -7, dtype=torch.int32, device="cuda")
    Tx = torch.full((300,), -7.0, dtype=torch.float64, device="cuda")
    Rr = torch.full((5,), -7.0, dtype=torch.float64, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert L.cmi_aggregates_fit_f64(300, 5, vp(dev(agg, torch)), vp(dev(B, torch)), vp(Tp), vp(Tj), vp(Tx), 300, vp(Rr), None) == INVALID
    torch.cuda.synchronize()
    assert (Tp == -7).all() and (Tj == -7).all() and (Tx == -7).all() and (Rr == -7).all()


# ---- (d) elementwise ------------------------------------------------------------------------------------------------------
def device_elementwise(cmi, torch, m, n, A, B, op):
    got = cmi.csr_elementwise(m, n, *(dev(a, torch) for a in A), *(dev(b, torch) for b in B), op=op)
    return None if got is None else host(got)


def compare_elementwise(cmi, torch, m, n, A, B, what):
    out = {}
    for op in ("add", "subtract"):
        got = device_elementwise(cmi, torch, m, n, A, B, op)
        assert got is not None, f"{what}: reported as unsorted"
        check_csr(got, R.elementwise(m, n, *A, *B, op), f"{what}, {op}")
        rows = R.csr_rows(got[0])
        assert np.all((rows[1:] != rows[:-1]) | (got[1][1:] > got[1][:-1])), f"{what}: columns not strictly ascending"
        out[op] = got
    return out


@pytest.mark.parametrize("dtype", DT)
def test_elementwise_patterns(cmi, torch_cuda, dtype):
    rng = np.random.default_rng(15)
    m, n = 300, 42
    A = R.random_sorted_csr(rng, m, n, 0.2, dtype, duplicates=False)
    B = R.random_sorted_csr(rng, m, n, 0.2, dtype, duplicates=False)
    compare_elementwise(cmi, torch_cuda, m, n, A, B, "overlapping")
    # disjoint: A moved to even columns, B to odd ones (rounding down may repeat a column: still sorted)
    even, odd = (A[0], A[1] // 2 * 2, A[2]), (B[0], B[1] // 2 * 2 + 1, B[2])
    out = compare_elementwise(cmi, torch_cuda, m, n, even, odd, "disjoint")
    assert np.array_equal(np.diff(out["add"][0]), np.diff(out["subtract"][0]))
    # identical: A + A doubles, A - A drops everything
    out = compare_elementwise(cmi, torch_cuda, m, n, A, A, "identical")
    same_bits(out["add"][2], (A[2] * 2)[A[2] != 0], "A + A")
    assert not out["subtract"][0].any() and len(out["subtract"][1]) == 0
    # nested: B holds every other entry of A
    keep = np.arange(len(A[1])) % 2 == 0
    rows = R.csr_rows(A[0])
    Bp = np.zeros(m + 1, np.int64)
    np.add.at(Bp, rows[keep] + 1, 1)
    nested = (np.cumsum(Bp).astype(np.int32), A[1][keep], rng.standard_normal(int(keep.sum())).astype(dtype))
    compare_elementwise(cmi, torch_cuda, m, n, A, nested, "nested")
    compare_elementwise(cmi, torch_cuda, m, n, nested, A, "nested, swapped")
    # an empty operand, both ways; a matrix without rows
    Z = (np.zeros(m + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, dtype))
    out = compare_elementwise(cmi, torch_cuda, m, n, A, Z, "A and nothing")
    out = compare_elementwise(cmi, torch_cuda, m, n, Z, A, "nothing and A")
    same_bits(out["subtract"][2], (-A[2])[A[2] != 0], "0 - A")
    out = compare_elementwise(cmi, torch_cuda, 0, n, (Z[0][:1], Z[1], Z[2]), (Z[0][:1], Z[1], Z[2]), "no rows")
    assert out["add"][0].tolist() == [0]


@pytest.mark.parametrize("dtype", DT)
def test_elementwise_order_zeros_and_duplicates(cmi, torch_cuda, dtype):
    big = dtype(2.0) ** (53 if dtype == np.float64 else 24)
    # (0,0): (big + 1) + 1 = big, B after A;  (0,1): -0.0 + 0.0 dropped;  (0,2): NaN kept;  (0,3): 1 - 1 dropped under subtract;
    # (1,*): duplicated columns in each operand, chains of three and four
    A = SR.csr([[(0, big), (1, -0.0), (2, np.nan), (3, 1.0)], [(0, 0.1), (0, 0.2), (2, big), (2, 1.0)]], dtype)
    B = SR.csr([[(0, 1.0), (0, 1.0), (1, 0.0), (3, 1.0)], [(0, 0.3), (2, 1.0), (2, -big)]], dtype)
    out = compare_elementwise(cmi, torch_cuda, 2, 4, A, B, "order deck")
    assert out["add"][2][0] == big and out["add"][1].tolist()[:3] == [0, 2, 3] and np.isnan(out["add"][2][1])
    assert out["subtract"][1].tolist()[:2] == [0, 2]
    bad = R.elementwise(2, 4, *A, *B, "add", mutant="b_before_a")
    assert bad[2][0] == big + 2 and bad[2][0] != out["add"][2][0]   # 1 + 1 + big: B's values before A's


def test_elementwise_reports_unsorted_operands_and_writes_nothing(cmi, torch_cuda):
    torch = torch_cuda
    L = cmi.lib()
    good = SR.csr([[(0, 1.0), (2, 2.0)], [(1, 3.0)]], np.float64)
    cases = {
        "columns descending in a row of B": (good, SR.csr([[(2, 1.0), (0, 2.0)], [(1, 3.0)]], np.float64)),
        "columns descending in a row of A": (SR.csr([[(0, 1.0)], [(2, 1.0), (1, 3.0)]], np.float64), good),
        "a column outside the matrix": (good, SR.csr([[(0, 1.0), (3, 2.0)], [(1, 3.0)]], np.float64)),
        "offsets that decrease": (good, (np.array([0, 2, 1], np.int32), good[1][:1].copy(), good[2][:1].copy())),
    }
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for what, (A, B) in cases.items():
        assert device_elementwise(cmi, torch, 2, 3, A, B, "add") is None, what
        d = [dev(a, torch) for a in (*A, *B)]
        cap = len(A[1]) + len(B[1])
        Cp = torch.full((3,), -7, dtype=torch.int32, device="cuda")
        Cj = torch.full((cap,), -7, dtype=torch.int32, device="cuda")
        Cx = torch.full((cap,), -7.0, dtype=torch.float64, device="cuda")
        ok = ctypes.c_int(5)
        cmi.check(L.cmi_csr_elementwise_f64(2, 3, len(A[1]), vp(d[0]), vp(d[1]), vp(d[2]), len(B[1]), vp(d[3]), vp(d[4]), vp(d[5]), 1, vp(Cp), vp(Cj), vp(Cx),
                                            cap, ctypes.byref(ok), None))
        torch.cuda.synchronize()
        assert ok.value == 0 and (Cp == -7).all() and (Cj == -7).all() and (Cx == -7).all(), what


@pytest.mark.parametrize("dtype", DT)
def test_elementwise_2049_rows(cmi, torch_cuda, dtype):
    rng = np.random.default_rng(16)
    m, n = 2049, 77
    compare_elementwise(cmi, torch_cuda, m, n, R.random_sorted_csr(rng, m, n, 0.05, dtype), R.random_sorted_csr(rng, m, n, 0.05, dtype), "2049 rows")


# ---- refusals and memory --------------------------------------------------------------------------------------------------
def test_refusals_before_any_device_call(cmi, torch_cuda):
    torch = torch_cuda
    L = cmi.lib()
    t = torch.zeros(8, dtype=torch.int32, device="cuda")
    v = torch.zeros(8, dtype=torch.float64, device="cuda")
    p, q, N = ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(v.data_ptr()), None
    ok = ctypes.c_int(0)
    bad = {
        "strength: negative": lambda: L.cmi_csr_strength_symmetric_f64(-1, -1, 0, p, p, q, 0.0, p, p, q, 0, N),
        "strength: not square": lambda: L.cmi_csr_strength_symmetric_f64(2, 3, 1, p, p, q, 0.0, p, p, q, 1, N),
        "strength: capacity": lambda: L.cmi_csr_strength_symmetric_f64(2, 2, 3, p, p, q, 0.0, p, p, q, 2, N),
        "strength: ceiling": lambda: L.cmi_csr_strength_symmetric_f64(2, 2, CEILING + 1, p, p, q, 0.0, p, p, q, CEILING + 1, N),
        "strength: null": lambda: L.cmi_csr_strength_symmetric_f64(2, 2, 3, p, N, q, 0.0, p, p, q, 3, N),
        "scale_rows: negative": lambda: L.cmi_csr_scale_rows_f64(2, -1, p, q, q, 1.0, q, N),
        "scale_rows: ceiling": lambda: L.cmi_csr_scale_rows_f64(2**31, 1, p, q, q, 1.0, q, N),
        "scale_rows: null": lambda: L.cmi_csr_scale_rows_f64(2, 3, p, q, N, 1.0, q, N),
        "fit: negative": lambda: L.cmi_aggregates_fit_f64(-1, 1, p, q, p, p, q, 0, q, N),
        "fit: capacity": lambda: L.cmi_aggregates_fit_f64(4, 2, p, q, p, p, q, 3, q, N),
        "fit: ceiling": lambda: L.cmi_aggregates_fit_f64(CEILING + 1, 2, p, q, p, p, q, CEILING + 1, q, N),
        "fit: null": lambda: L.cmi_aggregates_fit_f64(4, 2, p, q, p, p, q, 4, N, N),
        "elementwise: negative": lambda: L.cmi_csr_elementwise_f64(2, 2, -1, p, p, q, 0, p, p, q, 0, p, p, q, 0, ctypes.byref(ok), N),
        "elementwise: capacity": lambda: L.cmi_csr_elementwise_f64(2, 2, 2, p, p, q, 2, p, p, q, 0, p, p, q, 3, ctypes.byref(ok), N),
        "elementwise: ceiling": lambda: L.cmi_csr_elementwise_f64(2, 2, CEILING, p, p, q, 1, p, p, q, 0, p, p, q, CEILING + 1, ctypes.byref(ok), N),
        "elementwise: op": lambda: L.cmi_csr_elementwise_f64(2, 2, 2, p, p, q, 2, p, p, q, 2, p, p, q, 4, ctypes.byref(ok), N),
        "elementwise: null flag": lambda: L.cmi_csr_elementwise_f64(2, 2, 2, p, p, q, 2, p, p, q, 0, p, p, q, 4, N, N),
        "presmooth: negative": lambda: L.cmi_relax_jacobi_presmooth_f64(-1, q, q, 1.0, q, N),
        "presmooth: null": lambda: L.cmi_relax_jacobi_presmooth_f64(3, q, N, 1.0, q, N),
    }
    for what, call in bad.items():
        assert call() == INVALID, what
        assert L.cmi_last_error(), what
    for name in ("csr_strength_symmetric", "csr_scale_rows", "aggregates_fit", "csr_elementwise", "relax_jacobi_presmooth"):
        for suf in ("f64", "f32"):
            assert hasattr(L, f"cmi_{name}_{suf}")


def test_device_memory_returns_after_every_call(cmi, torch_cuda):
    torch = torch_cuda
    N, Ap, Aj, Ax = SR.poisson5pt(60, 60, np.float64)
    d = [dev(a, torch) for a in (Ap, Aj, Ax)]
    agg = dev((np.arange(N) % 400 - 1).astype(np.int32), torch)
    bad = agg.clone()
    bad[5] = 999
    B = dev(np.ones(N), torch)
    unsorted = dev(Aj[::-1].copy(), torch)
    diag, x = dev(np.full(N, 4.0), torch), dev(np.zeros(N), torch)

    def refused():
        with pytest.raises(cmi.CmiError):
            cmi.aggregates_fit(bad, B, 399)

    for call in (lambda: cmi.csr_strength_symmetric(N, *d, 0.25),
                 lambda: cmi.aggregates_fit(agg, B, 399),
                 refused,
                 lambda: cmi.csr_elementwise(N, N, *d, *d, op="subtract"),
                 lambda: cmi.csr_elementwise(N, N, *d, d[0], unsorted, d[2], op="add"),
                 lambda: cmi.csr_scale_rows(N, d[0], d[2], diag, 0.7, out=d[2]),
                 lambda: cmi.relax_jacobi_presmooth(diag, B, 0.7, x)):
        assert_memory_returns(cmi, torch, call)


# ---- the header layer on device_memory --------------------------------------------------------------------------------------
def test_amg_device_layer_program(cmi, torch_cuda, tmp_path):
    """tests/amg/test_amg_device.cpp, once, in a child process under its own time limit: the device hierarchy against the host
    hierarchy of the same program (components bit for bit with the host's rho), the coarse operators against R (A P) recomputed
    on the host, the conditions on cg's iteration counts, COO and ELL input, the one-level case."""
    import os
    import subprocess
    from conftest import ROOT
    inc, libd = os.path.join(ROOT, "cusp-autotuned_amd", "include"), os.path.join(ROOT, "cusp-autotuned_amd", "lib")
    exe = tmp_path / "test_amg_device"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fopenmp", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off",
                        f"-I{inc}", f"-I{os.path.join(ROOT, 'tests', 'cpp')}", os.path.join(ROOT, "tests", "amg", "test_amg_device.cpp"),
                        "-o", str(exe), f"-L{libd}", "-lcusp_mi355x", f"-Wl,-rpath,{libd}", "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run(["timeout", "-k", "10", "300", str(exe)], capture_output=True, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "13 tests, 0 failed" in r.stdout


# ---- hypothesis -----------------------------------------------------------------------------------------------------------
from hypothesis import HealthCheck, given, settings, strategies as st  # noqa: E402

SETTINGS = dict(max_examples=40, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))


@settings(**SETTINGS)
@given(m=st.integers(0, 70), n=st.integers(1, 40), da=st.floats(0, 0.6), db=st.floats(0, 0.6), f32=st.booleans(), dup=st.booleans(),
       seed=st.integers(0, 2**31 - 1))
def test_drawn_pairs(cmi, torch_cuda, m, n, da, db, f32, dup, seed):
    dtype = np.float32 if f32 else np.float64
    rng = np.random.default_rng(seed)
    A, B = R.random_sorted_csr(rng, m, n, da, dtype, duplicates=dup), R.random_sorted_csr(rng, m, n, db, dtype, duplicates=dup)
    compare_elementwise(cmi, torch_cuda, m, n, A, B, f"m={m} n={n} seed={seed}")
