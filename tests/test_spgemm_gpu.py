"""CSR x CSR (SpGEMM, cmi_spgemm_csr_* / cmi.spgemm) on the MI355X against tests/spgemm_refs.py: structure exactly, values
bit for bit (special_values.same_bits: -0.0 is not +0.0, a NaN is a NaN), f64 and f32.  No tolerance anywhere.

The workspace W and the tile size T are read from cmi_spgemm_limits; small slabs are forced with cmi_spgemm_set_workspace
and reset in a `finally`.  This build ships the slab path alone (T == 0, cmi_spgemm_info reports 0 rows in tiles), so
the tile-boundary cases of the LDS path are not here.
"""
import ctypes
import glob
import os

import numpy as np
import pytest

import spgemm_refs as R
import special_values as SV
from conftest import GOLDEN, coo_to_csr, read_mtx
from special_values import same_bits

pytestmark = pytest.mark.gpu
DT = [np.float64, np.float32]
NOT_SUPPORTED, INVALID = 3, 1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch


def dev(a, torch):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_product(cmi, torch, deck):
    m, k, n, Ap, Aj, Ax, Bp, Bj, Bx = deck
    Cp, Cj, Cx, info = cmi.spgemm_csr(m, k, n, *(dev(a, torch) for a in (Ap, Aj, Ax, Bp, Bj, Bx)))
    return (Cp.cpu().numpy(), Cj.cpu().numpy(), Cx.cpu().numpy()), info


def check_csr(got, want, m, what):
    Cp, Cj, Cx = got
    assert Cp[0] == 0 and Cp[m] == len(Cj) == len(Cx), what
    assert np.array_equal(Cp, want[0]), f"{what}: row offsets differ"
    assert np.array_equal(Cj, want[1]), f"{what}: column indices differ"
    same_bits(Cx, want[2], what)
    rows = np.repeat(np.arange(m), np.diff(Cp))
    inner = rows[1:] == rows[:-1]
    assert np.all(Cj[1:][inner] > Cj[:-1][inner]), f"{what}: columns not strictly ascending"


def compare(cmi, torch, deck, what):
    got, info = device_product(cmi, torch, deck)
    check_csr(got, R.spgemm(*deck), deck[0], what)
    assert info["rows_in_tiles"] == 0
    return got, info


def mtx_csr(path, dtype):
    rows, cols, I, J, V = read_mtx(path)
    return (rows, cols, *coo_to_csr(rows, I, J, V, dtype))


def pair(A, B):
    assert A[1] == B[0]
    return (A[0], A[1], B[1], *A[2:], *B[2:])


# ---- fixtures ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
def test_fixture_products(cmi, torch_cuda, dtype):
    five = mtx_csr(os.path.join(GOLDEN, "5pt_10x10.mtx"), dtype)
    nine = mtx_csr(os.path.join(GOLDEN, "ref_data", "laplacian", "9pt_10x10.mtx"), dtype)
    compare(cmi, torch_cuda, pair(five, five), "5pt_10x10 squared")
    compare(cmi, torch_cuda, pair(nine, five), "9pt_10x10 x 5pt_10x10")
    rng = np.random.default_rng(75)
    compare(cmi, torch_cuda, R.random_pair(rng, 7, 5, 9, 0.5, 0.5, dtype, duplicates=False), "7x5 . 5x9")


@pytest.mark.parametrize("dtype", DT)
def test_every_pair_of_random_10x10(cmi, torch_cuda, dtype):
    files = sorted(glob.glob(os.path.join(GOLDEN, "ref_data", "random_10x10", "*.mtx")))
    assert len(files) >= 10
    mats = [mtx_csr(f, dtype) for f in files]
    for fa, A in zip(files, mats):
        for fb, B in zip(files, mats):
            compare(cmi, torch_cuda, pair(A, B), f"{os.path.basename(fa)} x {os.path.basename(fb)}")


@pytest.mark.parametrize("dtype", DT)
def test_irregular_times_its_transpose(cmi, torch_cuda, golden_irregular, dtype):
    p = "f64" if dtype == np.float64 else "f32"
    rows, cols = int(golden_irregular["rows"]), int(golden_irregular["cols"])
    A = (rows, cols, golden_irregular[p + "_Ap"], golden_irregular[p + "_Aj"], golden_irregular[p + "_Ax"])
    At = (cols, rows, *R.transpose(*A))
    compare(cmi, torch_cuda, pair(A, At), "irregular x irregular^T")


@pytest.mark.parametrize("dtype", DT)
def test_galerkin_product_on_poisson_100x100(cmi, torch_cuda, dtype):
    N, Ap, Aj, Ax = R.poisson5pt(100, 100, dtype)
    rng = np.random.default_rng(5)
    Ax = (Ax * (1 + rng.random(len(Ax)))).astype(dtype)       # not symmetric in its values: the order of every chain matters
    A = (N, N, Ap, Aj, Ax)
    P = (N, N // 4, *R.aggregation_2x2(100, 100, dtype))
    Pt = (N // 4, N, *R.transpose(*P))
    AP_got, _ = compare(cmi, torch_cuda, pair(A, P), "A P")
    AP = (N, N // 4, *AP_got)
    got, info = compare(cmi, torch_cuda, pair(Pt, AP), "P^T (A P)")
    assert len(got[1]) == 2500 * 5 - 4 * 50 and info["products"] == len(AP_got[1])


# ---- degenerate -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
def test_degenerate_operands(cmi, torch_cuda, dtype):
    z = lambda n: np.zeros(n, np.int32)  # noqa: E731
    e, ev = np.zeros(0, np.int32), np.zeros(0, dtype)
    B = R.csr([[(0, 1.0), (2, 2.0)], [], [(1, 3.0)]], dtype)
    for what, deck in {
        "m = 0": (0, 3, 3, z(1), e, ev, *B),
        "nnz(A) = 0": (4, 3, 3, z(5), e, ev, *B),
        "nnz(B) = 0": (2, 3, 3, *R.csr([[(0, 1.0)], [(2, 1.0)]], dtype), z(4), e, ev),
        "A points at empty rows of B only": (2, 3, 3, *R.csr([[(1, 1.0), (1, 2.0)], [(1, 3.0)]], dtype), *B),
        "one row, one product": (1, 1, 1, *R.csr([[(0, 3.0)]], dtype), *R.csr([[(0, 0.5)]], dtype)),
    }.items():
        got, info = compare(cmi, torch_cuda, deck, what)
        if what != "one row, one product":
            assert info["products"] == 0 and len(got[1]) == 0 and not got[0].any(), what
        else:
            assert info["products"] == 1 and info["slabs"] == 1 and got[2][0] == 1.5


# ---- order, duplicates, unsorted input, special values -------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
def test_contract_decks(cmi, torch_cuda, dtype):
    D = R.decks(dtype)
    got = {name: compare(cmi, torch_cuda, deck, name)[0] for name, deck in D.items()}
    assert got["minus_zero"][2].tolist() == [0.0, 0.0] and not np.signbit(got["minus_zero"][2]).any()   # a lone -0.0 product comes out +0.0
    assert got["cancel"][1].tolist() == [0, 1, 0, 1] and got["cancel"][2][0] == 0                       # an exact cancellation is a kept entry
    assert got["fma"][2][0] == 0
    assert np.isnan(got["inf_nan"][2][0])                                                             # Inf * 0


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("deck", SV.DECKS)
def test_special_value_decks_as_values_of_a_and_b(cmi, torch_cuda, dtype, deck):
    M = SV.matrices(dtype)["poisson100"]
    Ax, x, _ = SV.decks(M, dtype)[deck]
    Ap, Aj = M.Ap.astype(np.int32), M.Aj.astype(np.int32)
    compare(cmi, torch_cuda, (M.rows, M.cols, M.cols, Ap, Aj, Ax, Ap, Aj, x[M.Aj].astype(dtype)), deck)


# ---- slabs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
def test_slab_boundaries(cmi, torch_cuda, dtype):
    N, Ap, Aj, Ax = R.poisson5pt(20, 20, dtype)
    rng = np.random.default_rng(6)
    Ax = (Ax * (1 + rng.random(len(Ax)))).astype(dtype)
    deck = (N, N, N, Ap, Aj, Ax, Ap, Aj, Ax)
    one, info = compare(cmi, torch_cuda, deck, "one slab")
    assert info["slabs"] == 1 and 9000 <= info["products"] <= 10000
    try:
        cmi.spgemm_set_workspace(1000)
        T, W = cmi.spgemm_limits()
        assert W == 1000 and T == 0
        many, info = compare(cmi, torch_cuda, deck, "slabs of 1000 products")
        assert info["slabs"] >= 3 and info["rows_in_slabs"] == N
        assert all(np.array_equal(a, b) for a, b in zip(one[:2], many[:2]))
        same_bits(many[2], one[2], "sliced against one slab")
        # a single row with exactly W products is accepted, one with W + 1 refused
        a = R.csr([[(0, 2.0)]], dtype)
        for width in (W, W + 1):
            b = (np.array([0, width], np.int32), np.arange(width, dtype=np.int32)[::-1].copy(), rng.standard_normal(width).astype(dtype))
            d = (1, 1, width, *a, *b)
            if width == W:
                _, info = compare(cmi, torch_cuda, d, "a row of exactly W products")
                assert info["slabs"] == 1 and info["products"] == W
            else:
                with pytest.raises(cmi.CmiError) as err:
                    device_product(cmi, torch_cuda, d)
                assert err.value.status == NOT_SUPPORTED and str(W + 1) in str(err.value) and "row 0" in str(err.value)
    finally:
        cmi.spgemm_set_workspace(0)
    assert cmi.spgemm_limits()[1] != 1000


def test_product_counts_are_64_bit(cmi, torch_cuda):
    n = 70000
    A = (np.array([0, n], np.int32), np.zeros(n, np.int32), np.ones(n, np.float32))
    B = (np.array([0, n], np.int32), np.arange(n, dtype=np.int32), np.ones(n, np.float32))
    with pytest.raises(cmi.CmiError) as err:
        device_product(cmi, torch_cuda, (1, 1, n, *A, *B))
    assert err.value.status == NOT_SUPPORTED and "4900000000" in str(err.value)


# ---- the handle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
def test_take_respects_capacity_and_guards(cmi, torch_cuda, dtype):
    torch = torch_cuda
    suf = "f64" if dtype == np.float64 else "f32"
    L = cmi.lib()
    rng = np.random.default_rng(9)
    deck = R.random_pair(rng, 33, 29, 31, 0.2, 0.2, dtype)
    m = deck[0]
    want = R.spgemm(*deck)
    d = [dev(a, torch) for a in deck[3:]]
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    h = ctypes.c_void_p()
    cmi.check(getattr(L, "cmi_spgemm_csr_" + suf)(m, deck[1], deck[2], len(deck[4]), vp(d[0]), vp(d[1]), vp(d[2]), len(deck[7]), vp(d[3]), vp(d[4]), vp(d[5]),
                                                 ctypes.byref(h), None))
    try:
        nnz = ctypes.c_int64(-1)
        cmi.check(L.cmi_spgemm_num_entries(h, ctypes.byref(nnz)))
        nnz = nnz.value
        assert nnz == len(want[1]) > 0
        G = 16
        Cp = torch.full((m + 1 + 2 * G,), -7, dtype=torch.int32, device="cuda")
        Cj = torch.full((nnz + 2 * G,), -7, dtype=torch.int32, device="cuda")
        Cx = torch.full((nnz + 2 * G,), -7.0, dtype=d[2].dtype, device="cuda")
        take = getattr(L, "cmi_spgemm_take_" + suf)
        inner = lambda t: ctypes.c_void_p(t.data_ptr() + G * t.element_size())  # noqa: E731
        assert take(h, inner(Cp), inner(Cj), inner(Cx), nnz - 1, None) == INVALID and b"capacity" in L.cmi_last_error()
        other = getattr(L, "cmi_spgemm_take_" + ("f32" if suf == "f64" else "f64"))
        assert other(h, inner(Cp), inner(Cj), inner(Cx), nnz, None) == INVALID
        torch.cuda.synchronize()
        assert (Cp == -7).all() and (Cj == -7).all() and (Cx == -7).all()          # a refused take writes nothing
        for _ in range(2):                                                           # take may be called several times
            cmi.check(take(h, inner(Cp), inner(Cj), inner(Cx), nnz, None))
            torch.cuda.synchronize()
            for t in (Cp, Cj, Cx):
                assert (t[:G] == -7).all() and (t[-G:] == -7).all()
            check_csr((Cp[G:-G].cpu().numpy(), Cj[G:-G].cpu().numpy(), Cx[G:-G].cpu().numpy()), want, m, "take")
    finally:
        cmi.check(L.cmi_spgemm_destroy(h))


def test_device_memory_returns_after_destroy_and_after_a_refusal(cmi, torch_cuda):
    torch = torch_cuda
    L = cmi.lib()
    N, Ap, Aj, Ax = R.poisson5pt(60, 60, np.float64)
    deck = (N, N, N, Ap, Aj, Ax, Ap, Aj, Ax)
    tiny = (1, 1, 1, *R.csr([[(0, 3.0)]], np.float64), *R.csr([[(0, 0.5)]], np.float64))
    d, t = [dev(a, torch) for a in deck[3:]], [dev(a, torch) for a in tiny[3:]]
    free = lambda: (torch.cuda.synchronize(), torch.cuda.mem_get_info()[0])[1]  # noqa: E731

    def round_trip(dk, arrays, expect=0):
        h = ctypes.c_void_p()
        vp = [ctypes.c_void_p(a.data_ptr()) for a in arrays]
        st = L.cmi_spgemm_csr_f64(dk[0], dk[1], dk[2], len(dk[4]), vp[0], vp[1], vp[2], len(dk[7]), vp[3], vp[4], vp[5], ctypes.byref(h), None)
        assert st == expect, L.cmi_last_error()
        assert (h.value is None) == (expect != 0)
        cmi.check(L.cmi_spgemm_destroy(h))

    round_trip(deck, d)                  # warm-up: code objects and the runtime's own pools are in place after this
    # the allocator's granularity: what one byte costs while it is held, and what a one-product round leaves behind
    before = free()
    p = ctypes.c_void_p()
    cmi.check(L.cmi_malloc(ctypes.byref(p), 1))
    held = free()
    cmi.check(L.cmi_free(p))
    round_trip(tiny, t)
    slack = max(before - held, abs(before - free()))
    print(f"allocator slack measured: {slack} bytes")
    base = free()
    round_trip(deck, d)
    assert abs(free() - base) <= slack, "scratch or result still held after destroy"
    try:
        cmi.spgemm_set_workspace(3)      # a row of the stencil squared holds more than 3 products: refused after the counting pass
        round_trip(deck, d, expect=NOT_SUPPORTED)
    finally:
        cmi.spgemm_set_workspace(0)
    assert abs(free() - base) <= slack, "scratch still held after a refused call"


def test_python_spgemm_takes_host_and_coo_operands(cmi, torch_cuda):
    torch = torch_cuda
    deck = R.random_pair(np.random.default_rng(21), 17, 13, 19, 0.3, 0.3, np.float64)
    m, k, n, Ap, Aj, Ax, Bp, Bj, Bx = deck
    want = R.spgemm(*deck)
    hA = cmi.CsrMatrix(m, k, len(Aj), *(torch.from_numpy(a) for a in (Ap, Aj, Ax)))
    hB = cmi.CsrMatrix(k, n, len(Bj), *(torch.from_numpy(a) for a in (Bp, Bj, Bx)))
    C = cmi.spgemm(hA, hB)
    assert not C.values.is_cuda and (C.num_rows, C.num_cols, C.num_entries) == (m, n, len(want[1])) and C.info["products"] > 0
    check_csr((C.row_offsets.numpy(), C.column_indices.numpy(), C.values.numpy()), want, m, "host operands")
    dA = cmi.CsrMatrix(m, k, len(Aj), *(dev(a, torch) for a in (Ap, Aj, Ax)))
    dB = cmi.CsrMatrix(k, n, len(Bj), *(dev(a, torch) for a in (Bp, Bj, Bx)))
    C = cmi.spgemm(cmi.convert(dA, "coo"), dB)
    assert C.values.is_cuda
    check_csr((C.row_offsets.cpu().numpy(), C.column_indices.cpu().numpy(), C.values.cpu().numpy()), want, m, "COO operand")
    with pytest.raises(ValueError):
        cmi.spgemm(dA, dA)
    with pytest.raises(TypeError):
        cmi.spgemm(cmi.convert(dA, "ell"), dB)


# ---- the header layer on device_memory ------------------------------------------------------------------------------------
def test_spgemm_device_layer_program(cmi, torch_cuda, tmp_path):
    import subprocess
    from conftest import ROOT
    inc, libd = os.path.join(ROOT, "cusp-autotuned_amd", "include"), os.path.join(ROOT, "cusp-autotuned_amd", "lib")
    exe = tmp_path / "test_spgemm_device"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fopenmp", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off",
                        f"-I{inc}", f"-I{os.path.join(ROOT, 'tests', 'cpp')}", os.path.join(ROOT, "tests", "spgemm", "test_spgemm_device.cpp"),
                        "-o", str(exe), f"-L{libd}", "-lcusp_mi355x", f"-Wl,-rpath,{libd}", "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "6 tests, 0 failed" in r.stdout


# ---- hypothesis -------------------------------------------------------------------------------------------------------
hypothesis = pytest.importorskip("hypothesis")
from hypothesis import HealthCheck, given, settings, strategies as st  # noqa: E402

SETTINGS = dict(max_examples=40, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))


@settings(**SETTINGS)
@given(m=st.integers(0, 60), k=st.integers(0, 60), n=st.integers(0, 60), da=st.floats(0, 0.5), db=st.floats(0, 0.5),
       f32=st.booleans(), small_w=st.booleans(), w=st.integers(1, 400), seed=st.integers(0, 2**31 - 1))
def test_drawn_products(cmi, torch_cuda, m, k, n, da, db, f32, small_w, w, seed):
    dtype = np.float32 if f32 else np.float64
    deck = R.random_pair(np.random.default_rng(seed), m, k, n, da, db, dtype)
    want = R.spgemm(*deck)
    if small_w:  # every row must fit: W is drawn, but never below the longest row's product count
        row, _, _ = R.expand(m, deck[3], deck[4], deck[6], deck[7])
        w = max(w, int(np.bincount(row, minlength=1).max()), 1)
    try:
        if small_w:
            cmi.spgemm_set_workspace(w)
        got, info = device_product(cmi, torch_cuda, deck)
    finally:
        cmi.spgemm_set_workspace(0)
    check_csr(got, want, m, f"m={m} k={k} n={n} seed={seed} W={w if small_w else 'default'}")
    if small_w and info["products"]:
        assert info["slabs"] >= -(-info["products"] // w)
