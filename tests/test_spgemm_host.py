"""CPU tests (-m "not gpu") of the sparse x sparse multiply (SpGEMM): the C-ABI symbols and every refusal that must happen
before a device call (host buffers only), the header layer's host_memory cusp::multiply(A, B, C) built from
tests/spgemm/test_spgemm_host.cpp -- once plainly and once as a stand-alone program under the address and undefined-behaviour
sanitizers --, the compile-time refusals, and the host results on the golden fixtures against tests/spgemm_refs.py with
zeros dropped."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import spgemm_refs as R
from conftest import ROOT, GOLDEN, coo_to_csr, read_mtx
from special_values import same_bits

INC = os.path.join(ROOT, "cusp-autotuned_amd", "include")
LIBD = os.path.join(ROOT, "cusp-autotuned_amd", "lib")
SRC = os.path.join(ROOT, "tests", "spgemm")
# the flags of tests/cpp/Makefile
CXXFLAGS = ["-std=c++17", "-O1", "-g", "-fopenmp", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off", f"-I{INC}",
            f"-I{os.path.join(ROOT, 'tests', 'cpp')}", f"-DGOLDEN_DIR=\"{GOLDEN}\""]
LDFLAGS = [f"-L{LIBD}", "-lcusp_mi355x", f"-Wl,-rpath,{LIBD}", "-Wl,-rpath,/opt/rocm/lib"]
INVALID = 1


def test_spgemm_symbols_are_exported(cmi):
    L = cmi.lib()
    for name in ("cmi_spgemm_csr_f64", "cmi_spgemm_csr_f32", "cmi_spgemm_take_f64", "cmi_spgemm_take_f32", "cmi_spgemm_num_entries",
                 "cmi_spgemm_info", "cmi_spgemm_destroy", "cmi_spgemm_limits", "cmi_spgemm_set_workspace"):
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, f"{name} has no prototype in binding.py"
    assert callable(cmi.spgemm) and callable(cmi.spgemm_csr) and callable(cmi.spgemm_limits) and callable(cmi.spgemm_set_workspace)


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_spgemm_argument_validation_without_a_device(cmi, suf):
    L = cmi.lib()
    create, take = getattr(L, f"cmi_spgemm_csr_{suf}"), getattr(L, f"cmi_spgemm_take_{suf}")
    # host buffers only: every call below must be refused (or succeed with nothing to do) before any device call
    buf = (ctypes.c_char * (1 << 16))()
    base = ctypes.addressof(buf)
    Ap, Aj, Ax, Bp, Bj, Bx = (base + 4096 * i for i in range(6))
    h = ctypes.c_void_p()
    ref = ctypes.byref(h)

    def refused(needle, *args):
        h.value = 0xdead
        assert create(*args) == INVALID
        assert needle in L.cmi_last_error(), L.cmi_last_error()
        assert h.value is None or args[-2] is None          # no handle comes back from a refused call

    ok = (4, 5, 6, 3, Ap, Aj, Ax, 2, Bp, Bj, Bx, ref, None)
    for pos in (0, 1, 2, 3, 7):                               # m, k, n, a_entries, b_entries
        bad = list(ok)
        bad[pos] = -1
        refused(b"negative", *bad)
    for pos in (0, 1, 2):                                     # beyond int32
        bad = list(ok)
        bad[pos] = 2**31
        refused(b"exceed", *bad)
    for pos in (3, 7):                                        # beyond the CSR ceiling INT32_MAX - 65536
        bad = list(ok)
        bad[pos] = 2**31 - 65535
        refused(b"exceed", *bad)
    for pos in (4, 5, 6, 8, 9, 10):                           # a null array with a non-zero size
        bad = list(ok)
        bad[pos] = None
        refused(b"null", *bad)
    bad = list(ok)
    bad[11] = None
    refused(b"result is NULL", *bad)

    # nothing to do: success without a device, an empty product whose take refuses a capacity below its size
    for args in ((0, 5, 6, 0, Ap, None, None, 2, Bp, Bj, Bx, ref, None), (4, 5, 6, 0, Ap, None, None, 0, Bp, None, None, ref, None)):
        assert create(*args) == 0, L.cmi_last_error()
        assert h.value
        n, info = ctypes.c_int64(-1), [ctypes.c_int64(-1) for _ in range(4)]
        assert L.cmi_spgemm_num_entries(h, ctypes.byref(n)) == 0 and n.value == 0
        assert L.cmi_spgemm_info(h, *[ctypes.byref(x) for x in info]) == 0 and [x.value for x in info] == [0, 0, 0, 0]
        assert take(h, Ap, None, None, -1, None) == INVALID and b"capacity" in L.cmi_last_error()
        other = getattr(L, "cmi_spgemm_take_" + ("f32" if suf == "f64" else "f64"))
        assert other(h, Ap, None, None, 0, None) == INVALID and b"value type" in L.cmi_last_error()
        assert take(h, None, None, None, 0, None) == INVALID and b"null" in L.cmi_last_error()
        assert L.cmi_spgemm_destroy(h) == 0
    assert L.cmi_spgemm_destroy(None) == 0
    assert L.cmi_spgemm_num_entries(None, None) == INVALID and take(None, Ap, None, None, 0, None) == INVALID
    assert L.cmi_spgemm_info(None, None, None, None, None) == INVALID
    with pytest.raises(cmi.CmiError) as e:
        cmi.check(create(-1, 5, 6, 3, Ap, Aj, Ax, 2, Bp, Bj, Bx, ref, None))
    assert e.value.status == INVALID


def test_spgemm_limits_and_workspace_setter(cmi):
    L = cmi.lib()
    T, W = cmi.spgemm_limits()
    assert T == 0, "this build ships the slab path alone"
    assert 0 < W <= 2**31 - 65536
    try:
        cmi.spgemm_set_workspace(1234)
        assert cmi.spgemm_limits() == (T, 1234)
        assert L.cmi_spgemm_set_workspace(-1) == INVALID and b"workspace" in L.cmi_last_error()
        assert L.cmi_spgemm_set_workspace(2**31) == INVALID
        assert cmi.spgemm_limits() == (T, 1234)
    finally:
        cmi.spgemm_set_workspace(0)
    assert cmi.spgemm_limits() == (T, W)


def test_python_spgemm_refuses_bad_operands(cmi):
    import torch
    z = torch.zeros(3, dtype=torch.int32)
    A = cmi.CsrMatrix(2, 2, 0, z, z[:0], torch.zeros(0, dtype=torch.float64))
    B = cmi.CsrMatrix(3, 2, 0, torch.zeros(4, dtype=torch.int32), z[:0], torch.zeros(0, dtype=torch.float64))
    with pytest.raises(ValueError):
        cmi.spgemm(A, B)                                      # 2 columns against 3 rows
    with pytest.raises(TypeError):
        cmi.spgemm(A, cmi.CsrMatrix(2, 2, 0, z, z[:0], torch.zeros(0, dtype=torch.float32)))
    with pytest.raises(TypeError):
        cmi.spgemm(A, object())


@pytest.fixture(scope="module")
def host_program(cmi, tmp_path_factory):
    exe = tmp_path_factory.mktemp("spgemm") / "test_spgemm_host"
    r = subprocess.run(["g++", *CXXFLAGS, os.path.join(SRC, "test_spgemm_host.cpp"), "-o", str(exe), *LDFLAGS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(exe)


def test_spgemm_host_layer_program(host_program):
    r = subprocess.run([host_program], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "8 tests, 0 failed" in r.stdout


def test_spgemm_host_layer_program_under_sanitizers(cmi, tmp_path):
    # host code with its own main, built stand-alone with the sanitizers: their runtime is linked in, nothing is preloaded
    exe = tmp_path / "test_spgemm_host_san"
    r = subprocess.run(["g++", *CXXFLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(SRC, "test_spgemm_host.cpp"),
                        "-o", str(exe), *LDFLAGS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "8 tests, 0 failed" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def _parse_product(text, dtype):
    lines = text.strip().split("\n")
    m, n, nnz = (int(v) for v in lines[0].split())
    Cp = np.array(lines[1].split(), np.int32)
    ent = [l.split() for l in lines[2:2 + nnz]]
    Cj = np.array([int(e[0]) for e in ent], np.int32)
    bits = np.array([int(e[1], 16) for e in ent], np.uint64)
    Cx = bits.view(np.float64) if dtype == np.float64 else bits.astype(np.uint32).view(np.float32)
    assert len(Cp) == m + 1
    return (m, n), (Cp, Cj, Cx)


GOLDEN_PAIRS = [("5pt_10x10.mtx", "5pt_10x10.mtx"), ("ref_data/laplacian/9pt_10x10.mtx", "5pt_10x10.mtx")] + \
    [(f"ref_data/random_10x10/{a}_nonzeros.mtx", f"ref_data/random_10x10/{b}_nonzeros.mtx")
     for a, b in (("000", "050"), ("050", "000"), ("010", "100"), ("100", "100"), ("030", "080"), ("001", "002"))]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_results_on_golden_fixtures_equal_the_reference_without_zeros(host_program, dtype):
    for fa, fb in GOLDEN_PAIRS:
        pa, pb = os.path.join(GOLDEN, fa), os.path.join(GOLDEN, fb)
        r = subprocess.run([host_program, "--product", "f64" if dtype == np.float64 else "f32", pa, pb], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        ra, ca, I, J, V = read_mtx(pa)
        A = coo_to_csr(ra, I, J, V, dtype)
        rb, cb, I, J, V = read_mtx(pb)
        B = coo_to_csr(rb, I, J, V, dtype)
        want = R.spgemm(ra, ca, cb, *A, *B, drop_zeros=True)
        shape, got = _parse_product(r.stdout, dtype)
        assert shape == (ra, cb), (fa, fb)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (fa, fb)
        same_bits(got[2], want[2], f"{fa} x {fb}")


@pytest.mark.parametrize("snippet,needle", [
    ("cusp::ell_matrix<int, double, cusp::host_memory> A, B, C; cusp::multiply(A, B, C);", "csr x csr -> csr and coo x coo -> coo only"),
    ("cusp::csr_matrix<int, double, cusp::host_memory> A, B; cusp::coo_matrix<int, double, cusp::host_memory> C; cusp::multiply(A, B, C);",
     "with cusp::convert first"),
    ("cusp::hyb_matrix<int, float, cusp::device_memory> A, B, C; cusp::multiply(A, B, C);", "csr x csr -> csr and coo x coo -> coo only"),
    ("cusp::csr_matrix<int, double, cusp::host_memory> A, B; cusp::array1d<double, cusp::host_memory> y(2); cusp::multiply(A, B, y);",
     "B and C must both be sparse matrices"),
])
def test_spgemm_refused_at_compile_time(tmp_path, snippet, needle):
    src = tmp_path / "bad.cpp"
    src.write_text("#include <cusp/coo_matrix.h>\n#include <cusp/csr_matrix.h>\n#include <cusp/ell_matrix.h>\n#include <cusp/hyb_matrix.h>\n"
                   f"#include <cusp/multiply.h>\nint main() {{ {snippet} return 0; }}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode != 0
    assert needle in r.stderr, r.stderr[-2000:]


def test_three_csr_matrices_compile_in_both_spaces(tmp_path):
    src = tmp_path / "good.cpp"
    src.write_text("#include <cusp/coo_matrix.h>\n#include <cusp/csr_matrix.h>\n#include <cusp/multiply.h>\n"
                   "template <typename M> void f() { M A, B, C; cusp::multiply(A, B, C); cusp::multiply(cusp::hip::par, A, B, C);\n"
                   "  typedef typename M::value_type V; cusp::multiply(A, B, C, cusp::constant_functor<V>(V(0)), cusp::multiplies<V>(), cusp::plus<V>()); }\n"
                   "int main() { f<cusp::csr_matrix<int, double, cusp::host_memory>>(); f<cusp::csr_matrix<int, float, cusp::device_memory>>();\n"
                   "  f<cusp::coo_matrix<int, double, cusp::device_memory>>(); f<cusp::coo_matrix<int, float, cusp::host_memory>>(); return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
