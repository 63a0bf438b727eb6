"""CPU tests (-m "not gpu") of cusp::relaxation: the C-ABI symbols of the fused CSR sweeps and their argument checks (no
device call happens before a bad argument is refused), the header layer's host_memory jacobi / polynomial built from
tests/relaxation/test_relax_host.cpp (plain, and as a stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer), and the compile-time refusal of the one-argument polynomial(A)."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT

INC = os.path.join(ROOT, "cusp-autotuned_amd", "include")
LIBD = os.path.join(ROOT, "cusp-autotuned_amd", "lib")
RELAX = os.path.join(ROOT, "tests", "relaxation")
# the flags of tests/cpp/Makefile
CXXFLAGS = ["-std=c++17", "-O1", "-g", "-fopenmp", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off", f"-I{INC}",
            f"-I{os.path.join(ROOT, 'tests', 'cpp')}"]
LDFLAGS = [f"-L{LIBD}", "-lcusp_mi355x", f"-Wl,-rpath,{LIBD}", "-Wl,-rpath,/opt/rocm/lib"]
HOST_TESTS = "43 tests, 0 failed"   # 4 templates x 5 formats x 2 value types + 3
CSR_CEILING = 2**31 - 1 - 65536


def test_relaxation_symbols_are_exported(cmi):
    L = cmi.lib()
    for suf in ("f64", "f32"):
        for name in ("cmi_spmv_csr_axpby", "cmi_csr_jacobi_sweep", "cmi_relax_jacobi_update"):
            assert hasattr(L, f"{name}_{suf}")
    assert callable(cmi.spmv_csr_axpby) and callable(cmi.csr_jacobi_sweep) and callable(cmi.relax_jacobi_update)
    assert cmi.version() == 400   # unchanged: callers find the feature by symbol


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_relaxation_argument_validation_without_a_device(cmi, suf):
    """Host buffers only: every call below is refused (or succeeds with nothing to do) before any device call."""
    L = cmi.lib()
    s = 8 if suf == "f64" else 4
    buf = (ctypes.c_char * (1 << 16))()
    base = ctypes.addressof(buf)
    Ap, Aj, Ax, x, z, out, d = base, base + 1024, base + 2048, base + 8192, base + 16384, base + 24576, base + 32768
    axpby = getattr(L, f"cmi_spmv_csr_axpby_{suf}")
    sweep = getattr(L, f"cmi_csr_jacobi_sweep_{suf}")
    update = getattr(L, f"cmi_relax_jacobi_update_{suf}")

    # ---- axpby form: (plan, rows, cols, nnz, Ap, Aj, Ax, x, alpha, beta, z, out, stream)
    assert axpby(None, -1, 4, 0, Ap, Aj, Ax, x, 1.0, 1.0, z, out, None) == 1
    assert b"negative" in L.cmi_last_error()
    assert axpby(None, 4, -4, 0, Ap, Aj, Ax, x, 1.0, 1.0, z, out, None) == 1
    assert axpby(None, 4, 4, -6, Ap, Aj, Ax, x, 1.0, 1.0, z, out, None) == 1
    assert axpby(None, 2**31, 4, 0, Ap, Aj, Ax, x, 1.0, 1.0, z, out, None) == 1
    assert b"exceed" in L.cmi_last_error()
    assert axpby(None, 4, 4, CSR_CEILING + 1, Ap, Aj, Ax, x, 1.0, 1.0, z, out, None) == 1
    assert b"exceed" in L.cmi_last_error()
    assert axpby(None, 2**26, 2**26, CSR_CEILING, None, None, None, None, 1.0, 1.0, None, None, None) == 1   # at the ceiling: the arrays
    assert b"null" in L.cmi_last_error()
    for hole in range(6):   # each array in turn is null
        a = [Ap, Aj, Ax, x, z, out]
        a[hole] = None
        assert axpby(None, 4, 4, 6, a[0], a[1], a[2], a[3], 1.0, 1.0, a[4], a[5], None) == 1
        assert b"null" in L.cmi_last_error()
    assert axpby(None, 4, 4, 6, Ap, Aj, Ax, x, 1.0, 1.0, z, x, None) == 1                 # out is x
    assert b"overlaps" in L.cmi_last_error()
    assert axpby(None, 4, 6, 6, Ap, Aj, Ax, x, 1.0, 1.0, z, x + 5 * s, None) == 1         # out starts in x's last element
    assert axpby(None, 4, 6, 6, Ap, Aj, Ax, x + 3 * s, 1.0, 1.0, z, x, None) == 1         # x starts in out's last element
    assert axpby(None, 0, 4, 0, None, None, None, None, 1.0, 1.0, None, None, None) == 0  # zero rows: nothing to do

    # ---- Jacobi form: (plan, rows, nnz, Ap, Aj, Ax, diag, b, x, omega, x_out, stream)
    assert sweep(None, -1, 0, Ap, Aj, Ax, d, z, x, 1.0, out, None) == 1
    assert b"negative" in L.cmi_last_error()
    assert sweep(None, 4, -1, Ap, Aj, Ax, d, z, x, 1.0, out, None) == 1
    assert sweep(None, 2**31, 0, Ap, Aj, Ax, d, z, x, 1.0, out, None) == 1
    assert sweep(None, 4, CSR_CEILING + 1, Ap, Aj, Ax, d, z, x, 1.0, out, None) == 1
    assert b"exceed" in L.cmi_last_error()
    for hole in range(7):
        a = [Ap, Aj, Ax, d, z, x, out]
        a[hole] = None
        assert sweep(None, 4, 6, a[0], a[1], a[2], a[3], a[4], a[5], 1.0, a[6], None) == 1
        assert b"null" in L.cmi_last_error()
    assert sweep(None, 4, 6, Ap, Aj, Ax, d, z, x, 1.0, x, None) == 1
    assert b"overlaps" in L.cmi_last_error()
    assert sweep(None, 4, 6, Ap, Aj, Ax, d, z, x, 1.0, x + 3 * s, None) == 1
    assert sweep(None, 4, 6, Ap, Aj, Ax, d, z, x, 1.0, d, None) == 1                       # x_out is diag
    assert b"overlaps diag or b" in L.cmi_last_error()
    assert sweep(None, 4, 6, Ap, Aj, Ax, d, z, x, 1.0, z + 3 * s, None) == 1               # x_out starts in b's last element
    assert b"overlaps diag or b" in L.cmi_last_error()
    assert sweep(None, 0, 0, None, None, None, None, None, None, 1.0, None, None) == 0

    # ---- the elementwise update: (n, diag, b, y, omega, x, stream)
    assert update(-1, d, z, out, 1.0, x, None) == 1
    assert b"negative" in L.cmi_last_error()
    for hole in range(4):
        a = [d, z, out, x]
        a[hole] = None
        assert update(4, a[0], a[1], a[2], 1.0, a[3], None) == 1
        assert b"null" in L.cmi_last_error()
    for hole in range(3):   # x overlapping each input in turn (its last element): refused
        a = [d, z, out]
        a[hole] = x + 3 * s
        assert update(4, a[0], a[1], a[2], 1.0, x, None) == 1
        assert b"overlaps" in L.cmi_last_error()
    assert update(4, x, x, x, 1.0, x, None) == 1
    assert update(0, None, None, None, 1.0, None, None) == 0
    with pytest.raises(cmi.CmiError) as e:
        cmi.check(axpby(None, 4, 4, 6, Ap, Aj, Ax, x, 1.0, 1.0, z, x, None))
    assert e.value.status == 1


def test_relaxation_python_refuses_host_tensors(cmi):
    import torch
    Ap = torch.zeros(3, dtype=torch.int32)
    v = torch.zeros(2, dtype=torch.float64)
    with pytest.raises(TypeError):
        cmi.spmv_csr_axpby(2, 2, Ap, Ap[:0], v[:0], v, 1.0, 1.0, v, v.clone())
    with pytest.raises(TypeError):
        cmi.csr_jacobi_sweep(2, Ap, Ap[:0], v[:0], v, v, v, 1.0, v.clone())
    with pytest.raises(TypeError):
        cmi.relax_jacobi_update(v, v, v, 1.0, v.clone())


def _build(tmp_path, name, extra=()):
    exe = tmp_path / name
    r = subprocess.run(["g++", *CXXFLAGS, *extra, os.path.join(RELAX, "test_relax_host.cpp"), "-o", str(exe), *LDFLAGS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_relaxation_host_layer_program(cmi, tmp_path):
    r = subprocess.run([str(_build(tmp_path, "test_relax_host"))], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert HOST_TESTS in r.stdout


def test_relaxation_host_layer_program_under_sanitizers(cmi, tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined (host code only; leak checking off: the HIP
    runtime the library links keeps process-lifetime allocations)."""
    exe = _build(tmp_path, "test_relax_host_asan", ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"))
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert HOST_TESTS in r.stdout and "runtime error" not in r.stderr


def test_one_argument_polynomial_is_a_compile_time_error(tmp_path):
    src = tmp_path / "bad.cpp"
    src.write_text("#include <cusp/csr_matrix.h>\n#include <cusp/relaxation/polynomial.h>\n"
                   "int main() { cusp::csr_matrix<int, double, cusp::host_memory> A(2, 2, 0);"
                   " cusp::relaxation::polynomial<double, cusp::host_memory> P(A); return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode != 0
    assert "no matching function" in r.stderr, r.stderr[-2000:]
