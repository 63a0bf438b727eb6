"""CPU tests (-m "not gpu") of cusp::relaxation::gauss_seidel / sor and cusp::graph::vertex_coloring: the C-ABI symbol of the
colour sweep and its argument checks (no device call happens before a bad argument is refused), the header layer on
host_memory built from tests/gauss_seidel/test_gs_host.cpp (plain, and as a stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer), the SOR values that program prints against tests/gauss_seidel_refs.py, and the compile-time
refusal of a matrix that is not CSR."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import gauss_seidel_refs as G
from conftest import ROOT

INC = os.path.join(ROOT, "cusp-autotuned_amd", "include")
LIBD = os.path.join(ROOT, "cusp-autotuned_amd", "lib")
SRC = os.path.join(ROOT, "tests", "gauss_seidel")
# the flags of tests/cpp/Makefile
CXXFLAGS = ["-std=c++17", "-O1", "-g", "-fopenmp", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off", f"-I{INC}",
            f"-I{os.path.join(ROOT, 'tests', 'cpp')}"]
LDFLAGS = [f"-L{LIBD}", "-lcusp_mi355x", f"-Wl,-rpath,{LIBD}", "-Wl,-rpath,/opt/rocm/lib"]
HOST_TESTS = "5 tests, 0 failed"
CSR_CEILING = 2**31 - 1 - 65536
M5 = [[1, 1, 2, 0, 0], [3, 2, 0, 0, 5], [0, 0, 0.5, 0, 0], [0, 6, 7, 4, 0], [0, 8, 0, 0, 8]]


def test_gauss_seidel_symbols_are_exported(cmi):
    L = cmi.lib()
    for suf in ("f64", "f32"):
        assert hasattr(L, f"cmi_csr_gauss_seidel_colour_{suf}")
    assert callable(cmi.csr_gauss_seidel_colour)
    assert cmi.version() == 400   # unchanged: callers find the feature by symbol


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_gauss_seidel_argument_validation_without_a_device(cmi, suf):
    """Host buffers only: every call below is refused (or succeeds with nothing to do) before any device call."""
    L = cmi.lib()
    s = 8 if suf == "f64" else 4
    buf = (ctypes.c_char * (1 << 16))()
    base = ctypes.addressof(buf)
    Ap, Aj, Ax, b, x, order, park = base, base + 1024, base + 2048, base + 8192, base + 16384, base + 24576, base + 32768
    fn = getattr(L, f"cmi_csr_gauss_seidel_colour_{suf}")
    # (rows, nnz, Ap, Aj, Ax, b, x, ordering, slot_begin, slot_end, scratch, stream)
    assert fn(-1, 0, Ap, Aj, Ax, b, x, order, 0, 0, None, None) == 1
    assert b"negative" in L.cmi_last_error()
    assert fn(4, -6, Ap, Aj, Ax, b, x, order, 0, 4, None, None) == 1
    assert b"negative" in L.cmi_last_error()
    assert fn(2**31, 0, Ap, Aj, Ax, b, x, order, 0, 4, None, None) == 1
    assert b"exceed" in L.cmi_last_error()
    assert fn(4, CSR_CEILING + 1, Ap, Aj, Ax, b, x, order, 0, 4, None, None) == 1
    assert b"exceed" in L.cmi_last_error()
    assert fn(2**26, CSR_CEILING, None, None, None, None, None, None, 0, 4, None, None) == 1   # at the ceiling: the arrays
    assert b"null" in L.cmi_last_error()
    for lo, hi in ((-1, 2), (3, 2), (0, 5), (5, 5), (4, 6)):   # reversed, or outside [0, num_rows]
        assert fn(4, 6, Ap, Aj, Ax, b, x, order, lo, hi, None, None) == 1, (lo, hi)
        assert b"slot range" in L.cmi_last_error()
    for hole in range(6):   # each array in turn is null
        a = [Ap, Aj, Ax, b, x, order]
        a[hole] = None
        assert fn(4, 6, *a, 1, 3, None, None) == 1
        assert b"null" in L.cmi_last_error()
    assert fn(4, 6, Ap, Aj, Ax, x, x, order, 0, 4, None, None) == 1                       # b is x
    assert b"b overlaps x" in L.cmi_last_error()
    assert fn(4, 6, Ap, Aj, Ax, x + 3 * s, x, order, 0, 4, None, None) == 1               # b starts in x's last element
    assert fn(4, 6, Ap, Aj, Ax, x - 3 * s, x, order, 0, 4, None, None) == 1               # x starts in b's last element
    assert fn(4, 6, Ap, Aj, Ax, b, x, order, 0, 4, x, None) == 1                          # scratch is x
    assert b"scratch overlaps x" in L.cmi_last_error()
    assert fn(4, 6, Ap, Aj, Ax, b, x, order, 1, 3, x + 3 * s, None) == 1                  # scratch starts in x's last element
    assert fn(4, 6, Ap, Aj, Ax, b, x, order, 1, 3, x - 1 * s, None) == 1                  # its 2 values end in x's first
    assert b"scratch overlaps x" in L.cmi_last_error()
    # an empty range: success, nothing to do -- whatever the arrays
    assert fn(4, 6, None, None, None, None, None, None, 2, 2, None, None) == 0
    assert fn(0, 0, None, None, None, None, None, None, 0, 0, None, None) == 0
    assert fn(4, 6, Ap, Aj, Ax, b, x, order, 4, 4, park, None) == 0
    with pytest.raises(cmi.CmiError) as e:
        cmi.check(fn(4, 6, Ap, Aj, Ax, b, x, order, 3, 2, None, None))
    assert e.value.status == 1


def test_gauss_seidel_python_refuses_host_tensors(cmi):
    import torch
    Ap = torch.zeros(3, dtype=torch.int32)
    v = torch.zeros(2, dtype=torch.float64)
    with pytest.raises(TypeError):
        cmi.csr_gauss_seidel_colour(2, Ap, Ap[:0], v[:0], v, v.clone(), Ap[:2], 0, 2)


def _build(tmp_path, name, extra=()):
    exe = tmp_path / name
    r = subprocess.run(["g++", *CXXFLAGS, *extra, os.path.join(SRC, "test_gs_host.cpp"), "-o", str(exe), *LDFLAGS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def sor_lines_match_the_refs(stdout, space):
    """The program prints one SOR step (omega = 1.5, FORWARD, the reference's 5 x 5 matrix, b = 5, x = -1) per value type as
    hexadecimal floats: the refs module's values, bit for bit."""
    seen = 0
    for line in stdout.splitlines():
        if not line.startswith("SOR5 "):
            continue
        head, vals = line.split(":")
        _, suf, where = head.split()
        assert where == space
        dtype = np.float64 if suf == "f64" else np.float32
        Ap, Aj, Ax = G.from_dense(M5, dtype)
        want = G.Sor(Ap, Aj, Ax, 1.5, G.FORWARD)(np.full(5, 5, dtype), np.full(5, -1, dtype))
        got = np.array([float.fromhex(t) for t in vals.split()], dtype)
        assert got.tobytes() == want.tobytes(), (line, want)
        seen += 1
    assert seen == 2


def test_gauss_seidel_host_layer_program(cmi, tmp_path):
    r = subprocess.run([str(_build(tmp_path, "test_gs_host"))], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert HOST_TESTS in r.stdout
    sor_lines_match_the_refs(r.stdout, "host_memory")


def test_gauss_seidel_host_layer_program_under_sanitizers(cmi, tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined (host code only; leak checking off: the HIP
    runtime the library links keeps process-lifetime allocations)."""
    exe = _build(tmp_path, "test_gs_host_asan", ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"))
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert HOST_TESTS in r.stdout and "runtime error" not in r.stderr


@pytest.mark.parametrize("header", ["gauss_seidel", "sor"])
def test_a_matrix_that_is_not_csr_is_a_compile_time_error(tmp_path, header):
    cls = "gauss_seidel<double, cusp::host_memory> S(A)" if header == "gauss_seidel" else "sor<double, cusp::host_memory> S(A, 1.0)"
    for fmt, ok in (("csr", True), ("ell", False)):
        src = tmp_path / f"{fmt}.cpp"
        src.write_text(f"#include <cusp/csr_matrix.h>\n#include <cusp/ell_matrix.h>\n#include <cusp/relaxation/{header}.h>\n"
                       f"int main() {{ cusp::{fmt}_matrix<int, double, cusp::host_memory> A; cusp::relaxation::{cls}; return 0; }}\n")
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", f"-I{INC}", str(src)], capture_output=True, text=True)
        assert (r.returncode == 0) == ok, r.stderr[-2000:]
        if not ok:
            assert "no matching function" in r.stderr, r.stderr[-2000:]
