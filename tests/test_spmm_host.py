"""CPU tests (-m "not gpu") of the CSR x dense-block multiply (SpMM): the C-ABI symbols and their argument checks (no
device call happens before a bad argument is refused), and the header layer's host_memory cusp::multiply(A, X, Y) built
from tests/spmm/test_spmm_host.cpp -- plus the compile-time refusal of other formats and of mixed arguments."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, GOLDEN

INC = os.path.join(ROOT, "cusp-autotuned_amd", "include")
LIBD = os.path.join(ROOT, "cusp-autotuned_amd", "lib")
SPMM = os.path.join(ROOT, "tests", "spmm")
# the flags of tests/cpp/Makefile
CXXFLAGS = ["-std=c++17", "-O1", "-g", "-fopenmp", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off", f"-I{INC}",
            f"-I{os.path.join(ROOT, 'tests', 'cpp')}", f"-DGOLDEN_DIR=\"{GOLDEN}\""]
LDFLAGS = [f"-L{LIBD}", "-lcusp_mi355x", f"-Wl,-rpath,{LIBD}", "-Wl,-rpath,/opt/rocm/lib"]


def _call(L, suf, rows, cols, nnz, Ap, Aj, Ax, k, X, xrs, xcs, Y, yrs, ycs, acc=0, cfg=None):
    fn = getattr(L, f"cmi_spmm_csr_{suf}")
    return fn(rows, cols, nnz, Ap, Aj, Ax, k, X, xrs, xcs, Y, yrs, ycs, acc, cfg, None)


def test_spmm_symbols_are_exported(cmi):
    L = cmi.lib()
    for suf in ("f64", "f32"):
        assert hasattr(L, f"cmi_spmm_csr_{suf}")
    assert cmi.CSR_SPMM_ROWS == 40 and cmi.CSR_SPMM_COLS == 41
    assert callable(cmi.spmm_csr)


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_spmm_argument_validation_without_a_device(cmi, suf):
    L = cmi.lib()
    # host buffers only: every call below must be refused (or succeed with nothing to do) before any device call
    s = 8 if suf == "f64" else 4
    buf = (ctypes.c_char * (1 << 16))()
    base = ctypes.addressof(buf)
    Ap, Aj, Ax, X, Y = base, base + 1024, base + 2048, base + 8192, base + 32768
    # negative sizes, int32 limits, null arrays
    assert _call(L, suf, -1, 4, 0, Ap, Aj, Ax, 2, X, 2, 1, Y, 2, 1) == 1
    assert b"negative" in L.cmi_last_error()
    assert _call(L, suf, 4, 4, 0, Ap, Aj, Ax, -3, X, 2, 1, Y, 2, 1) == 1
    assert b"negative" in L.cmi_last_error()
    assert _call(L, suf, 2**31, 4, 0, Ap, Aj, Ax, 2, X, 2, 1, Y, 2, 1) == 1
    assert _call(L, suf, 4, 4, 6, Ap, None, Ax, 2, X, 2, 1, Y, 2, 1) == 1
    assert b"null" in L.cmi_last_error()
    assert _call(L, suf, 4, 4, 6, Ap, Aj, Ax, 2, None, 2, 1, Y, 2, 1) == 1
    assert _call(L, suf, 4, 4, 6, Ap, Aj, Ax, 2, X, 2, 1, None, 2, 1) == 1
    # a stride pair with no unit stride; rows that would overlap (row stride below k / column stride below the rows)
    assert _call(L, suf, 4, 4, 6, Ap, Aj, Ax, 2, X, 2, 2, Y, 2, 1) == 1
    assert b"X strides" in L.cmi_last_error()
    assert _call(L, suf, 4, 4, 6, Ap, Aj, Ax, 3, X, 2, 1, Y, 3, 1) == 1
    assert b"X strides" in L.cmi_last_error()
    assert _call(L, suf, 4, 4, 6, Ap, Aj, Ax, 3, X, 3, 1, Y, 1, 3) == 1
    assert b"Y strides" in L.cmi_last_error()
    assert _call(L, suf, 4, 4, 6, Ap, Aj, Ax, 3, X, 3, 1, Y, -3, 1) == 1
    # Y overlapping X (the last row of X reaches into Y)
    assert _call(L, suf, 4, 4, 6, Ap, Aj, Ax, 2, X, 2, 1, X + 6 * s, 2, 1) == 1
    assert b"overlaps" in L.cmi_last_error()
    assert _call(L, suf, 4, 4, 6, Ap, Aj, Ax, 2, X, 1, 4, X + 4 * s, 1, 4) == 1
    # nothing to do: k = 0, zero rows -- success without a device (even with null arrays)
    assert _call(L, suf, 4, 4, 6, Ap, Aj, Ax, 0, None, 0, 1, None, 0, 1) == 0
    assert _call(L, suf, 0, 4, 0, None, None, None, 3, None, 3, 1, None, 3, 1) == 0
    with pytest.raises(cmi.CmiError) as e:
        cmi.check(_call(L, suf, 4, 4, 6, Ap, Aj, Ax, 2, X, 2, 2, Y, 2, 1))
    assert e.value.status == 1


def test_spmm_python_refuses_host_tensors_and_dtype_mismatch(cmi):
    import torch
    Ap = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(TypeError):
        cmi.spmm_csr(2, 2, Ap, Ap[:0], torch.zeros(0, dtype=torch.float64), torch.zeros(2, 2, dtype=torch.float64),
                     torch.zeros(2, 2, dtype=torch.float64))


def _golden_irregular_mtx(path):
    d = np.load(os.path.join(GOLDEN, "irregular_1500x1237.npz"))
    Ap, Aj, Ax = d["f64_Ap"], d["f64_Aj"], d["f64_Ax"]
    rows, cols = int(d["rows"]), int(d["cols"])
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write(f"{rows} {cols} {len(Aj)}\n")
        for i in range(rows):
            for jj in range(Ap[i], Ap[i + 1]):
                f.write(f"{i + 1} {Aj[jj] + 1} {float(Ax[jj])!r}\n")


def test_spmm_host_layer_program(cmi, tmp_path):
    exe = tmp_path / "test_spmm_host"
    r = subprocess.run(["g++", *CXXFLAGS, os.path.join(SPMM, "test_spmm_host.cpp"), "-o", str(exe), *LDFLAGS],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    mtx = tmp_path / "irregular.mtx"
    _golden_irregular_mtx(str(mtx))
    r = subprocess.run([str(exe), str(mtx)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "8 tests, 0 failed" in r.stdout


@pytest.mark.parametrize("snippet,needle", [
    ("cusp::coo_matrix<int, double, cusp::host_memory> A(2, 2, 0); cusp::array2d<double, cusp::host_memory> X(2, 2), Y(2, 2);"
     " cusp::multiply(A, X, Y);", "implemented for CSR matrices only"),
    ("cusp::csr_matrix<int, double, cusp::host_memory> A(2, 2, 0); cusp::array2d<double, cusp::host_memory> X(2, 2);"
     " cusp::array1d<double, cusp::host_memory> y(2); cusp::multiply(A, X, y);", "mixed array1d / array2d"),
])
def test_spmm_refused_at_compile_time(tmp_path, snippet, needle):
    src = tmp_path / "bad.cpp"
    src.write_text("#include <cusp/coo_matrix.h>\n#include <cusp/csr_matrix.h>\n#include <cusp/multiply.h>\n"
                   f"int main() {{ {snippet} return 0; }}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode != 0
    assert needle in r.stderr, r.stderr[-2000:]
