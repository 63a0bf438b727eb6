"""CPU tests (-m "not gpu") of cusp::eigen: the C-ABI symbols of csrc/eigen.hip and their argument checks (no device call
happens before a bad argument is refused), the hash of cusp/detail/random_hash.h against tests/eigen_refs.py, and the
header layer on host_memory built from tests/eigen/test_eigen_host.cpp (plain, and as a stand-alone program under
AddressSanitizer + UndefinedBehaviorSanitizer)."""
import ctypes
import os
import subprocess

import pytest

import eigen_refs as E
from conftest import ROOT

INC = os.path.join(ROOT, "cusp-autotuned_amd", "include")
LIBD = os.path.join(ROOT, "cusp-autotuned_amd", "lib")
SRC = os.path.join(ROOT, "tests", "eigen")
# the flags of tests/cpp/Makefile
CXXFLAGS = ["-std=c++17", "-O1", "-g", "-fopenmp", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off", f"-I{INC}",
            f"-I{os.path.join(ROOT, 'tests', 'cpp')}"]
LDFLAGS = [f"-L{LIBD}", "-lcusp_mi355x", f"-Wl,-rpath,{LIBD}", "-Wl,-rpath,/opt/rocm/lib"]
HOST_TESTS = "24 tests, 0 failed"
ENTRIES = ("cmi_csr_abs_row_sums", "cmi_ell_abs_row_sums", "cmi_dia_abs_row_sums", "cmi_random_fill", "cmi_blas_scal_recip")


def test_eigen_symbols_are_exported(cmi):
    L = cmi.lib()
    for name in ENTRIES:
        for suf in ("f64", "f32"):
            assert hasattr(L, f"{name}_{suf}")
    assert hasattr(L, "cmi_random_hash") and hasattr(L, "cmi_random_unit_f64") and hasattr(L, "cmi_random_unit_f32")
    for fn in ("csr_abs_row_sums", "ell_abs_row_sums", "dia_abs_row_sums", "random_fill", "blas_scal_recip", "abs_row_sums", "disks_spectral_radius"):
        assert callable(getattr(cmi, fn))
    assert cmi.version() == 400   # unchanged: callers find the feature by symbol


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_eigen_argument_validation_without_a_device(cmi, suf):
    """Host buffers only: every call below is refused (or succeeds with nothing to do) before any device call."""
    L = cmi.lib()
    buf = (ctypes.c_char * (1 << 16))()
    base = ctypes.addressof(buf)
    base += -base % 16
    Ap, Ax, out, off = base, base + 4096, base + 8192, base + 12288
    csr = getattr(L, f"cmi_csr_abs_row_sums_{suf}")
    assert csr(-1, Ap, Ax, out, 0, None) == 1 and b"negative" in L.cmi_last_error()
    assert csr(2**31, Ap, Ax, out, 0, None) == 1 and b"exceeds" in L.cmi_last_error()
    assert csr(4, None, Ax, out, 0, None) == 1 and b"null" in L.cmi_last_error()
    assert csr(4, Ap, Ax, None, 0, None) == 1 and b"null" in L.cmi_last_error()
    assert csr(4, Ap, Ax + 1, out, 0, None) == 1 and b"aligned" in L.cmi_last_error()
    assert csr(0, None, None, None, 0, None) == 0
    ell = getattr(L, f"cmi_ell_abs_row_sums_{suf}")
    # (rows, cols, width, pitch, Aj, Ax, row_lengths, row_sums, accumulate, stream)
    assert ell(-1, 4, 2, 4, None, Ax, None, out, 0, None) == 1 and b"negative" in L.cmi_last_error()
    assert ell(4, 4, -2, 4, None, Ax, None, out, 0, None) == 1 and b"negative" in L.cmi_last_error()
    assert ell(4, 4, 2, 3, None, Ax, None, out, 0, None) == 1 and b"pitch" in L.cmi_last_error()
    assert ell(4, 4, 2, 4, None, None, None, out, 0, None) == 1 and b"null" in L.cmi_last_error()
    assert ell(4, 4, 2, 4, None, Ax, None, None, 0, None) == 1 and b"null" in L.cmi_last_error()
    assert ell(0, 0, 0, 0, None, None, None, None, 0, None) == 0
    dia = getattr(L, f"cmi_dia_abs_row_sums_{suf}")
    # (rows, cols, diagonals, pitch, offsets, values, row_sums, accumulate, stream)
    assert dia(4, -1, 2, 4, off, Ax, out, 0, None) == 1 and b"negative" in L.cmi_last_error()
    assert dia(4, 4, 2, 3, off, Ax, out, 0, None) == 1 and b"pitch" in L.cmi_last_error()
    assert dia(4, 4, 2, 4, None, Ax, out, 0, None) == 1 and b"null" in L.cmi_last_error()
    assert dia(4, 4, 2, 4, off, None, out, 0, None) == 1 and b"null" in L.cmi_last_error()
    assert dia(4, 4, 2, 4, off, Ax, None, 0, None) == 1 and b"null" in L.cmi_last_error()
    assert dia(0, 4, 2, 0, None, None, None, 0, None) == 0
    fill = getattr(L, f"cmi_random_fill_{suf}")
    assert fill(-1, 0, out, None) == 1 and b"negative" in L.cmi_last_error()
    assert fill(3, 0, None, None) == 1 and b"null" in L.cmi_last_error()
    assert fill(0, 5, None, None) == 0
    recip = getattr(L, f"cmi_blas_scal_recip_{suf}")
    # (n, s_dev, s_is_squared_norm, x, s_out_dev, stream)
    assert recip(-1, Ax, 0, out, None, None) == 1 and b"negative" in L.cmi_last_error()
    assert recip(3, None, 0, out, None, None) == 1 and b"null" in L.cmi_last_error()
    assert recip(3, Ax, 1, None, None, None) == 1 and b"null" in L.cmi_last_error()
    assert recip(3, Ax, 1, out, Ax, None) == 1 and b"s_out_dev is s_dev" in L.cmi_last_error()
    assert recip(3, Ax, 0, out + 2, None, None) == 1 and b"aligned" in L.cmi_last_error()
    assert recip(0, None, 0, None, None, None) == 0
    with pytest.raises(cmi.CmiError) as e:
        cmi.check(csr(-1, Ap, Ax, out, 0, None))
    assert e.value.status == 1


def test_eigen_python_refuses_host_tensors(cmi):
    import torch
    Ap = torch.zeros(3, dtype=torch.int32)
    v = torch.zeros(2, dtype=torch.float64)
    with pytest.raises(TypeError):
        cmi.csr_abs_row_sums(2, Ap, v, v.clone())
    with pytest.raises(TypeError):
        cmi.random_fill(v)
    with pytest.raises(TypeError):
        cmi.blas_scal_recip(v[:1], v)


def test_the_hash_is_the_refs_hash(cmi, tmp_path):
    """cmi_random_hash / cmi_random_unit_* (host functions of the library) and the inline definition of cusp/detail/random_hash.h they and
    the kernel are compiled from: the values of tests/eigen_refs.py, bit for bit."""
    L = cmi.lib()
    src = tmp_path / "hash.cpp"
    src.write_text('#include <cstdio>\n#include <cusp/detail/random_hash.h>\nint main() {\n'
                   '  const unsigned long long seeds[2] = {0, 12345};\n'
                   '  for (int s = 0; s < 2; s++) for (unsigned long long i = 0; i < 70; i += 23) {\n'
                   '    const uint64_t h = cusp::detail::random_hash(i, seeds[s]);\n'
                   '    std::printf("%llu %llu %llx %a %a\\n", seeds[s], i, (unsigned long long)h, cusp::detail::random_unit(h, (double *)0),\n'
                   '                (double)cusp::detail::random_unit(h, (float *)0)); }\n'
                   '  return 0; }\n')
    exe = tmp_path / "hash"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", f"-I{INC}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True).stdout.split("\n")[:-1]
    assert len(out) == 8
    for line in out:
        seed, i, h, d, f = line.split()
        want = E.random_hash(int(i), int(seed))
        assert int(h, 16) == want == L.cmi_random_hash(int(i), int(seed))
        assert float.fromhex(d) == (want >> 11) * 2.0 ** -53 == L.cmi_random_unit_f64(want)
        assert float.fromhex(f) == (want >> 40) * 2.0 ** -24 == L.cmi_random_unit_f32(want)
        assert 0 <= float.fromhex(d) < 1 and 0 <= float.fromhex(f) < 1
    assert L.cmi_random_unit_f64(2**64 - 1) < 1 and L.cmi_random_unit_f32(2**64 - 1) < 1


def _build(tmp_path, name, extra=()):
    exe = tmp_path / name
    r = subprocess.run(["g++", *CXXFLAGS, *extra, os.path.join(SRC, "test_eigen_host.cpp"), "-o", str(exe), *LDFLAGS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_eigen_host_layer_program(cmi, tmp_path):
    r = subprocess.run([str(_build(tmp_path, "test_eigen_host"))], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert HOST_TESTS in r.stdout


def test_eigen_host_layer_program_under_sanitizers(cmi, tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined (host code only; leak checking off: the HIP
    runtime the library links keeps process-lifetime allocations)."""
    exe = _build(tmp_path, "test_eigen_host_asan", ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"))
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert HOST_TESTS in r.stdout and "runtime error" not in r.stderr


def test_one_argument_polynomial_stays_a_compile_time_error_beside_the_factory(tmp_path):
    """cusp/relaxation/chebyshev.h adds the factory and leaves the class as it was: polynomial(A) does not compile, the factory does."""
    for body, ok in (("cusp::relaxation::polynomial<double, cusp::host_memory> M(A);", False),
                     ("auto M = cusp::relaxation::make_chebyshev_polynomial<double, cusp::host_memory>(A); (void)M;", True)):
        src = tmp_path / f"poly_{int(ok)}.cpp"
        src.write_text("#include <cusp/csr_matrix.h>\n#include <cusp/relaxation/chebyshev.h>\n"
                       f"int main() {{ cusp::csr_matrix<int, double, cusp::host_memory> A; {body} return 0; }}\n")
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", f"-I{INC}", str(src)], capture_output=True, text=True)
        assert (r.returncode == 0) == ok, r.stderr[-2000:]
