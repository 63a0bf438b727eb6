"""CPU tests (-m "not gpu") of cusp::krylov::cg_m and bicgstab_m on host_memory: tests/multishift/test_multishift_host.cpp built plain and
as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer (exactly as tests/test_eigen_host.py builds its program), the
solutions of the host path bit for bit against the numpy restatement of tests/multishift_refs.py, and the reference's own example
programs compiled unchanged against the header layer (skipped where the reference tree is absent)."""
import os
import subprocess

import numpy as np
import pytest

import multishift_refs as R
from conftest import ROOT
from test_eigen_host import CXXFLAGS, LDFLAGS

SRC = os.path.join(ROOT, "tests", "multishift")
HOST_TESTS = "13 tests, 0 failed"
REFERENCE = os.environ.get("REFERENCE", "/root/reference")   # oracle/Makefile's default


def _build(tmp_path, name, extra=()):
    exe = tmp_path / name
    r = subprocess.run(["g++", *CXXFLAGS, *extra, os.path.join(SRC, "test_multishift_host.cpp"), "-o", str(exe), *LDFLAGS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def host_program(cmi, tmp_path_factory):
    return _build(tmp_path_factory.mktemp("multishift"), "test_multishift_host")


def test_multishift_host_layer_program(host_program):
    r = subprocess.run([str(host_program)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert HOST_TESTS in r.stdout


def test_multishift_host_layer_program_under_sanitizers(cmi, tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined (host code only; leak checking off: the HIP
    runtime the library links keeps process-lifetime allocations)."""
    exe = _build(tmp_path, "test_multishift_host_asan", ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"))
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert HOST_TESTS in r.stdout and "runtime error" not in r.stderr


def test_host_solutions_are_the_refs_bit_for_bit(host_program):
    """`test_multishift_host bits` prints x of both solvers on Poisson 10 x 10 and 7 x 5 in float and double as %a: the same bits and the same
    iteration counts as the numpy restatement (sequential dots, the CSR loop, every expression in the reference's association)."""
    out = subprocess.run([str(host_program), "bits"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    cases, cur = [], None
    for line in out.stdout.split("\n"):
        if line.startswith("case "):
            _, solver, tname, grid, _, its = line.split()
            cur = (solver, tname, tuple(int(v) for v in grid.split("x")), int(its), [])
            cases.append(cur)
        elif line:
            cur[4].append(float.fromhex(line))
    assert len(cases) == 8
    sigma = (0.1, 0.5, 1.0, 5.0)
    for solver, tname, (nx, ny), its, values in cases:
        T = {"f32": np.float32, "f64": np.float64}[tname]
        A = R.poisson5pt(nx, ny, T)
        want, mon = getattr(R, solver)(A, np.ones(A[0], T), np.array(sigma, T), 100, 1e-6 if T is np.float32 else 1e-10)
        got = np.array(values, np.float64).astype(T)
        assert np.array_equal(got.astype(np.float64), np.array(values))       # the printed doubles are values of T
        assert its == mon.iteration_count, (solver, tname, nx, ny)
        assert got.tobytes() == want.reshape(-1).tobytes(), (solver, tname, nx, ny)


@pytest.mark.parametrize("example", ["cg_m", "bicgstab_m"])
def test_reference_examples_compile_unchanged(cmi, tmp_path, example):
    """examples/Solvers/{cg_m,bicgstab_m}.cu of the reference against this header layer, with the flags oracle/Makefile uses for its
    examples; compile and link only, into tmp_path."""
    src = os.path.join(REFERENCE, "examples", "Solvers", example + ".cu")
    if not os.path.exists(src):
        pytest.skip("the reference tree is not present")
    inc = os.path.join(ROOT, "cusp-autotuned_amd", "include")
    libd = os.path.join(ROOT, "cusp-autotuned_amd", "lib")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-x", "c++", f"-I{inc}", src, "-x", "none", "-o", str(tmp_path / example), f"-L{libd}", "-lcusp_mi355x",
                        f"-Wl,-rpath,{libd}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
