"""CPU tests (-m "not gpu") of cusp::eigen::lobpcg on host_memory: tests/lobpcg/test_lobpcg_host.cpp built plain and as a stand-alone
program under AddressSanitizer + UndefinedBehaviorSanitizer (exactly as tests/test_eigen_host.py builds its program); the solver cases
against the exact eigenvalues (numpy.linalg.eigvalsh of the dense matrix) and the iteration counts of the numpy restatement of
tests/lobpcg_refs.py; the header's small dense solver bit for bit against its restatement."""
import os
import subprocess

import numpy as np
import pytest

import lobpcg_refs as R
from conftest import ROOT
from test_eigen_host import CXXFLAGS, LDFLAGS
from test_lobpcg_refs import small_pairs

SRC = os.path.join(ROOT, "tests", "lobpcg")
HOST_TESTS = "15 tests, 0 failed"


def build(tmp_path, source, name, extra=()):
    exe = tmp_path / name
    r = subprocess.run(["g++", *CXXFLAGS, *extra, os.path.join(SRC, source), "-o", str(exe), *LDFLAGS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def parse_cases(stdout):
    """`case <which> <kind> <nx>x<ny> <type> <tolerance> <precond> run <run> iterations <n> converged <0|1> lambda <%a> xnorm <%a> residual <%a>`"""
    out = []
    for line in stdout.split("\n"):
        if not line.startswith("case "):
            continue
        f = line.split()
        nx, ny = (int(v) for v in f[3].split("x"))
        out.append({"case": (f[1], f[2], nx, ny, f[4], float(f[5]), f[6]), "run": f[8], "iterations": int(f[10]), "converged": f[12] == "1",
                    "lambda": float.fromhex(f[14]), "xnorm": float.fromhex(f[16]), "residual": float.fromhex(f[18])})
    return out


_reference_counts = {}


def reference_count(case):
    """The iteration count of the restated loop on this case, computed once."""
    if case not in _reference_counts:
        _reference_counts[case] = R.run_case(case)[2].iteration_count
    return _reference_counts[case]


def check_case(row):
    """The bars of every solver case, host or device."""
    which, kind, nx, ny, tname, tol, precond = case = row["case"]
    exact = R.exact_eigenvalue(kind, nx, ny, which == "largest")
    count = reference_count(case)
    print(case, row["run"], "iterations", row["iterations"], "restatement", count, "eigenvalue error", abs(row["lambda"] - exact), "residual / tolerance",
          row["residual"] / tol)
    assert row["converged"], row
    assert abs(row["lambda"] - exact) <= tol, (row, exact)
    assert row["residual"] <= 2 * tol, row
    assert abs(row["xnorm"] - 1) <= 1e-5, row
    assert row["iterations"] <= 1.5 * count and row["iterations"] <= min(nx * ny, R.LIMIT), (row, count)


@pytest.fixture(scope="module")
def host_program(cmi, tmp_path_factory):
    return build(tmp_path_factory.mktemp("lobpcg"), "test_lobpcg_host.cpp", "test_lobpcg_host")


def test_lobpcg_host_layer_program(host_program):
    r = subprocess.run([str(host_program)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert HOST_TESTS in r.stdout


def test_lobpcg_host_layer_program_under_sanitizers(cmi, tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined (host code only; leak checking off: the HIP
    runtime the library links keeps process-lifetime allocations)."""
    exe = build(tmp_path, "test_lobpcg_host.cpp", "test_lobpcg_host_asan", ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert HOST_TESTS in r.stdout and "runtime error" not in r.stderr
    r = subprocess.run([str(exe), "cases"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and len(parse_cases(r.stdout)) == len(R.CASES), r.stderr[-4000:]


def test_host_solver_cases(host_program):
    """Every case of the table: converged, |S[0] - lambda_exact| <= tolerance, the true residual <= 2 x tolerance, | ||x|| - 1 | <= 1e-5, at most
    1.5 x the restated loop's iterations (the margin covers the path difference between two correct small solvers) and at most min(N, limit)."""
    r = subprocess.run([str(host_program), "cases"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = parse_cases(r.stdout)
    assert [row["case"] for row in rows] == list(R.CASES) and all(row["run"] == "host" for row in rows)
    for row in rows:
        check_case(row)
        # the host path and the restatement form the same operations in the same order, the small solver included: the same count
        assert row["iterations"] == reference_count(row["case"]), row


def test_small_solver_is_its_restatement_bit_for_bit(host_program, tmp_path):
    """cusp::detail::sygv_small on the pairs of test_lobpcg_refs.py (B's smallest eigenvalue down to 1e-6) and on matrices that are not positive
    definite: the same answer, the same bits as lobpcg_refs.sygv_small."""
    pairs = [(n, A, B) for _, n, A, B in small_pairs()]
    pairs += [(2, np.array([[1.0, 0.5], [0.5, 2.0]]), np.array(B)) for B in ([[1.0, 1.5], [1.5, 1.0]], [[1.0, 1.0], [1.0, 1.0]], [[0.0, 0.0], [0.0, 1.0]])]
    pairs += [(3, np.diag([9.0, 1.0, 4.0]), np.array([[1.0, 0.1, 1.5], [0.1, 1.0, 0.2], [1.5, 0.2, 1.0]])), (3, np.diag([9.0, 1.0, 4.0]), np.eye(3))]
    path = tmp_path / "pairs.txt"
    path.write_text("".join(f"{n} " + " ".join(float(x).hex() for x in np.r_[A.ravel(), B.ravel()]) + "\n" for n, A, B in pairs))
    r = subprocess.run([str(host_program), "sygv", str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(pairs)
    refused = 0
    for line, (n, A, B) in zip(lines, pairs):
        f = line.split()
        ok, w, Z = R.sygv_small(n, A, B)
        assert (f[0] == "1") == ok, (n, A, B)
        refused += not ok
        if ok:
            got = np.array([float.fromhex(x) for x in f[1:]])
            assert got.tobytes() == np.r_[w, Z.ravel()].tobytes(), (n, A, B)
    assert refused == 4
