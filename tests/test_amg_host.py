"""CPU tests (-m "not gpu") of the header layer's smoothed aggregation on host_memory: tests/amg/test_amg_host.cpp built once
plainly and once as a stand-alone program under the address and undefined-behaviour sanitizers, the hierarchy it builds with a
supplied rho per level against tests/amg_refs.py -- aggregates, sizes and entry counts identical, values bit for bit -- and the
compile-time refusals."""
import os
import subprocess

import numpy as np
import pytest

import amg_refs as R
import spgemm_refs as SR
from conftest import ROOT, GOLDEN
from special_values import same_bits

INC = os.path.join(ROOT, "cusp-autotuned_amd", "include")
LIBD = os.path.join(ROOT, "cusp-autotuned_amd", "lib")
SRC = os.path.join(ROOT, "tests", "amg")
# the flags of tests/cpp/Makefile
CXXFLAGS = ["-std=c++17", "-O1", "-g", "-fopenmp", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off", f"-I{INC}",
            f"-I{os.path.join(ROOT, 'tests', 'cpp')}", f"-DGOLDEN_DIR=\"{GOLDEN}\""]
LDFLAGS = [f"-L{LIBD}", "-lcusp_mi355x", f"-Wl,-rpath,{LIBD}", "-Wl,-rpath,/opt/rocm/lib"]
TESTS = "6 tests, 0 failed"


@pytest.fixture(scope="module")
def host_program(cmi, tmp_path_factory):
    exe = tmp_path_factory.mktemp("amg") / "test_amg_host"
    r = subprocess.run(["g++", *CXXFLAGS, os.path.join(SRC, "test_amg_host.cpp"), "-o", str(exe), *LDFLAGS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(exe)


def test_amg_host_layer_program(host_program):
    r = subprocess.run([host_program], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert TESTS in r.stdout


def test_amg_host_layer_program_under_sanitizers(cmi, tmp_path):
    # host code with its own main, built stand-alone with the sanitizers: their runtime is linked in, nothing is preloaded
    exe = tmp_path / "test_amg_host_san"
    r = subprocess.run(["g++", *CXXFLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(SRC, "test_amg_host.cpp"),
                        "-o", str(exe), *LDFLAGS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert TESTS in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def _parse_levels(text, dtype):
    lines = iter(text.strip().split("\n"))
    count = int(next(lines).split()[1])

    def csr(tag):
        name, m, n, nnz = next(lines).split()
        assert name == tag
        m, n, nnz = int(m), int(n), int(nnz)
        Ap = np.array(next(lines).split(), np.int32)
        ent = [next(lines).split() for _ in range(nnz)]
        Aj = np.array([int(e[0]) for e in ent], np.int32)
        bits = np.array([int(e[1], 16) for e in ent], np.uint64)
        Ax = bits.view(np.float64) if dtype == np.float64 else bits.astype(np.uint32).view(np.float32)
        assert len(Ap) == m + 1
        return m, n, Ap, Aj, Ax

    out = []
    for l in range(count):
        A = csr("A")
        if l + 1 == count:
            out.append((A, None, None))
            break
        assert next(lines).startswith("aggregates")
        agg = np.array(next(lines).split(), np.int32)
        out.append((A, agg, csr("P")))
    return out


def reference_levels(dtype, nx, ny, min_level_size, rhos, theta=0.0, matrix=None):
    if matrix is None:
        N, Ap, Aj, Ax = SR.poisson5pt(nx, ny, dtype)
        matrix = (N, N, Ap, Aj, Ax)
    A, B, out = matrix, np.ones(matrix[0], dtype), []
    while A[0] > min_level_size and len(out) < len(rhos):
        n = A[0]
        S = R.strength(n, *A[2:], theta)
        agg, _ = R.standard_aggregate(n, S[0], S[1])
        na = int(agg.max()) + 1
        Tp, Tj, Tx, Rr = R.fit(agg, B, na)
        P = R.smooth_prolongator(A, (n, na, Tp, Tj, Tx), rhos[len(out)])
        out.append((A, agg, P))
        A, B = R.galerkin((na, n, *SR.transpose(*P)), A, P), Rr
    return out + [(A, None, None)]


def same_csr(got, want, what):
    assert got[:2] == want[:2], what
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), f"{what}: structure differs"
    same_bits(got[4], want[4], what)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("case", [(100, 100, 500, (1.9995162822919836, 1.4076716791442256)), (10, 10, 20, (1.9, 1.5, 1.4))])
def test_host_hierarchy_equals_the_references_level_by_level(host_program, dtype, case):
    nx, ny, min_level_size, rhos = case
    r = subprocess.run([host_program, "--levels", "f64" if dtype == np.float64 else "f32", str(nx), str(ny), str(min_level_size), *(repr(v) for v in rhos)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got, want = _parse_levels(r.stdout, dtype), reference_levels(dtype, nx, ny, min_level_size, rhos)
    assert len(got) == len(want) >= 2
    if nx == 100:
        assert [g[0][0] for g in got] == [10000, 1700, 192] and [len(g[0][3]) for g in got] == [49600, 14928, 1692]
    for l, (g, w) in enumerate(zip(got, want)):
        same_csr(g[0], w[0], f"A of level {l}")
        if w[1] is not None:
            assert np.array_equal(g[1], w[1]), f"aggregates of level {l}"
            same_csr(g[2], w[2], f"P of level {l}")


def write_mtx(path, n, Ap, Aj, Ax):
    with open(path, "w") as f:
        f.write(f"%%MatrixMarket matrix coordinate real general\n{n} {n} {len(Aj)}\n")
        for i, j, v in zip(R.csr_rows(Ap), Aj, Ax):
            f.write(f"{i + 1} {j + 1} {float(v)!r}\n")              # repr round-trips the bits (a float32 is exact as a double)


def irregular_square(golden_irregular, dtype):
    """The square part (the leading 1237 rows) of the irregular fixture, every row ordered by column (stable)."""
    p = "f64" if dtype == np.float64 else "f32"
    n = int(golden_irregular["cols"])
    Ap, Aj, Ax = golden_irregular[p + "_Ap"][:n + 1].astype(np.int32), golden_irregular[p + "_Aj"], golden_irregular[p + "_Ax"]
    Aj, Ax = Aj[:Ap[n]], Ax[:Ap[n]].astype(dtype)
    order = np.lexsort((Aj, R.csr_rows(Ap)))                           # stable: a repeated column keeps its storage order
    return n, Ap, Aj[order].astype(np.int32), Ax[order]


def compare_levels(got, want):
    assert len(got) == len(want) >= 2
    for l, (g, w) in enumerate(zip(got, want)):
        same_csr(g[0], w[0], f"A of level {l}")
        if w[1] is not None:
            assert np.array_equal(g[1], w[1]), f"aggregates of level {l}"
            same_csr(g[2], w[2], f"P of level {l}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("theta", [0.0, 0.25])
def test_host_hierarchy_on_the_irregular_fixture_equals_the_references(host_program, golden_irregular, tmp_path, dtype, theta):
    """The square part of irregular_1500x1237: a pattern that is not symmetric, rows without a diagonal, repeated columns.  Aggregates
    (isolated nodes are -1 and give empty rows of T), sizes and entry counts identical, values bit for bit with rho supplied."""
    n, Ap, Aj, Ax = irregular_square(golden_irregular, dtype)
    path = tmp_path / "irregular_square.mtx"
    write_mtx(path, n, Ap, Aj, Ax)
    rhos, min_level_size = (1.7, 1.5, 1.4, 1.3), 40
    r = subprocess.run([host_program, "--levels-mtx", "f64" if dtype == np.float64 else "f32", str(path), repr(theta), str(min_level_size), *(repr(v) for v in rhos)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = _parse_levels(r.stdout, dtype)
    want = reference_levels(dtype, 0, 0, min_level_size, rhos, theta=theta, matrix=(n, n, Ap, Aj, Ax))
    print([(g[0][0], len(g[0][3])) for g in got], "unaggregated on level 0:", int((got[0][1] < 0).sum()))
    compare_levels(got, want)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_hierarchy_on_the_5pt_10x10_fixture_equals_the_references(host_program, dtype):
    from conftest import coo_to_csr, read_mtx
    path = os.path.join(GOLDEN, "5pt_10x10.mtx")
    rows, cols, I, J, V = read_mtx(path)
    A = (rows, cols, *coo_to_csr(rows, I, J, V, dtype))
    rhos = (1.9, 1.5, 1.4)
    r = subprocess.run([host_program, "--levels-mtx", "f64" if dtype == np.float64 else "f32", path, "0.0", "20", *(repr(v) for v in rhos)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    compare_levels(_parse_levels(r.stdout, dtype), reference_levels(dtype, 0, 0, 20, rhos, matrix=A))


@pytest.mark.parametrize("snippet,needle", [
    ("cusp::ell_matrix<int, double, cusp::host_memory> A, B, C; cusp::add(A, B, C);", "csr and coo matrices of one format"),
    ("cusp::csr_matrix<int, double, cusp::host_memory> A, B; cusp::coo_matrix<int, double, cusp::host_memory> C; cusp::subtract(A, B, C);", "csr and coo matrices of one format"),
    ("cusp::csr_matrix<int, double, cusp::host_memory> A, B; cusp::csr_matrix<int, double, cusp::device_memory> C; cusp::add(A, B, C);", "one memory space"),
    ("cusp::coo_matrix<int, double, cusp::host_memory> A, S; cusp::precond::aggregation::symmetric_strength_of_connection(A, S);", "implemented for csr matrices"),
])
def test_amg_refused_at_compile_time(tmp_path, snippet, needle):
    src = tmp_path / "bad.cpp"
    src.write_text("#include <cusp/ell_matrix.h>\n#include <cusp/precond/aggregation/smoothed_aggregation.h>\n" f"int main() {{ {snippet} return 0; }}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode != 0
    assert needle in r.stderr, r.stderr[-2000:]


def test_the_preconditioner_compiles_in_both_spaces_with_every_solver(tmp_path):
    src = tmp_path / "good.cpp"
    src.write_text("#include <cusp/precond/aggregation/smoothed_aggregation.h>\n#include <cusp/krylov/cg.h>\n#include <cusp/krylov/bicgstab.h>\n#include <cusp/krylov/gmres.h>\n"
                   "template <typename S, typename V> void f() { cusp::csr_matrix<int, V, S> A; cusp::precond::aggregation::smoothed_aggregation<int, V, S> M(A);\n"
                   "  cusp::array1d<V, S> x, b; cusp::monitor<V> m(b); cusp::krylov::cg(A, x, b, m, M); cusp::krylov::bicgstab(A, x, b, m, M); cusp::krylov::gmres(A, x, b, 10, m, M);\n"
                   "  cusp::precond::aggregation::smoothed_aggregation<int, V, cusp::host_memory> H(M); }\n"
                   "int main() { f<cusp::host_memory, double>(); f<cusp::device_memory, double>(); f<cusp::device_memory, float>(); return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
