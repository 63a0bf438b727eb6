"""CPU tests (-m "not gpu") of cusp::graph::maximal_independent_set, mis_aggregate and smoothed_aggregation::mis_aggregation on
host_memory: tests/mis/test_mis_host.cpp built once plainly and once as a stand-alone program under the address and
undefined-behaviour sanitizers; what it prints for the five formats against tests/mis_refs.py, exactly."""
import os
import subprocess

import numpy as np
import pytest

import mis_refs as M
from conftest import ROOT, GOLDEN

INC = os.path.join(ROOT, "cusp-autotuned_amd", "include")
LIBD = os.path.join(ROOT, "cusp-autotuned_amd", "lib")
SRC = os.path.join(ROOT, "tests", "mis")
# the flags of tests/cpp/Makefile
CXXFLAGS = ["-std=c++17", "-O1", "-g", "-fopenmp", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off", f"-I{INC}",
            f"-I{os.path.join(ROOT, 'tests', 'cpp')}", f"-I{os.path.join(ROOT, 'tests', 'amg')}", f"-DGOLDEN_DIR=\"{GOLDEN}\""]
LDFLAGS = [f"-L{LIBD}", "-lcusp_mi355x", f"-Wl,-rpath,{LIBD}", "-Wl,-rpath,/opt/rocm/lib"]
TESTS = "4 tests, 0 failed"
FORMATS = ["coo", "csr", "ell", "dia", "hyb"]


@pytest.fixture(scope="module")
def host_program(cmi, tmp_path_factory):
    exe = tmp_path_factory.mktemp("mis") / "test_mis_host"
    r = subprocess.run(["g++", *CXXFLAGS, os.path.join(SRC, "test_mis_host.cpp"), "-o", str(exe), *LDFLAGS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(exe)


def test_mis_host_layer_program(host_program):
    r = subprocess.run([host_program], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert TESTS in r.stdout


def test_mis_host_layer_program_under_sanitizers(cmi, tmp_path):
    # host code with its own main, built stand-alone with the sanitizers: their runtime is linked in, nothing is preloaded
    exe = tmp_path / "test_mis_host_san"
    r = subprocess.run(["g++", *CXXFLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(SRC, "test_mis_host.cpp"),
                        "-o", str(exe), *LDFLAGS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert TESTS in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def write_pattern(path, n, Ap, Aj):
    with open(path, "w") as f:
        f.write(f"%%MatrixMarket matrix coordinate real general\n{n} {n} {len(Aj)}\n")
        for i, j in zip(M.csr_rows(Ap), Aj):
            f.write(f"{i + 1} {j + 1} 1.0\n")


def parse_formats(text):
    """format -> ([(size, rounds, stencil) for k = 0..3], aggregates, mis)"""
    out = {}
    lines = iter(text.strip().split("\n"))
    ints = lambda line, tag: np.array(line.split()[1:], np.int32) if line.split()[0] == tag else None  # noqa: E731
    for line in lines:
        name = line.split()
        assert name[0] == "format"
        per_k = []
        for k in range(4):
            head = next(lines).split()
            assert head[0] == "k" and int(head[1]) == k
            per_k.append((int(head[3]), int(head[5]), ints(next(lines), "stencil")))
        out[name[1]] = (per_k, ints(next(lines), "aggregates"), ints(next(lines), "mis"))
    return out


@pytest.mark.parametrize("name", list(M.reference_graphs()))
def test_host_results_equal_the_references_in_all_five_formats(host_program, tmp_path, name):
    n, Ap, Aj = M.reference_graphs()[name]
    path = tmp_path / "pattern.mtx"
    write_pattern(path, n, Ap, Aj)
    for seed in (0, 77):
        r = subprocess.run([host_program, "--print", str(path), str(seed)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        got = parse_formats(r.stdout)
        assert sorted(got) == sorted(FORMATS)
        want_k = [M.mis(n, Ap, Aj, k, seed) for k in range(4)]
        want_agg = M.mis_aggregate(n, Ap, Aj, seed)
        for fmt in FORMATS:
            per_k, agg, mis = got[fmt]
            for k in range(4):
                size, rounds, stencil = per_k[k]
                assert np.array_equal(stencil, want_k[k][0]), (fmt, k, seed)
                assert (size, rounds) == (int(want_k[k][0].sum()), want_k[k][1]), (fmt, k, seed)
            assert np.array_equal(agg, want_agg[0]) and np.array_equal(mis, want_agg[1]), (fmt, seed)


def test_host_results_on_an_unsorted_non_symmetric_pattern(host_program, tmp_path):
    """Repeated columns, rows without a diagonal, a pattern that is not symmetric: COO and CSR keep the entries as they are."""
    n, Ap, Aj = M.non_symmetric(300, np.random.default_rng(8))
    path = tmp_path / "pattern.mtx"
    write_pattern(path, n, Ap, Aj)
    r = subprocess.run([host_program, "--print", str(path), "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = parse_formats(r.stdout)
    want_agg = M.mis_aggregate(n, Ap, Aj, 3)
    assert (want_agg[0] == -1).any()
    for fmt in FORMATS:                                         # (the graph is the SET of stored entries: the other formats agree too)
        per_k, agg, mis = got[fmt]
        for k in range(4):
            want = M.mis(n, Ap, Aj, k, 3)
            assert np.array_equal(per_k[k][2], want[0]) and per_k[k][1] == want[1], (fmt, k)
        assert np.array_equal(agg, want_agg[0]) and np.array_equal(mis, want_agg[1]), fmt


def test_mis_aggregation_hierarchy_starts_from_the_reference_aggregates(host_program):
    r = subprocess.run([host_program, "--levels", "100", "100"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    levels, aggregates = r.stdout.strip().split("\n")
    sizes = [int(v) for v in levels.split()[1:]]
    n, Ap, Aj = M.poisson5pt(100, 100)
    agg, _, count = M.mis_aggregate(n, Ap, Aj)
    assert sizes[0] == 10000 and sizes[1] == count == 1422 and len(sizes) >= 2 and sizes[-1] <= 500
    assert np.array_equal(np.array(aggregates.split()[1:], np.int32), agg)


def test_mis_headers_compile_in_both_spaces(tmp_path):
    src = tmp_path / "good.cpp"
    src.write_text("#include <cusp/coo_matrix.h>\n#include <cusp/graph/maximal_independent_set.h>\n#include <cusp/precond/aggregation/smoothed_aggregation.h>\n"
                   "template <typename S> void f() { cusp::coo_matrix<int, float, S> G; cusp::array1d<int, S> s, a, m; cusp::array1d<char, cusp::host_memory> c;\n"
                   "  size_t k = 2; cusp::graph::maximal_independent_set(G, s); cusp::graph::maximal_independent_set(G, c, k); cusp::graph::maximal_independent_set(cusp::hip::par, G, s, k);\n"
                   "  cusp::precond::aggregation::mis_aggregate(G, a, m); cusp::precond::aggregation::mis_aggregate(G, a);\n"
                   "  cusp::precond::aggregation::smoothed_aggregation<int, float, S> M; M.mis_aggregation = true; M.initialize(G);\n"
                   "  cusp::precond::aggregation::smoothed_aggregation<int, float, cusp::host_memory> H(M); }\n"
                   "int main() { f<cusp::host_memory>(); f<cusp::device_memory>(); return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
